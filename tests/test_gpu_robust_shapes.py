"""The robust (conic) kernels -- group_robust_kernel<D, L> at 1..16 dof, robust_solve_kernel for everything else -- at the shapes,
dofs and limits that tests/test_gpu_robust.py never reaches: all of its problems are make_synthetic_batch (four segments, shared
breakpoints, a uniform shared grid, sd_start = None, ordinary limits, B <= 300).

There is no reference solver for this path (ECOS is absent), so the authorities are the two the project has: the C restatement of
the kernels' method (oracle.robust_solve_batch), bit for bit on EVERY trajectory -- status, K, sd2, u, and X when asked for, NaNs
coinciding, no tolerance -- and the independent conic solver (oracle/robust_independent.py) at the project's bars, K and X to 1e-7.

1. every dof instantiation 1..16: shared uniform and per-trajectory non-uniform grids, both discretisations, with and without X,
   non-zero sd_start / sd_end on 30 % of the trajectories; the lane kernel (variant=1) against the automatic choice;
2. the block geometries of group_launch_geometry that B <= 300 never leaves (128 and 256 threads, a ragged last block), and the
   benchmark's own C4 batch with N cut to 20;
3. both sides of the LDS limit of the spline table, where robust_launch_group hands over to the lane kernel;
4. 17..32 dof (the lane kernel through !group_supported);
5. single trajectories, N = 1 and 2, batches one off a block's worth of groups, the empty batch;
6. the independent solver on the new shape classes (CPU twin: tests/test_oracle_robust_independent.py, 1e-9);
7. device tensors in, device tensors out;
8. which kernel ran, from a kernel trace of a child process;
9. limits at the edge of the number range (tests/solver_support.py::extreme_limit_batch), and: acceleration limits
   written as 1e300 x the ordinary ones give the bits of limits written as +-inf.

Part 9 found a defect: rob_row_interval squared m = b x + c, which overflows from |m| ~ 1.3e154, and the +inf root turned a row that
is slack by 1e300 into u <= -inf -- "no limit" written as 1e300 made every trajectory uncontrollable while +-inf worked (the NaN it
produces is skipped by the comparisons).  Trajectories the restatement solves per kind, of 16 each, in the part 9 batches
(d, N) = (7, 24) | (12, 16) | (3, 20), each as Interpolation / Collocation:

    vinf, ainf, ainf_one, vhuge   16/16 | 16/16 | 16/16          vsub, vtiny   11/11 | 11/11 | 11/11
    still, shifted                16/16 | 15/15 | 16/16          plain         16/16 | 15/16 | 16/16
    vneg                           0/1  |  1/1  |  2/2           inverted       0/0  |  0/0  |  0/0
    ahuge      before the fix      0/0  |  0/0  |  0/0           mix  before    0/0  |  0/0  |  0/0
               with it            16/16 | 16/16 | 16/16               with it  11/11 | 11/11 | 11/11

(`mix` holds a vsub joint: 11 of 16, as vsub.)  The A < 0 and A == 0 branches of rob_row_interval meet the same overflow and degrade
to "row absent" for m < 0, which is right: the `slow` cases of the 1e300-against-inf test were green before the fix as well.

RUN TIME: one run on an MI355X, of this module alone (`pytest tests/test_gpu_robust_shapes.py -m gpu --durations=40`): 56 passed in
12.96 s by pytest's own figure, session set-up included; the traced child of part 8 took 3.19 s, every other test between 0.06 s
and 0.39 s (part 1: 0.06 s at 2 dof .. 0.39 s at 16 dof -- its batches are 96 x d x 48).  That run predates one change that does
not touch what the tests compute: the problem builders now in tests/robust_shapes.py were part of this module, and part 4 had no
bar on the solved share.  The module has not been timed since, nor beside the rest of `-m gpu`.
"""
import numpy as np
import pytest

from tests.robust_shapes import (ELL, EXTREME_SHAPES, RELAXED_CASES, as_checker_data, block_threads, check_extreme_counts, check_relaxed_twins,
                                 extreme_case, inf_twin, instantiation_case, keys, last_fitting_nseg, many_dof_case, ok_share, PARITY_CASES,
                                 parity_cases, restatement, table_case, table_fits_lds)
from tests.solver_support import dispatches, irregular_batch, problem, same, traced
from toppra_amd import batch

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------------------------------
# shared setup (problems and host-side checks: tests/robust_shapes.py)

def kernel(prob, interp, want_X, variant=0):
    coef, breaks, grid, vlim, alim, sd0, sd1 = prob
    return batch.robust_solve_batch(coef, breaks, grid, vlim, alim, ELL, sd0, sd1, interp, want_X=want_X, variant=variant)


def check(oracle, prob, interp, want_X, what, variants=(0,)):
    """The kernels behind `variants` against the restatement on every trajectory.  -> the restatement's output"""
    ref = restatement(oracle, prob, interp, want_X)
    for variant in variants:
        same(kernel(prob, interp, want_X, variant), ref, keys(want_X), what + (interp, want_X, variant))
    return ref


# --------------------------------------------------------------------------------------------------------------------------
# 1. every dof instantiation

@pytest.mark.parametrize("d", range(1, 17))
def test_every_robust_instantiation(gpu, oracle, d):
    """group_robust_kernel<d, L> is compiled once per dof, and 2, 9, 10, 11, 13, 14, 15 had never run (why that matters:
    tests/test_gpu_instantiations.py).  96 x d x 48, shared uniform grid and per-trajectory non-uniform grids, Interpolation and
    Collocation, with and without X: the automatic choice and the lane kernel against the restatement."""
    for per_traj_grid in (False, True):
        prob = instantiation_case(d, per_traj_grid)
        assert prob[2].ndim == (2 if per_traj_grid else 1) and (prob[5] != 0).any() and (prob[6] != 0).any()
        for interp in (True, False):
            for want_X in (False, True):
                ref = check(oracle, prob, interp, want_X, (d, per_traj_grid), variants=(0, 1))
                assert ok_share(ref) >= 0.5, (d, per_traj_grid, interp, ok_share(ref))


# --------------------------------------------------------------------------------------------------------------------------
# 2. block geometries

GEOMETRIES = [(16384, 3, 128), (32768, 7, 256), (32768 + 5, 7, 256), (8192, 12, 128), (16384, 12, 256), (16384 + 3, 16, 256)]


def geometry_case(B, d, N, seed):
    data = batch.make_synthetic_batch(B, d, N, seed=seed)
    rng = np.random.default_rng(seed)
    sd1 = np.where(rng.random(B) < 0.3, 0.2 * rng.random(B), 0.0)
    return problem(data) + (None, sd1)


@pytest.mark.parametrize("B,d,threads", GEOMETRIES)
def test_multi_wave_blocks(gpu, oracle, B, d, threads):
    """Blocks of two and four waves (16 / 32 trajectories per block at 8 lanes, 8 / 16 at 16 lanes), a last block that is not full:
    every trajectory of the batch at N = 8, without X under Interpolation and with X under Collocation."""
    assert block_threads(B, d, 4) == threads and block_threads(300, d, 4) == 64
    prob = geometry_case(B, d, 8, seed=B % 1000 + d)
    for interp, want_X in ((True, False), (False, True)):
        assert ok_share(check(oracle, prob, interp, want_X, (B, d))) >= 0.5


def test_the_benchmarks_robust_batch(gpu, oracle):
    """bench.py's C4 case -- make_synthetic_batch(16384, 7, .) through robust_solve_batch(..., ELL), 128-thread blocks -- with N cut
    from 100 to 20."""
    assert block_threads(16384, 7, 4) == 128
    data = batch.make_synthetic_batch(16384, 7, 20)
    prob = problem(data) + (None, None)
    assert ok_share(check(oracle, prob, True, False, ("C4",))) >= 0.9


# --------------------------------------------------------------------------------------------------------------------------
# 3. both sides of the LDS table limit

def test_the_table_limits_are_where_the_cases_sit():
    assert last_fitting_nseg(7) == 41 and last_fitting_nseg(16) == 37 and last_fitting_nseg(1) > 100


@pytest.mark.parametrize("side", [0, 1], ids=["last table in LDS", "first fallback"])
@pytest.mark.parametrize("d", [7, 16, 1])
def test_spline_tables_on_both_sides_of_the_lds_limit(gpu, oracle, d, side):
    """d = 7 with 42 | 43 waypoints, d = 16 with 38 | 39, d = 1 at its own limit: the last table group_robust_kernel takes and the
    first that goes to the lane kernel.  64 x d x 24, non-uniform knots and grid; the three two-way choices (breakpoints shared or
    per trajectory, discretisation, X) as a half fraction in which every pair of choices occurs together."""
    nseg = last_fitting_nseg(d) + side
    assert table_fits_lds(d, nseg) == (side == 0)
    shared, own = table_case(d, nseg + 1, False), table_case(d, nseg + 1, True)
    assert shared[0].shape[2] == nseg and own[1].shape == (64, nseg + 1) and not np.array_equal(own[1][0], own[1][1])
    assert own[2].shape == (64, 25) and not np.array_equal(own[2][0], own[2][1]) and (np.diff(own[2], axis=1) > 0).all()
    for prob, interp, want_X in ((shared, True, True), (own, True, False), (shared, False, False), (own, False, True)):
        ref = check(oracle, prob, interp, want_X, (d, nseg, prob[1].ndim))
        assert ok_share(ref) >= 0.5, (d, nseg, prob[1].ndim, interp, ok_share(ref))


# --------------------------------------------------------------------------------------------------------------------------
# 4. 17..32 dof

@pytest.mark.parametrize("d", [17, 24, 32])
def test_above_16_dof(gpu, oracle, d):
    """The lane kernel as the ONLY kernel (!group_supported): 64 x d x 24, Interpolation with X, and Collocation without a
    velocity constraint."""
    prob = many_dof_case(d)
    ref = check(oracle, prob, True, True, (d, "vlim"))
    assert ok_share(ref) >= 0.3, (d, ok_share(ref))  # (the restatement solves 0.50 / 0.41 / 0.41 of them at 17 / 24 / 32 dof ...
    free = prob[:3] + (None,) + prob[4:]
    ref = check(oracle, free, False, True, (d, "no vlim"))
    assert ok_share(ref) >= 0.3, (d, ok_share(ref))  # ... and 0.73 / 0.56 / 0.45 without the velocity constraint)


# --------------------------------------------------------------------------------------------------------------------------
# 5. tiny and odd shapes

@pytest.mark.parametrize("B,d,N", [(1, 7, 1), (3, 2, 2), (130, 9, 1), (65, 13, 5), (1, 16, 40)])
def test_tiny_and_odd_shapes(gpu, oracle, B, d, N):
    """One trajectory, one and two stages, batches just past a whole number of blocks (a 64-thread block holds four trajectories
    at 16 lanes each: 130 = 32 blocks + 2 at 9 dof, 65 = 16 blocks + 1 at 13 dof)."""
    data = irregular_batch(B, d, N, 5, seed=10 * d + N)
    prob = problem(data) + (data["sd0"], data["sd1"])
    for interp in (True, False):
        for want_X in (False, True):
            check(oracle, prob, interp, want_X, (B, d, N), variants=(0, 1))


@pytest.mark.parametrize("d", [7, 20])
def test_the_empty_batch(gpu, d):
    data = irregular_batch(4, d, 10, 5, seed=d)
    out = batch.robust_solve_batch(data["coef"][:0], data["breaks"], data["grid"], data["vlim"][:0], data["alim"][:0], ELL, want_X=True)
    assert {k: v.shape for k, v in out.items()} == {"sd2": (0, 11), "sd": (0, 11), "u": (0, 10), "K": (0, 11, 2), "X": (0, 11, 2), "status": (0,)}


# --------------------------------------------------------------------------------------------------------------------------
# 6. the independent solver on the new shape classes

@pytest.mark.parametrize("name", PARITY_CASES)
def test_new_shape_classes_match_the_independent_solver(gpu, name):
    """Every fifth stage of every solved trajectory -- K and X to 1e-7, u to the checker's default -- and the failed ones
    confirmed infeasible (the CPU twin holds the restatement to 1e-9 on the same cases)."""
    from oracle import robust_independent as ri
    prob, interp = parity_cases()[name]
    out = kernel(prob, interp, True)
    assert (out["status"] == 0).sum() >= 4, name
    agg = ri.check_batch(as_checker_data(prob), ELL, out, interp, stride=5, tol_x=1e-7)
    assert agg["stages"] >= (prob[2].shape[-1] - 1) // 5 * int((out["status"] == 0).sum())
    print("independent solver, %s: %d stage problems, max dev K %.2e X %.2e u %.2e" % (name, agg["stages"], agg["K"], agg["X"], agg["u"]))


# --------------------------------------------------------------------------------------------------------------------------
# 7. device tensors

def test_device_tensors_in_device_tensors_out(gpu):
    import torch
    prob = instantiation_case(7, True)
    host = kernel(prob, True, True)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    got = kernel(tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in prob), True, True)
    assert set(got) == set(host)
    for k, v in got.items():
        assert isinstance(v, torch.Tensor) and v.is_cuda, k
        assert np.array_equal(v.cpu().numpy(), host[k], equal_nan=True), k


# --------------------------------------------------------------------------------------------------------------------------
# 8. which kernel ran

_TRACED_CHILD = """
import numpy as np
from tests.solver_support import irregular_batch
from toppra_amd import batch
for d, n_waypoints in ((7, %d), (7, %d), (17, 6)):
    data = irregular_batch(64, d, 8, n_waypoints, seed=d)
    out = batch.robust_solve_batch(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"], [1e-3, 5e-2, 9e-3])
    assert out["status"].shape == (64,) and data["coef"].shape[2] == n_waypoints - 1
print("traced child done")
""" % (last_fitting_nseg(7) + 1, last_fitting_nseg(7) + 2)


def test_the_kernel_that_ran(gpu):
    """The C-ABI does not say which kernel it launched, and parts 3 and 4 pass whichever did.  A fresh child process under the
    kernel tracer (no counters) makes one automatic robust call at 7 dof with 41 segments, one with 42 and one at 17 dof: the
    rows-across-lanes kernel must be what ran for the first, the lane kernel for the other two."""
    with traced(_TRACED_CHILD) as (calls, _):
        pass  # (the child leaves no files to read)
    group, group7 = dispatches(calls, "group_robust_kernel"), dispatches(calls, "group_robust_kernel", 7)
    lane = dispatches(calls, "robust_solve_kernel")
    assert (group, group7, lane) == (1, 1, 2), (group, group7, lane, [n for n, _ in calls])


# --------------------------------------------------------------------------------------------------------------------------
# 9. limits at the edge of the number range

@pytest.mark.parametrize("interp", [True, False], ids=["interpolation", "collocation"])
@pytest.mark.parametrize("d,N", EXTREME_SHAPES)
def test_extreme_limits(gpu, oracle, d, N, interp):
    """The twelve kinds of extreme_limit_batch and their `plain` controls, 208 trajectories: the automatic choice and the lane kernel
    against the restatement on every trajectory; `ahuge` solved wherever its +-inf twin is; the controls' bits those of the
    all-ordinary batch."""
    data, prob = extreme_case(d, N)
    ref = check(oracle, prob, interp, True, (d, N), variants=(0, 1))
    same(kernel(prob, interp, False), ref, keys(False), (d, N, interp, "no X"))
    twin = check(oracle, inf_twin(data, prob), interp, True, (d, N, "inf twin"))
    print(d, N, interp, check_extreme_counts(ref, twin, data["kinds"]))
    base = data["base"]
    ordinary = (base["coef"], base["breaks"], base["grid"], base["vlim"], base["alim"], data["sd0"], data["sd1"])
    plain = data["kinds"] == "plain"
    assert plain.sum() == 16 and all(np.array_equal(x[plain], y[plain]) for x, y in zip(prob[:5], ordinary[:5]))
    for variant in (0, 1):
        got, quiet = kernel(prob, interp, True, variant), kernel(ordinary, interp, True, variant)
        for k in ("status",) + keys(True):
            assert np.array_equal(got[k][plain], quiet[k][plain], equal_nan=True), (d, N, interp, variant, k)


@pytest.mark.parametrize("d,slow", RELAXED_CASES)
def test_limits_written_as_1e300_are_limits_written_as_inf(gpu, d, slow):
    for variant in (0, 1):
        check_relaxed_twins(lambda prob, interp, want_X: kernel(prob, interp, want_X, variant), d, slow)

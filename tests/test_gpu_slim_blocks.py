"""The certified lane kernels (kernel family 3) at 9..15 dof -- the "slim blocks" -- at the shapes they ship for.

Above 8 dof family 3 is another kernel than the 1..8-dof one the rest of the suite covers (CertStage::kSlim: no LDS copy of the
row constants or the grid, K staged two stages at a time, a per-block transposed workspace GroupArgs::tws that TwsScope allocates
per launch, spline coefficients read through cbase / cstride from that workspace or -- for long tables -- from the caller's array,
limits and coefficients re-read per stage from 10 / 11 dof, 4 / 2 / 1 cooperative batch groups, K stored straight to its row at
14 / 15 dof).  Before this module every run of it had a 4-segment spline on shared breakpoints, 40 .. 50 stages, few or no failing
trajectories and at most 1200 of them (tests/test_gpu_parity.py::test_certified_lane_kernel_above_8_dof,
tests/test_gpu_instantiations.py).
Here, always bit for bit (no tolerance anywhere):

1. spline tables on both sides of the workspace's coefficient limit, shared and per-trajectory breakpoints;
2. stage counts around the two-stage K ring and the 8-stage output staging, single trajectories, partly filled waves, a long grid;
3. the batch sizes from which the library picks this kernel by itself, and just below them;
4. the batches the README's 9..15-dof timings are taken on, every trajectory, and the largest workspace / longest-table launches;
5. the adversarial families that make certificates fail and send lanes into the cooperative batches;
6. which kernel the automatic choice dispatched, from a kernel trace of a child process.

Authorities: the CPU restatement of the reference (oracle/, pinned to the reference's compiled solver by
tests/test_oracle_vs_reference.py) on EVERY trajectory for the solve and TOPPRAsd; the oracle's wrapper object on a sample plus the
rows-across-lanes kernels' full iteration (variant=2, strict=True) on the whole batch for controllable and feasible sets.

RUN TIME, pytest's own figure on an MI355X machine with 16 host threads: 40.6 s for this module (128 tests) beside 28.3 s
for the rest of `-m gpu` (374 tests: what the whole GPU suite was before this module).  With part 1 as a full factorial (eight runs
per case instead of four) the module took 49.7 s and 48.7 s in two runs -- 20.2 s of it part 1, 5.0 s part 2 -- beside 27.6 s for the
rest of the suite; parts 3 .. 6 and the session set-up are 24 s by themselves, so the module costs more than the earlier suite
whatever parts 1 and 2 do, and part 1 was cut to the half fraction described at its test.
"""
import numpy as np
import pytest

from tests.solver_support import (CERT_AUTO_FROM, dispatches, irregular_batch, near_parallel_family, oracle_flags, own_breakpoints, problem, same,
                                  same_array, traced)
from toppra_amd import batch

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------------------------------
# shared setup (the irregular batch, the comparison and CERT_AUTO_FROM -- cert_auto_from(d), on which parts 3 and 6 sit:
# tests/solver_support.py)

def block_sample(B, every=None):
    """Trajectories for the per-trajectory wrapper checks: every `every`-th one, or -- large batches -- at least 128 spread over all
    64-lane blocks, with both ends of block 0, of the last full block and of the partial block."""
    if every is not None:
        return np.arange(0, B, every)
    full = B // 64
    ends = [0, min(63, B - 1), max(full - 1, 0) * 64, max(full * 64 - 1, 0), min(full * 64, B - 1), B - 1]
    return np.unique(np.concatenate([np.linspace(0, B - 1, 128).astype(np.int64), np.asarray(ends, dtype=np.int64)]))


def row(x, b):
    """Trajectory b's own row of a per-trajectory array, or the shared one."""
    return x[b] if x.ndim == 2 else x


def check_sets(oracle, coef, breaks, grid, vlim, alim, interp, sample, seed, what):
    """feasible_sets_batch and controllable_sets_batch (sdmin != sdmax: the backward scan alone) on family 3: the oracle's wrapper
    object on `sample`, the full iteration of family 2 on the whole batch."""
    B = coef.shape[0]
    flags = oracle_flags(oracle, vlim is not None, interp)
    rng = np.random.default_rng(seed)
    sdmin = np.where(rng.random(B) < 0.5, 0.0, 0.2 * rng.random(B))
    sdmax = sdmin + 0.02 + 0.5 * rng.random(B)
    X = batch.feasible_sets_batch(coef, breaks, grid, vlim, alim, interp, variant=3)
    same_array(X, batch.feasible_sets_batch(coef, breaks, grid, vlim, alim, interp, variant=2, strict=True), what + ("X vs family 2",))
    K = batch.controllable_sets_batch(coef, breaks, grid, vlim, alim, sdmin, sdmax, interp, variant=3)
    same_array(K, batch.controllable_sets_batch(coef, breaks, grid, vlim, alim, sdmin, sdmax, interp, variant=2, strict=True),
               what + ("controllable sets vs family 2",))
    for b in sample:
        w = oracle.Wrapper(coef[b], row(breaks, b), row(grid, b), None if vlim is None else vlim[b], alim[b], flags=flags)
        assert np.array_equal(X[b], w.compute_feasible_sets(), equal_nan=True), what + ("X vs oracle", int(b))
        w = oracle.Wrapper(coef[b], row(breaks, b), row(grid, b), None if vlim is None else vlim[b], alim[b], flags=flags)
        assert np.array_equal(K[b], w.compute_controllable_sets(sdmin[b], sdmax[b]), equal_nan=True), what + ("controllable sets vs oracle", int(b))
    return K


def check_sd(oracle, coef, breaks, grid, vlim, alim, sd0, sd1, interp, desired, what, variants=(3,)):
    """TOPPRAsd through `variants`: the oracle on every trajectory (sd2, u, alpha, status), family 2 on the whole batch (K, sd).
    -> the oracle's output"""
    ref = oracle.solve_batch_sd(coef, breaks, grid, vlim, alim, desired, sd0, sd1, flags=oracle_flags(oracle, vlim is not None, interp), nthreads=0)
    f2 = batch.solve_desired_duration_batch(coef, breaks, grid, vlim, alim, desired, sd0, sd1, variant=2, interpolation=interp)
    same(f2, ref, ("sd2", "u", "alpha"), what + ("TOPPRAsd, family 2 vs oracle",))
    for variant in variants:
        got = batch.solve_desired_duration_batch(coef, breaks, grid, vlim, alim, desired, sd0, sd1, variant=variant, interpolation=interp)
        same(got, ref, ("sd2", "u", "alpha"), what + ("TOPPRAsd vs oracle", variant))
        same(got, f2, ("K", "sd"), what + ("TOPPRAsd vs family 2", variant))
    return ref


def desired_durations(B, seed):
    """TOPPRAsd's desired durations: uniform in 0.3 .. 12 s."""
    return np.random.default_rng(seed).uniform(0.3, 12.0, size=B)


def blend_kinds(ref):
    """(trajectories blended between the two profiles, trajectories at alpha == 1) of a TOPPRAsd oracle output."""
    ok = ref["status"] == 0
    return int((ok & (ref["alpha"] > 0) & (ref["alpha"] < 1)).sum()), int((ref["alpha"] == 1).sum())


def check_solve(oracle, coef, breaks, grid, vlim, alim, sd0, sd1, interp, what):
    """solve_batch on family 3 with and without the sd output against the oracle on every trajectory (sd: against family 2's full
    iteration, itself held to the oracle here).  -> the oracle's output"""
    args = (coef, breaks, grid, vlim, alim, sd0, sd1)
    ref = oracle.solve_batch(*args, flags=oracle_flags(oracle, vlim is not None, interp), nthreads=0)
    f2 = batch.solve_batch(*args, interp, want_sd=True, variant=2, strict=True)
    same(f2, ref, ("K", "sd2", "u"), what + ("family 2 vs oracle",))
    same(batch.solve_batch(*args, interp, variant=3), ref, ("K", "sd2", "u"), what + ("family 3 vs oracle",))
    got = batch.solve_batch(*args, interp, want_sd=True, variant=3)
    same(got, ref, ("K", "sd2", "u"), what + ("family 3 with sd vs oracle",))
    same(got, f2, ("sd",), what + ("family 3 sd vs family 2",))
    return ref


def four_entries(oracle, coef, breaks, grid, vlim, alim, sd0, sd1, interp, desired, seed, what):
    """Solve (with and without the sd output), feasible sets, controllable sets and TOPPRAsd on family 3 for one discretisation.
    -> successes of the solve"""
    what = what + ("Interpolation" if interp else "Collocation",)
    ref = check_solve(oracle, coef, breaks, grid, vlim, alim, sd0, sd1, interp, what)
    check_sets(oracle, coef, breaks, grid, vlim, alim, interp, block_sample(coef.shape[0], 7), seed, what)
    check_sd(oracle, coef, breaks, grid, vlim, alim, sd0, sd1, interp, desired, what)
    return int((ref["status"] == 0).sum())


# --------------------------------------------------------------------------------------------------------------------------
# 1. spline-table length against the workspace limit

# From 11 dof (TPR_LEAN_COEF_FROM) the slim blocks copy a trajectory's 3 nseg d coefficients into the transposed workspace, but only
# while nseg <= kTwsMaxSeg = 16 (toppra_amd/csrc/tpr_group.hip.inc:725, cert_tws_fields); the stage loop reads them there at stride
# 64, or -- longer tables -- from the caller's array at stride 1 (tpr_cert.hip.inc: cbase / cstride).  Waypoints 2, 3, 16, 17, 18, 41 are
# nseg = 1, 2, 15, 16 | 17, 40: the smallest tables, the last two that go to the workspace, the first that does not, a long one.
# Whoever moves kTwsMaxSeg moves the middle four.
TWS_WAYPOINTS = (2, 3, 16, 17, 18, 41)


def table_case(d, n_waypoints):
    """One case of part 1 (B = 200, N = 60) with its TOPPRAsd durations: what the kernels run and what the condition test reads."""
    data = irregular_batch(200, d, 60, n_waypoints, seed=100 * d + n_waypoints)
    data["desired"] = desired_durations(200, seed=d)
    return data


@pytest.mark.parametrize("n_waypoints", TWS_WAYPOINTS)
@pytest.mark.parametrize("d", range(9, 16))
def test_spline_table_length_around_the_workspace_limit(gpu, oracle, d, n_waypoints):
    """B = 200 (three full blocks and a partial one), N = 60, non-uniform knots; shared and per-trajectory breakpoints, with and
    without the velocity constraint, Interpolation and Collocation, the four entry points.  The three two-way choices run as a
    half fraction -- four runs per case in which every pair of choices occurs together -- instead of all eight (never run: own
    breakpoints with vlim and shared breakpoints without vlim under Interpolation, the two complements under Collocation): RUN TIME
    in the module's docstring."""
    data = table_case(d, n_waypoints)
    assert data["coef"].shape[2] == n_waypoints - 1
    shared, own = (data["coef"], data["breaks"]), own_breakpoints(data, seed=d + n_waypoints)
    assert n_waypoints == 2 or not np.array_equal(own[1][0], own[1][1])
    succeeded = 0
    for (coef, breaks), vlim, interp in ((shared, data["vlim"], True), (own, None, True), (shared, None, False), (own, data["vlim"], False)):
        what = (d, n_waypoints, "own breakpoints" if breaks.ndim == 2 else "shared breakpoints", "no vlim" if vlim is None else "vlim")
        succeeded += four_entries(oracle, coef, breaks, data["grid"], vlim, data["alim"], data["sd0"], data["sd1"], interp, data["desired"],
                                  seed=d, what=what)
    assert succeeded > 0, "no trajectory of the case succeeds: it exercises the NaN filling only"


def test_spline_table_cases_blend_and_saturate(oracle):
    """Across the cases above TOPPRAsd both blends (0 < alpha < 1, status 0) and saturates (alpha == 1) -- on the oracle's output
    (the shared-breakpoint, velocity-limited Interpolation run of every case)."""
    kinds = np.zeros(2, dtype=np.int64)
    for d in range(9, 16):
        for n_waypoints in TWS_WAYPOINTS:
            data = table_case(d, n_waypoints)
            kinds += blend_kinds(oracle.solve_batch_sd(*problem(data), data["desired"], data["sd0"], data["sd1"], nthreads=0))
    assert kinds[0] > 0 and kinds[1] > 0, kinds


# --------------------------------------------------------------------------------------------------------------------------
# 2. stage-count and batch-size edges

EDGE_SHAPES = [(1, 1), (3, 2), (63, 3), (65, 4), (64, 7), (130, 8), (100, 9), (64, 16), (70, 17), (40, 2100)]
EDGE_DOFS = [9, 10, 13, 14, 15]


def edge_case(d, B, N):
    data = irregular_batch(B, d, N, 5, seed=1000 * d + N)
    rng = np.random.default_rng(N + d)
    data["sd0"], data["sd1"] = 0.1 * (1.0 - rng.random(B)), 0.1 * (1.0 - rng.random(B))  # in (0, 0.1]: non-zero at both ends
    data["desired"] = desired_durations(B, seed=N)
    return data


@pytest.mark.parametrize("B,N", EDGE_SHAPES)
@pytest.mark.parametrize("d", EDGE_DOFS)
def test_stage_count_and_batch_size_edges(gpu, oracle, d, B, N):
    """The slim blocks at the edges of their launch geometry: single trajectories and partly filled waves, stage counts around the
    ring of two K stages and the 8-stage output staging, a long grid; non-zero boundary velocities everywhere.  dofs: the ring of
    two (9), the velocity re-read (10), two batch groups (13), K stored directly (14), one batch group (15)."""
    data = edge_case(d, B, N)
    assert np.all(data["sd0"] > 0) and np.all(data["sd1"] > 0)
    for interp in (True, False):
        four_entries(oracle, *problem(data), data["sd0"], data["sd1"], interp, data["desired"], seed=N, what=(d, B, N))


def test_edge_cases_blend_and_saturate(oracle):
    """... and across these cases as well, on the oracle's output."""
    kinds = np.zeros(2, dtype=np.int64)
    for d in EDGE_DOFS:
        for B, N in EDGE_SHAPES:
            data = edge_case(d, B, N)
            kinds += blend_kinds(oracle.solve_batch_sd(*problem(data), data["desired"], data["sd0"], data["sd1"], nthreads=0))
    assert kinds[0] > 0 and kinds[1] > 0, kinds


# --------------------------------------------------------------------------------------------------------------------------
# 3. the sizes the kernel is chosen for

@pytest.mark.parametrize("offset", [37, -27])
@pytest.mark.parametrize("d", range(9, 16))
def test_the_batch_sizes_the_kernel_is_chosen_for(gpu, oracle, d, offset):
    """The irregular batch at cert_auto_from(d) + 37 (the automatic choice, with a ragged last block) and at cert_auto_from(d) - 27
    (just under it): the automatic choice, family 3 and family 2 against the oracle on every trajectory."""
    B, N = CERT_AUTO_FROM[d] + offset, 100
    data = irregular_batch(B, d, N, 6, seed=4242)  # (one set of knots for every dof: the conditions below hold on it, 13 .. 16 % blended)
    prob = problem(data)
    args = prob + (data["sd0"], data["sd1"])
    what = (d, B)
    ref = oracle.solve_batch(*args, nthreads=0)
    share = (ref["status"] == 0).mean()
    assert 0.25 < share < 0.75, (what, share)  # successful paths and the NaN filling of failed lanes in every block
    for kw in (dict(), dict(variant=3), dict(variant=2)):
        same(batch.solve_batch(*args, **kw), ref, ("K", "sd2", "u"), what + ("solve", kw))
    # feasible sets and the backward scan alone: family 3 against the full iteration of family 2 and the wrapper sample, and the
    # automatic choice of the feasible sets against that full iteration
    sample = block_sample(B)
    assert len(sample) >= 128 and {0, (B // 64 - 1) * 64, (B // 64) * 64, B - 1} <= set(sample.tolist())
    check_sets(oracle, *prob, True, sample, seed=B, what=what)
    same_array(batch.feasible_sets_batch(*prob), batch.feasible_sets_batch(*prob, variant=2, strict=True), what + ("X", "automatic choice"))
    # TOPPRAsd: the oracle on every trajectory
    sd = check_sd(oracle, *args, True, desired_durations(B, seed=d), what=what, variants=(0, 3))
    blended, saturated = blend_kinds(sd)
    assert blended >= 0.1 * B and saturated >= 0.1 * B, (what, blended, saturated)


# --------------------------------------------------------------------------------------------------------------------------
# 4. what the README times

@pytest.mark.parametrize("d", range(9, 16))
def test_the_batches_the_readme_times(gpu, oracle, d):
    """make_synthetic_batch(65536, d, 200) -- what bench.py --dof d times -- through the automatic choice: every trajectory
    against the oracle."""
    data = batch.make_synthetic_batch(65536, d, 200)
    args = problem(data)
    got = batch.solve_batch(*args)
    ref = oracle.solve_batch(*args, nthreads=0)
    assert (ref["status"] == 0).mean() > 0.99
    same(got, ref, ("K", "sd2", "u"), (d,))


@pytest.mark.parametrize("n_waypoints", [18, 17])
def test_full_chip_launches_on_either_side_of_the_workspace_limit(gpu, oracle, n_waypoints):
    """65536 x 15 x 60, irregular.  17 segments: 1024 blocks on the long-table path (coefficients from the caller's array at stride
    1), the smallest workspace per block.  16 segments: the largest workspace the library allocates -- 1024 blocks x
    (4 x 15 + 3 x 16 x 15) fields x 64 lanes x 8 B = 409 MB (TwsScope: a failed allocation is TPR_E_UNSUPPORTED, and a failure
    of this test)."""
    B, d, N = 65536, 15, 60
    data = irregular_batch(B, d, N, n_waypoints, seed=n_waypoints)
    args = problem(data) + (data["sd0"], data["sd1"])
    ref = oracle.solve_batch(*args, nthreads=0)
    assert len(np.unique(ref["status"])) >= 2 and (ref["status"] == 0).mean() > 0.1
    for kw in (dict(), dict(variant=3)):
        same(batch.solve_batch(*args, **kw), ref, ("K", "sd2", "u"), (n_waypoints, kw))


# --------------------------------------------------------------------------------------------------------------------------
# 5. adversarial families

def sliver_family(B, d, N, seed):
    """tests/test_gpu_fullsize.py::test_concurrent_rows_and_sliver_pivots_are_bit_exact's generator: the acceleration limits of three
    joints moved so that their rows at a random stage pass through a point of the solution to within 1e-13 .. 1e-8."""
    rng = np.random.default_rng(4200 + seed)
    data = batch.make_synthetic_batch(B, d, N, seed=4300 + seed)
    scale = 10.0 ** rng.uniform(-3, 1, size=(B, 1, 1, 1))
    scale[rng.random(B) < 0.5] = 1.0
    coef = data["coef"] * scale
    grid = data["grid"]
    base = batch.solve_batch(coef, data["breaks"], grid, data["vlim"], data["alim"])
    ok = base["status"] == 0
    j = rng.integers(1, N - 1, size=B)
    rows = np.arange(B)
    u0 = np.where(ok, base["u"][rows, j], 0.0)
    x0 = np.where(ok, base["sd2"][rows, j], 0.5)
    off = np.where(rng.random(B) < 0.4, 0.0, 10.0 ** rng.uniform(-8, -2, size=B))
    u0 = u0 + off * rng.standard_normal(B) * np.maximum(1.0, np.abs(u0))
    x0 = np.maximum(x0 + off * rng.standard_normal(B) * np.maximum(1.0, np.abs(x0)), 0.0)
    qs, qss = np.empty((B, d)), np.empty((B, d))                  # q'(s_j), q''(s_j)
    for lo in range(0, B, 1024):                                  # (in slices: the row arrays are [B, N + 1, 2 + 4 d] each)
        sl = slice(lo, min(lo + 1024, B))
        par = batch.constraint_params_batch(coef[sl], data["breaks"], grid, data["vlim"][sl], data["alim"][sl])
        qs[sl], qss[sl] = par["qs"][np.arange(sl.stop - lo), j[sl]], par["qss"][np.arange(sl.stop - lo), j[sl]]
    alim = data["alim"].copy()
    joints = np.argsort(rng.random((B, d)), axis=1)[:, :3]        # three distinct joints per trajectory
    for t in range(3):
        k = joints[:, t]
        val = qs[rows, k] * u0 + qss[rows, k] * x0                # the row's left-hand side at P
        eps = 10.0 ** rng.uniform(-13, -8, size=B) * rng.choice([-1.0, 1.0], size=B) * np.maximum(1.0, np.abs(val))
        upper = rng.random(B) < 0.5                               # which twin goes through P
        width = 10 + 2 * rng.random(B)
        amax = np.where(upper, val + eps, val + eps + width)
        amin = np.where(upper, val + eps - width, val + eps)
        alim[rows, k, 0], alim[rows, k, 1] = amin, amax
    sd1 = np.where(rng.random(B) < 0.3, 0.2 * rng.random(B), 0.0)
    return coef, data["breaks"], grid, data["vlim"], alim, None, sd1


def _adversarial(oracle, args, condition):
    """Family 3 and the automatic choice against the full iteration of family 2 on the whole batch; all three against the oracle on
    the first 512 trajectories.  args: (coef, breaks, grid, vlim, alim, sd_start, sd_end), breaks and grid shared."""
    coef, breaks, grid, vlim, alim, sd0, sd1 = args
    m = 512
    ref = oracle.solve_batch(coef[:m], breaks, grid, vlim[:m], alim[:m], None if sd0 is None else sd0[:m], None if sd1 is None else sd1[:m],
                             nthreads=0)
    full = batch.solve_batch(*args, variant=2, strict=True)
    condition(full["status"])
    for kw, got in [("family 2, full iteration", full)] + [(kw, batch.solve_batch(*args, **kw)) for kw in (dict(variant=3), dict())]:
        same(got, full, ("K", "sd2", "u"), (kw,))
        same({k: got[k][:m] for k in ("status", "K", "sd2", "u")}, ref, ("K", "sd2", "u"), (kw, "vs oracle"))


@pytest.mark.parametrize("d", [9, 11, 13, 15])
def test_near_parallel_rows_on_slim_blocks(gpu, oracle, d):
    """Four, two and one cooperative batch groups (9 / 11, 13, 15 dof) on the family that makes certificates fail: family 3 and the
    automatic choice against the full iteration of family 2 on 8192 trajectories, the first 512 against the oracle."""
    def condition(status):
        assert (status == 1).sum() >= 1  # the reference itself trips over some of them
    _adversarial(oracle, near_parallel_family(8192, d, 48, seed=d), condition)


@pytest.mark.parametrize("d", [9, 11, 13, 15])
def test_sliver_pivots_on_slim_blocks(gpu, oracle, d):
    def condition(status):
        assert 0.02 < (status == 0).mean() < 0.999  # the family is hard: many of them fail in the reference too
    _adversarial(oracle, sliver_family(8192, d, 48, seed=d), condition)


def test_boundary_velocities_and_scaled_paths_at_12_dof(gpu, oracle):
    """The two cases of test_lower_bound_shortcut_is_exact on a slim block: boundary velocities on 30 % of the trajectories, and
    whole-path scales 1e-6 .. 1 (on which the reference itself fails)."""
    B, d, N, seed = 8192, 12, 50, 12
    data = batch.make_synthetic_batch(B, d, N, seed=seed)
    rng = np.random.default_rng(seed)
    sd0 = np.where(rng.random(B) < 0.3, 0.1 * rng.random(B), 0.0)
    sd1 = np.where(rng.random(B) < 0.3, 0.3 * rng.random(B), 0.0)
    scale = 10.0 ** rng.uniform(-6, 0, size=(B, 1, 1, 1))
    for coef, s0, s1 in ((data["coef"], sd0, sd1), (data["coef"] * scale, None, None)):
        def condition(status, need=1 if s0 is not None else 2):
            assert len(np.unique(status)) >= need
        _adversarial(oracle, (coef, data["breaks"], data["grid"], data["vlim"], data["alim"], s0, s1), condition)


# --------------------------------------------------------------------------------------------------------------------------
# 6. which kernel the automatic choice ran

_TRACED_CHILD = """
import sys
import numpy as np
from toppra_amd import batch
offset = int(sys.argv[1])
for d, at in ((9, %d), (15, %d)):
    B = at + offset
    data = batch.make_synthetic_batch(B, d, 16, seed=d)
    args = (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])
    out = batch.solve_batch(*args)
    X = batch.feasible_sets_batch(*args)
    sd = batch.solve_desired_duration_batch(*args, np.full(B, 3.0))
    assert out["status"].shape == (B,) and X.shape == (B, 17, 2) and sd["alpha"].shape == (B,)
print("traced child done")
""" % (CERT_AUTO_FROM[9], CERT_AUTO_FROM[15])


@pytest.mark.parametrize("offset", [0, -1])
def test_the_documented_thresholds_are_the_dispatched_ones(gpu, offset):
    """The C-ABI does not say which family it launched, and the parity tests above pass whichever did.  A fresh child process under
    the kernel tracer (no counters) makes one automatic solve_batch, feasible_sets_batch and solve_desired_duration_batch at 9 and 15
    dof, at cert_auto_from(d) (offset 0) or one trajectory below: the certified lane kernels must be what ran at the threshold
    (tpr_kernels.hip: pick_variant; tpr_solve_desired_duration_batch for TOPPRAsd; tpr_feasible_sets_batch) and the
    rows-across-lanes kernels below it."""
    with traced(_TRACED_CHILD, str(offset)) as (calls, _):
        pass  # (the child leaves no files to read)
    cert = ("cert_solve_kernel", "cert_feasible_kernel")
    group = ("group_solve_kernel", "group_feasible_kernel", "group_sd_forward_kernel")
    for d in (9, 15):
        ran = {k: dispatches(calls, k, d) for k in cert + group}
        if offset == 0:
            # the fused solve and the fused TOPPRAsd launch (another instantiation of cert_solve_kernel), the feasible sets -- and no
            # rows-across-lanes kernel at this dof for any of the three calls
            assert ran["cert_solve_kernel"] >= 1 and ran["cert_feasible_kernel"] >= 1, (d, ran)
            assert not any(ran[k] for k in group), (d, ran)
        else:
            # the solve and TOPPRAsd's backward scan, its two forward profiles, the feasible sets: rows across lanes
            assert ran["group_solve_kernel"] >= 1 and ran["group_sd_forward_kernel"] >= 1 and ran["group_feasible_kernel"] >= 1, (d, ran)
            assert not any(ran[k] for k in cert), (d, ran)

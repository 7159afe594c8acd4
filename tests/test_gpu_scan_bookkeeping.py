"""The certified lane kernels' scan-loop bookkeeping (kernel family 3): everything in a stage that is NOT certificate or LP
arithmetic -- the by-index row fetch (CertStage::fetch), the K ring and the forward outputs' staging with their tails, the
spline segment tracking, partial last blocks and their shadow lanes, the hand-over to the cooperative batches and the NaN /
status flags.  None of it may change a bit of the result, so every case is compared bit for bit (NaN pattern included) with the
full Seidel iteration (strict=True, kernel family 2) AND with the CPU restatement of the reference (oracle/).

Shapes: N around multiples of 4 and 8 (K ring of 4 stages, forward staging of 8), B around the 64-lane block; 1 and 7 dof (fetch
reads every row as a pair of loads, rows 0..5 from the block's six-double table), 8 dof (non-slim blocks with the select form of
fetch; the full block stride of the internal row numbering) and 9 dof (slim blocks: the merged-load form of fetch)."""
import numpy as np
import pytest

from tests.solver_support import lattice_boundary_velocities, oracle_flags, per_trajectory_grid, problem, same, same_array
from toppra_amd import batch

pytestmark = pytest.mark.gpu
NS = (1, 2, 3, 4, 5, 7, 8, 9, 13, 17)
BS = (1, 63, 64, 65, 130)
KNOT_SETS = (np.linspace(0, 1, 5), np.array([0.0, 0.2, 0.45, 0.8, 1.0]), np.array([0.0, 0.3, 0.5, 0.625, 1.0]))


def _problem(B, d, N, seed, per_traj_grid=False, per_traj_breaks=False, one_segment=False, boundary=True):
    rng = np.random.default_rng(seed)
    m = 2 if one_segment else 5
    way = rng.standard_normal((B, m, d))
    vmax = 10 + 20 * rng.random((B, d))
    amax = 10 + 2 * rng.random((B, d))
    bc = "clamped" if one_segment else "not-a-knot"  # (two waypoints, not-a-knot: a straight line)
    if per_traj_breaks:
        sets = [np.linspace(0, 1, m)] if one_segment else KNOT_SETS
        fits = [batch.spline_coefficients(k, way, bc_type=bc) for k in sets]
        pick = np.arange(B) % len(sets)
        coef = np.ascontiguousarray(np.stack([fits[pick[b]][0][b] for b in range(B)]))
        breaks = np.ascontiguousarray(np.stack([fits[pick[b]][1] for b in range(B)]))
    else:
        coef, breaks = batch.spline_coefficients(np.linspace(0, 1, m), way, bc_type=bc)
    grid = per_trajectory_grid(rng, B, N) if per_traj_grid else np.linspace(0, 1, N + 1)
    sd0, sd1 = lattice_boundary_velocities(rng, B, 0.1, 0.2) if boundary else (None, None)
    return {"coef": coef, "breaks": breaks, "grid": grid, "vlim": np.ascontiguousarray(np.stack([-vmax, vmax], axis=-1)),
            "alim": np.ascontiguousarray(np.stack([-amax, amax], axis=-1)), "sd0": sd0, "sd1": sd1}


def _check(oracle, p, what, interp=True, want_sd=False, variants=(3,)):
    args = problem(p) + (p["sd0"], p["sd1"])
    want = batch.solve_batch(*args, interp, want_sd=want_sd, strict=True)
    ref = oracle.solve_batch(*args, flags=oracle_flags(oracle, True, interp), nthreads=4)
    for v in variants:
        got = batch.solve_batch(*args, interp, want_sd=want_sd, variant=v)
        same(got, want, ("sd2", "u", "K") + (("sd",) if want_sd else ()), what + (v, "strict"))
        same(got, ref, ("sd2", "u", "K"), what + (v, "oracle"))
    return ref


@pytest.mark.parametrize("d", (1, 7, 8, 9))
def test_ring_and_staging_tails_partial_blocks(gpu, oracle, d):
    """Every N x B of the lists above; shared / per-trajectory grid and breaks, the sd output and Collocation rotate through them
    (each with small and large N, full and partial blocks)."""
    solved = total = 0
    for a, N in enumerate(NS):
        for c, B in enumerate(BS):
            i = 3 * a + c
            per_grid, per_breaks, want_sd, interp = bool(i & 1), bool(i & 2), bool(i & 4), i % 5 != 3
            p = _problem(B, d, N, 1000 * d + 10 * N + c, per_grid, per_breaks)
            ref = _check(oracle, p, (d, N, B, per_grid, per_breaks, want_sd, interp), interp, want_sd)
            solved += int((ref["status"] == 0).sum())
            total += B
    assert solved > 0.5 * total, (d, solved, total)


@pytest.mark.parametrize("d", (1, 7, 8, 9))
def test_every_flag_combination_at_one_shape(gpu, oracle, d):
    for per_grid in (False, True):
        for per_breaks in (False, True):
            p = _problem(130, d, 13, 77 + d, per_grid, per_breaks)
            for interp in (True, False):
                for want_sd in (False, True):
                    _check(oracle, p, (d, per_grid, per_breaks, interp, want_sd), interp, want_sd)


@pytest.mark.parametrize("d", (7, 8, 9))
def test_spline_with_one_segment(gpu, oracle, d):
    for N in (1, 4, 9, 17):
        for per_grid, per_breaks in ((False, False), (True, False), (False, True)):
            p = _problem(65, d, N, 300 + d + N, per_grid, per_breaks, one_segment=True)
            assert p["coef"].shape[2] == 1
            _check(oracle, p, (d, N, per_grid, per_breaks), want_sd=bool(N & 1))


@pytest.mark.parametrize("d", (7, 8, 9))
def test_gridpoints_exactly_on_breakpoints(gpu, oracle, d):
    """Uniform grids of 4 and 8 stages hit the breakpoints 0.25, 0.5, 0.75 exactly; an irregular grid that contains every
    breakpoint of its trajectory; and a grid whose points sit one ulp on either side of them."""
    for N in (4, 8):
        _check(oracle, _problem(65, d, N, 400 + d + N), (d, N, "uniform"))
    p = _problem(65, d, 13, 450 + d, per_traj_breaks=True)
    B = 65
    rng = np.random.default_rng(5)
    rest = np.sort(rng.random((B, 9)), axis=1) * 0.98 + 0.01
    grid = np.sort(np.concatenate([p["breaks"], rest], axis=1), axis=1)
    assert grid.shape == (B, 14) and (np.diff(grid, axis=1) > 0).all()
    _check(oracle, dict(p, grid=grid), (d, "every breakpoint in the grid"))
    knots = np.linspace(0, 1, 5)
    near = np.sort(np.concatenate([[0.0, 1.0], np.nextafter(knots[1:4], 0.0), knots[1:4], np.nextafter(knots[1:4], 1.0)]))
    q = _problem(64, d, len(near) - 1, 470 + d)
    _check(oracle, dict(q, grid=near), (d, "one ulp around the breakpoints"), want_sd=True)


@pytest.mark.parametrize("d", (7, 8, 9))
def test_uncontrollable_trajectories_in_the_batch(gpu, oracle, d):
    """A third of the batch cannot stop from its end speed (NaN controllable sets from the last stage down), a third starts
    outside K[0] (FailUncontrollable with K intact): the status and NaN paths beside lanes that solve."""
    for N, B in ((13, 130), (17, 65), (4, 63)):
        p = _problem(B, d, N, 500 + d + N, boundary=False)
        kind = np.arange(B) % 3
        p["sd1"] = np.where(kind == 1, 80.0, 0.0)
        p["sd0"] = np.where(kind == 2, 80.0, 0.0)
        for want_sd in (False, True):
            ref = _check(oracle, p, (d, N, B, want_sd), want_sd=want_sd)
        assert (ref["status"][kind == 0] == 0).mean() > 0.5, (d, N)
        assert (ref["status"][kind != 0] != 0).all(), (d, N, ref["status"])
        assert np.isnan(ref["K"][kind == 1]).any() and not np.isnan(ref["K"][kind == 2]).all()


def test_auto_choice_at_a_family_3_batch_size(gpu, oracle):
    """variant = 0 hands 9216 trajectories of up to 8 dof to the certified lane kernel (toppra_amd.batch.solve_batch)."""
    for d, N in ((7, 5), (8, 9)):
        p = _problem(9216 + 1, d, N, 600 + d)
        _check(oracle, p, (d, N, "auto"), variants=(0, 3))


@pytest.mark.parametrize("d", (7, 8))
def test_feasible_sets_and_toppra_sd_share_the_fetch(gpu, d):
    for N, B in ((5, 65), (13, 130)):
        for interp in (True, False):
            p = _problem(B, d, N, 700 + d + N)
            args = problem(p)
            X2 = batch.feasible_sets_batch(*args, interp, variant=2)
            X3 = batch.feasible_sets_batch(*args, interp, variant=3)
            same_array(X3, X2, (d, N, B, interp, "X"))
            desired = np.random.default_rng(d).uniform(0.5, 5.0, size=B)
            a = batch.solve_desired_duration_batch(*args, desired, p["sd0"], p["sd1"], variant=2, interpolation=interp)
            b = batch.solve_desired_duration_batch(*args, desired, p["sd0"], p["sd1"], variant=3, interpolation=interp)
            same(b, a, ("K", "sd2", "sd", "u", "alpha"), (d, N, B, interp, "TOPPRAsd"))

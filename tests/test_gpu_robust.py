"""Robust (conic) TOPP-RA, BASELINE config 4.  The reference's solver for these stage problems is ECOS
(unavailable; the reference's own tests at this boundary are skipped or qualitative), so parity is
pinned to an INDEPENDENT solution of the same second-order-cone stage problems instead
(oracle/robust_independent.py: problems rebuilt from ecos_solverwrapper.py:94-188 with scipy/numpy,
solved by cutting planes + exhaustive vertex enumeration -- nothing in common with the kernels'
closed-form-interval + bisection method): K and X to 1e-7 (stated bar; ~1e-12 measured), u to 1e-6
relative, over > 10^3 stage problems incl. Collocation, non-zero sd_end, no velocity constraint and
uncontrollable trajectories.  Also: the HIP kernels against the CPU restatement of their own method (bit
for bit), the zero ellipsoid against the seidel LP path, nestedness, worst-case constraint satisfaction,
and the reference's qualitative test (tests/tests/retime/test_retime_wconic_constraints.py:30-48)."""
import numpy as np
import pytest

import toppra_amd as ta
from tests.helpers import assert_same
from tests.solver_support import oracle_flags, problem
from toppra_amd import batch

pytestmark = pytest.mark.gpu
ELL = [1e-3, 5e-2, 9e-3]  # examples/plot_robust_kinematics.py:26-28


@pytest.mark.parametrize("B,d,N,interp", [(96, 7, 100, True), (64, 3, 40, False), (40, 6, 150, True), (300, 8, 60, True), (33, 1, 30, True)])
def test_kernel_is_self_consistent_with_its_restatement(gpu, oracle, B, d, N, interp):
    """SELF-CONSISTENCY, not parity: oracle.robust_solve_batch is the C restatement of THIS kernel's own method (closed-form row
    intervals + Illinois regula falsi on the edges of the feasible x interval), so bit-equality says the two implementations of
    that method agree -- nothing about ECOS, the reference's solver for these problems (absent here: parity unpinned).  That
    the method solves the reference's stage problems is test_kernel_matches_independent_solver's job (1e-7)."""
    data = batch.make_synthetic_batch(B, d, N, seed=d)
    rng = np.random.default_rng(0)
    sd1 = np.where(rng.random(B) < 0.3, 0.2 * rng.random(B), 0.0)
    got = batch.robust_solve_batch(*problem(data), ELL, None, sd1, interp, want_X=True)
    ref = oracle.robust_solve_batch(*problem(data), ELL, None, sd1, flags=oracle_flags(oracle, True, interp), nthreads=0)
    assert np.array_equal(got["status"], ref["status"]) and (ref["status"] == 0).mean() > 0.9
    for k in ("K", "X", "sd2", "u"):
        assert_same(got[k], ref[k], k)
    # without feasible sets the Interpolation case runs the rows-across-lanes kernel: same bits
    fast = batch.robust_solve_batch(*problem(data), ELL, None, sd1, interp)
    assert np.array_equal(fast["status"], ref["status"])
    for k in ("K", "sd2", "u"):
        assert_same(fast[k], ref[k], k)


INDEPENDENT_CASES = [
    # B, d, N, interpolation, ellipsoid, non-zero sd_end, velocity constraint, stage stride
    (96, 7, 100, True, ELL, False, True, 5),
    (48, 3, 40, False, ELL, True, True, 3),                 # Collocation, non-zero sd_end
    (32, 6, 150, True, [1e-2, 1e-1, 5e-2], True, True, 7),
    (32, 4, 60, True, ELL, False, False, 4),                # no velocity constraint: +-ECOS_INFTY stand-ins bind
    (24, 8, 50, False, [5e-3, 2e-2, 1e-2], False, False, 3),
]


@pytest.mark.parametrize("B,d,N,interp,ell,end_vel,has_vel,stride", INDEPENDENT_CASES)
def test_kernel_matches_independent_solver(gpu, B, d, N, interp, ell, end_vel, has_vel, stride):
    """Row f4's parity pin: every sampled stage of every Ok trajectory -- backward K, feasible X, forward
    u -- against the independent SOCP solution; trajectories the kernel gives up on must be infeasible
    for the independent solver too."""
    from oracle import robust_independent as ri
    data = batch.make_synthetic_batch(B, d, N, seed=200 + d)
    rng = np.random.default_rng(d)
    sd_end = 0.3 * rng.random(B) if end_vel else None
    vlim = data["vlim"] if has_vel else None
    d2 = dict(data, vlim=vlim)
    # lane kernel (feasible sets + any discretisation) ...
    full = batch.robust_solve_batch(data["coef"], data["breaks"], data["grid"], vlim, data["alim"], ell,
                                    None, sd_end, interp, want_X=True)
    assert (full["status"] == 0).mean() >= 0.7
    agg = ri.check_batch(d2, ell, full, interp, stride=stride, tol_x=1e-7)
    assert agg["stages"] >= (N // stride - 1) * int((full["status"] == 0).sum())
    # ... and whatever the auto path picks without feasible sets (rows across lanes for Interpolation)
    fast = batch.robust_solve_batch(data["coef"], data["breaks"], data["grid"], vlim, data["alim"], ell,
                                    None, sd_end, interp)
    agg2 = ri.check_batch(d2, ell, fast, interp, stride=stride, want_X=False, tol_x=1e-7)
    assert agg2["stages"] == agg["stages"]
    print("independent solver: %d stage problems, max dev K %.2e X %.2e u %.2e" % (
        agg["stages"], max(agg["K"], agg2["K"]), agg["X"], max(agg["u"], agg2["u"])))


def test_uncontrollable_is_confirmed_by_independent_solver(gpu):
    from oracle import robust_independent as ri
    data = batch.make_synthetic_batch(32, 5, 60, seed=77)
    sd_end = np.full(32, 40.0)
    out = batch.robust_solve_batch(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"], ELL,
                                   None, sd_end)
    assert (out["status"] == 1).all()
    assert ri.check_batch(data, ELL, out, True)["failed_confirmed"] >= 24


def test_zero_ellipsoid_is_the_lp_path(gpu):
    data = batch.make_synthetic_batch(128, 7, 100, seed=9)
    rob = batch.robust_solve_batch(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"], [0, 0, 0])
    lp = batch.solve_batch(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])
    assert np.array_equal(rob["status"], lp["status"])
    assert np.nanmax(np.abs(rob["K"][:, :, 1] - lp["K"][:, :, 1])) < 1e-9
    assert np.nanmax(np.abs(rob["sd2"] - lp["sd2"])) < 1e-8
    assert np.nanmax(np.abs(rob["u"] - lp["u"])) < 1e-5  # u is less well conditioned than sd^2


def test_nested_and_worst_case_feasible(gpu):
    data = batch.make_synthetic_batch(64, 7, 80, seed=10)
    lp = batch.solve_batch(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])
    rob = batch.robust_solve_batch(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"], ELL)
    ok = (rob["status"] == 0) & (lp["status"] == 0)
    assert ok.mean() > 0.9
    assert np.all(rob["K"][ok][:, :, 1] <= lp["K"][ok][:, :, 1] + 1e-9)      # robust sets are nested
    # the profile itself is lower almost everywhere (at discretised switch points the greedy forward
    # step can overshoot the nominal valley by ~1e-4: 5 of 5184 gridpoints here)
    assert np.mean(rob["sd2"][ok] <= lp["sd2"][ok] + 1e-7) > 0.99
    assert np.all(rob["sd2"][ok] <= lp["sd2"][ok] + 1e-3)
    assert np.any(rob["sd2"][ok] < lp["sd2"][ok] - 1e-6)
    # every conic row holds at the solution: a u + b x + c + ||(ru u, rx x, rc)|| <= 0
    par = batch.constraint_params_batch(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])
    a, b, c = (par[k][ok][:, :-1, 2:] for k in ("a", "b", "c"))
    u, x = rob["u"][ok][:, :, None], rob["sd2"][ok][:, :-1, None]
    res = a * u + b * x + c + np.sqrt((ELL[0] * u) ** 2 + (ELL[1] * x) ** 2 + ELL[2] ** 2)
    assert np.max(res) <= 1e-7, np.max(res)
    assert np.all(np.abs(par["qs"][ok][:, :-1] * np.sqrt(x)) <= data["vlim"][ok][:, None, :, 1] * (1 + 1e-5))


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_qualitative_test(gpu, seed):
    """tests/tests/retime/test_retime_wconic_constraints.py:30-48 with this build's solver."""
    np.random.seed(seed)
    path = ta.SplineInterpolator(np.linspace(0, 1, 5), np.random.randn(5, 3))
    lims = np.array([[-1, 1], [-1, 2], [-1, 4]], dtype=float)
    vel_c = ta.constraint.JointVelocityConstraint(lims)
    acc_c = ta.constraint.JointAccelerationConstraint(lims, 1)
    ro_acc_c = ta.constraint.RobustLinearConstraint(acc_c, [1e-4, 1e-4, 5e-4], 1)
    inst = ta.algorithm.TOPPRA([vel_c, ro_acc_c], path, solver_wrapper="ecos")
    X = inst.compute_feasible_sets()
    assert np.all(X >= 0) and not np.any(np.isnan(X))
    K = inst.compute_controllable_sets(0, 0)
    assert np.all(K >= 0) and not np.any(np.isnan(K))
    traj = inst.compute_trajectory(0, 0)
    assert traj is not None and 0 < traj.duration < 20


@pytest.mark.parametrize("B,d,N", [(300, 7, 40), (96, 12, 24), (64, 16, 16)])
def test_rows_across_lanes_serves_every_case_with_the_lane_kernels_bits(gpu, B, d, N):
    """Round 3: the rows-across-lanes robust kernel takes Collocation, feasible sets and 9..16 dof as well (the generic
    lane kernel with its 4 KB of scratch rows is left with > 16 dof and very long spline tables): bit-identical to the
    lane kernel (variant=1) in every combination."""
    data = batch.make_synthetic_batch(B, d, N, seed=40 + d)
    rng = np.random.default_rng(d)
    sd1 = np.where(rng.random(B) < 0.3, 0.3 * rng.random(B), 0.0)
    ell = [1e-3, 5e-2, 9e-3]
    for vlim, kw in ((data["vlim"], dict()), (data["vlim"], dict(want_X=True)), (data["vlim"], dict(interpolation=False, want_X=True, sd_end=sd1)),
                     (None, dict(want_X=True))):
        args = (data["coef"], data["breaks"], data["grid"], vlim, data["alim"], ell)
        want = batch.robust_solve_batch(*args, variant=1, **kw)
        got = batch.robust_solve_batch(*args, **kw)
        for k in want:
            assert np.array_equal(got[k], want[k], equal_nan=True), (k, kw)


def _ecos_fixtures():
    import glob
    import os
    return sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robust_ecos_*.npz")))


@pytest.mark.parametrize("path", _ecos_fixtures() or [None])
def test_ecos_fixture(gpu, path):
    """Row f4's pin against the reference's OWN solver: fixtures written by tools/make_robust_golden.py on a machine that
    has PyPI `ecos` next to the reference (neither is available in this repository's build container, so none is committed
    yet and the test skips).  ECOS is an interior-point method stopped at ~1e-8: K, X and sd^2 are compared at 1e-6, u at
    1e-4 relative to its range."""
    if path is None:
        pytest.skip("no tests/golden/robust_ecos_*.npz: generate them with tools/make_robust_golden.py where `ecos` imports")
    fx = np.load(path)
    vlim = fx["vlim"] if fx["vlim"].size else None
    got = batch.robust_solve_batch(fx["coef"], fx["breaks"], fx["grid"], vlim, fx["alim"], list(fx["ell"]),
                                   None, fx["sd_end"], bool(fx["interpolation"]), want_X=True)
    ok = fx["return_code"] == 0
    assert np.array_equal(got["status"] == 0, ok)
    assert np.nanmax(np.abs(got["K"][ok] - fx["K"][ok])) <= 1e-6
    assert np.nanmax(np.abs(got["X"][ok] - fx["X"][ok])) <= 1e-6
    assert np.nanmax(np.abs(got["sd2"][ok] - fx["sd"][ok] ** 2)) <= 1e-6
    span = np.nanmax(np.abs(fx["sdd"][ok]), axis=1, keepdims=True)
    assert np.nanmax(np.abs(got["u"][ok] - fx["sdd"][ok]) / span) <= 1e-4

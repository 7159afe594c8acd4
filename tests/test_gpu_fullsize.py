"""BASELINE.json's full sizes through size-independent properties (the oracle is too slow to
check 65536 x 200 x 7 entry by entry in a test): structural invariants of K / sd^2 / u, agreement of
the two kernel families, idempotence, and exact oracle parity on a random 1024-trajectory sample."""
import numpy as np
import pytest

from toppra_amd import batch
from tests.helpers import need_reference_solver
from tests.solver_support import irregular_batch, near_parallel_family, oracle_flags, problem, same, same_array

pytestmark = pytest.mark.gpu


def _invariants(data, out, N):
    st = out["status"]
    ok = st == 0
    assert ok.mean() > 0.99
    K, x, u = out["K"][ok], out["sd2"][ok], out["u"][ok]
    assert not np.isnan(K).any() and np.all(K[:, :, 0] >= 0) and np.all(K[:, :, 0] <= K[:, :, 1] + 1e-9)
    assert np.all(x[:, 0] == 0) and np.all(x[:, -1] == 0)          # rest to rest
    assert np.all(x >= K[:, :, 0] - 1e-9) and np.all(x <= K[:, :, 1] + 1e-9)
    delta = np.diff(data["grid"])
    xn = x[:, :-1] + 2 * delta * u                                  # x_{i+1} = clip(shrink(x_i + 2 d u))
    assert np.all(x[:, 1:] <= xn + 1e-12)
    # the reference's shrink per forward stage: max(xn - 1e-8, 0.9999 xn), then the clip into K[i+1] (which
    # only lowers x where xn overshoots the controllable set)
    clipped = x[:, 1:] >= K[:, 1:, 1] - 1e-12
    assert np.all((xn - x[:, 1:] <= 1e-8 + 1e-4 * np.abs(xn) + 1e-12) | clipped)
    # joint acceleration limits hold at every gridpoint: q' u + q'' x within alim (collocation part)
    par = batch.constraint_params_batch(data["coef"][:256], data["breaks"], data["grid"], data["vlim"][:256],
                                        data["alim"][:256])
    ok256 = ok[:256]
    qs, qss = par["qs"][ok256][:, :-1], par["qss"][ok256][:, :-1]
    acc = qs * out["u"][:256][ok256][:, :, None] + qss * out["sd2"][:256][ok256][:, :-1, None]
    amax = data["alim"][:256][ok256][:, None, :, 1]
    assert np.all(np.abs(acc) <= amax * (1 + 1e-7) + 1e-7)
    vmax = data["vlim"][:256][ok256][:, None, :, 1]
    assert np.all(np.abs(qs) * np.sqrt(out["sd2"][:256][ok256][:, :-1, None]) <= vmax * (1 + 1e-5))


@pytest.mark.parametrize("B,d,N", [(65536, 7, 200), (4096, 7, 200), (65536, 6, 500)])
def test_full_size_properties(gpu, oracle, B, d, N):
    data = batch.make_synthetic_batch(B, d, N)
    out = batch.solve_batch(*problem(data))
    _invariants(data, out, N)
    # idempotence: a second launch returns the same bits
    same(batch.solve_batch(*problem(data)), out, ("K", "sd2", "u"), "a second launch")
    # exact oracle parity on a random sample (seconds on the host)
    idx = np.sort(np.random.default_rng(1).choice(B, size=1024 if N <= 200 else 256, replace=False))
    ref = oracle.solve_batch(data["coef"][idx], data["breaks"], data["grid"], data["vlim"][idx], data["alim"][idx],
                             nthreads=0)
    same({k: out[k][idx] for k in ("K", "sd2", "u", "status")}, ref, ("K", "sd2", "u"), "oracle sample")
    # the kernel families agree bit for bit on a 4096 slice (the default is family 3 at 65536, family 4 at 4096)
    sl = slice(0, 4096)
    for variant in (1, 2, 4):
        v = batch.solve_batch(data["coef"][sl], data["breaks"], data["grid"], data["vlim"][sl], data["alim"][sl],
                              variant=variant)
        same(v, {k: out[k][sl] for k in ("K", "sd2", "u", "status")}, ("K", "sd2", "u"), (variant,))


@pytest.mark.parametrize("B,d,N,seed", [(65536, 7, 200, 20240924), (32768, 6, 500, 3), (16384, 3, 100, 5),
                                        (16384, 8, 64, 6), (8192, 1, 50, 8)])
def test_lower_bound_shortcut_is_exact(gpu, B, d, N, seed):
    """The certified shortcut of the backward lower-bound LP (default) against the full Seidel
    iteration (TPR_STRICT_SEIDEL) on every stage of large batches: identical bits, including
    non-zero boundary velocities and badly scaled paths on which the reference itself fails."""
    data = batch.make_synthetic_batch(B, d, N, seed=seed)
    rng = np.random.default_rng(seed)
    sd0 = np.where(rng.random(B) < 0.3, 0.1 * rng.random(B), 0.0)
    sd1 = np.where(rng.random(B) < 0.3, 0.3 * rng.random(B), 0.0)
    scale = 10.0 ** rng.uniform(-6, 0, size=(B, 1, 1, 1))
    for coef, s0, s1 in ((data["coef"], sd0, sd1), (data["coef"] * scale, None, None)):
        args = (coef, data["breaks"], data["grid"], data["vlim"], data["alim"], s0, s1)
        full = batch.solve_batch(*args, strict=True)
        assert len(np.unique(full["status"])) >= (1 if s0 is not None else 2)
        # rows-across-lanes with shortcuts; certified lane kernel (default for large batches, d <= 13); one trajectory
        # per wave (default for small batches)
        for variant in (2, 3, 4):
            fast = batch.solve_batch(*args, variant=variant)
            same(fast, full, ("K", "sd2", "u"), (variant,))


@pytest.mark.parametrize("B,d,N,seed", [(65536, 7, 200, 21), (20480, 4, 120, 22), (16384, 8, 64, 23)])
def test_collocation_on_the_certified_lane_kernel(gpu, B, d, N, seed):
    """Collocation at full size: the certified lane kernel (the interpolation blocks are null rows there; default
    from 9 216 trajectories) against the full Seidel iteration of family 2 (disabled rows), bit for bit, with
    and without the velocity constraint, incl. non-zero boundary velocities and badly scaled paths."""
    data = batch.make_synthetic_batch(B, d, N, seed=seed)
    rng = np.random.default_rng(seed)
    sd0 = np.where(rng.random(B) < 0.3, 0.1 * rng.random(B), 0.0)
    sd1 = np.where(rng.random(B) < 0.3, 0.3 * rng.random(B), 0.0)
    scale = 10.0 ** rng.uniform(-6, 0, size=(B, 1, 1, 1))
    for coef, vlim, s0, s1 in ((data["coef"], data["vlim"], sd0, sd1), (data["coef"] * scale, data["vlim"], None, None),
                               (data["coef"], None, None, sd1)):
        args = (coef, data["breaks"], data["grid"], vlim, data["alim"], s0, s1, False)
        full = batch.solve_batch(*args, strict=True)
        for kw in (dict(variant=3), dict()):
            fast = batch.solve_batch(*args, **kw)
            same(fast, full, ("K", "sd2", "u"), (kw,))
        assert (full["status"] == 0).any()


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 8])
def test_certified_lane_kernel_all_dofs(gpu, oracle, d):
    """Kernel family 3 for every dof it serves, odd batch sizes (idle lanes), per-trajectory grids and
    breakpoints, no velocity constraint, sd requested, non-zero boundary velocities: identical bits to
    the full iteration of family 2 and to the oracle."""
    B, N = 1000 + d, 60 + 7 * d
    data = batch.make_synthetic_batch(B, d, N, seed=40 + d, n_waypoints=4 + d % 3)
    rng = np.random.default_rng(d)
    sd0 = np.where(rng.random(B) < 0.5, 0.2 * rng.random(B), 0.0)
    sd1 = np.where(rng.random(B) < 0.5, 0.2 * rng.random(B), 0.0)
    grid_b = np.sort(np.concatenate([np.zeros((B, 1)), rng.random((B, N - 1)), np.ones((B, 1))], axis=1), axis=1)
    grid_b[:, 1:-1] = 0.5 * grid_b[:, 1:-1] + 0.5 * data["grid"][None, 1:-1]  # keep the steps away from zero
    breaks_b = np.repeat(data["breaks"][None], B, axis=0)
    cases = [
        (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"], sd0, sd1),
        (data["coef"], breaks_b, grid_b, data["vlim"], data["alim"], None, None),
        (data["coef"], data["breaks"], data["grid"], None, data["alim"], None, sd1),
    ]
    for ci, args in enumerate(cases):
        full = batch.solve_batch(*args, strict=True, want_sd=True)
        got = batch.solve_batch(*args, variant=3, want_sd=True)
        auto = batch.solve_batch(*args)
        same(got, full, ("K", "sd2", "sd", "u"), (ci, "family 3"))
        same(auto, full, ("K", "sd2", "u"), (ci, "automatic choice"))
    idx = np.arange(0, B, 7)
    ref = oracle.solve_batch(data["coef"][idx], data["breaks"], data["grid"], data["vlim"][idx], data["alim"][idx],
                             sd0[idx], sd1[idx], nthreads=0)
    got = batch.solve_batch(*cases[0], variant=3)
    same({k: got[k][idx] for k in ("K", "sd2", "u", "status")}, ref, ("K", "sd2", "u"), "oracle sample")


@pytest.mark.parametrize("B,d,N", [(40000, 7, 48), (700, 5, 60), (600, 12, 30)])
def test_controllable_sets_on_fast_kernels(gpu, oracle, B, d, N):
    """compute_controllable_sets(sdmin, sdmax) with sdmin != sdmax runs the backward scan of the fast
    kernels (family 3 for the large batch, family 2 for the small / 12-dof ones): oracle parity on a sample."""
    data = batch.make_synthetic_batch(B, d, N, seed=77 + d)
    rng = np.random.default_rng(B)
    sdmin = np.where(rng.random(B) < 0.5, 0.0, 0.2 * rng.random(B))
    sdmax = sdmin + np.where(rng.random(B) < 0.5, 0.0, 0.5 * rng.random(B))
    K = batch.controllable_sets_batch(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"], sdmin, sdmax)
    for b in rng.choice(B, size=120, replace=False):
        w = oracle.Wrapper(data["coef"][b], data["breaks"], data["grid"], data["vlim"][b], data["alim"][b])
        assert np.array_equal(K[b], w.compute_controllable_sets(sdmin[b], sdmax[b]), equal_nan=True), b


@pytest.mark.parametrize("B,N", [(1, 1), (3, 7), (63, 8), (65, 9), (130, 15), (64, 16), (100, 17), (70, 2100)])
def test_certified_lane_kernel_edge_shapes(gpu, oracle, B, N):
    """Family 3 at the edges of its launch geometry: single trajectories and partly filled waves, stage
    counts around the 8-stage output staging, a grid too long for its LDS copy (N = 2100)."""
    d = 4
    data = batch.make_synthetic_batch(B, d, N, seed=1000 + N)
    rng = np.random.default_rng(N)
    sd0, sd1 = 0.1 * rng.random(B), 0.1 * rng.random(B)
    args = (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"], sd0, sd1)
    got = batch.solve_batch(*args, variant=3, want_sd=True)
    full = batch.solve_batch(*args, strict=True, want_sd=True)
    same(got, full, ("K", "sd2", "sd", "u"), "full iteration")
    n = min(B, 8)
    ref = oracle.solve_batch(data["coef"][:n], data["breaks"], data["grid"], data["vlim"][:n], data["alim"][:n],
                             sd0[:n], sd1[:n], nthreads=0)
    same({k: got[k][:n] for k in ("K", "sd2", "u", "status")}, ref, ("K", "sd2", "u"), "oracle")


@pytest.mark.parametrize("B,d,N", [(300, 7, 50), (200, 12, 40), (129, 2, 33)])
def test_feasible_sets_on_fast_kernel(gpu, oracle, B, d, N):
    """compute_feasible_sets runs the rows-across-lanes kernel (incl. the final gridpoint's duplicated
    interpolation block and the warm-start state carried from stage to stage): oracle parity."""
    data = batch.make_synthetic_batch(B, d, N, seed=5 + d)
    X = batch.feasible_sets_batch(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])
    for b in range(0, B, 7):
        w = oracle.Wrapper(data["coef"][b], data["breaks"], data["grid"], data["vlim"][b], data["alim"][b])
        assert np.array_equal(X[b], w.compute_feasible_sets(), equal_nan=True), b


@pytest.mark.parametrize("interp", [True, False])
def test_feasible_sets_on_the_certified_lane_kernel(gpu, oracle, interp):
    """compute_feasible_sets at the headline shape runs family 3 (cert_feasible_kernel: certified answers for the min-x /
    max-x LPs of every stage, the reference's warm-start state carried along, the last gridpoint's own row set): every
    stage of all 65 536 trajectories -- plain and scaled by 1e-6..1 -- against the reference's full iteration for every
    LP (rows-across-lanes kernel, strict), fast and sound certificates, and a sample against the oracle."""
    B, d, N = 65536, 7, 200
    data = batch.make_synthetic_batch(B, d, N, seed=77)
    rng = np.random.default_rng(77)
    scale = np.where(rng.random((B, 1, 1, 1)) < 0.5, 1.0, 10.0 ** rng.uniform(-6, 0, size=(B, 1, 1, 1)))
    coef = data["coef"] * scale
    args = (coef, data["breaks"], data["grid"], data["vlim"], data["alim"], interp)
    full = batch.feasible_sets_batch(*args, variant=2, strict=True)
    for kw in (dict(), dict(variant=3), dict(variant=3, sound=True)):   # (auto picks family 3 at this size)
        same_array(batch.feasible_sets_batch(*args, **kw), full, (kw,))
    for b in range(0, B, 4099):
        w = oracle.Wrapper(coef[b], data["breaks"], data["grid"], data["vlim"][b], data["alim"][b], flags=oracle_flags(oracle, True, interp))
        assert np.array_equal(full[b], w.compute_feasible_sets(), equal_nan=True), b


def test_headline_batch_oracle_parity_every_trajectory(gpu, oracle):
    """All 65 536 trajectories of the headline batch, and an irregular batch of the same size (asymmetric
    and positive lower velocity limits, standing joints, non-uniform knots and grid, boundary velocities),
    against the oracle on every host thread: identical bits, trajectory by trajectory."""
    B, d, N = 65536, 7, 200
    data = batch.make_synthetic_batch(B, d, N)
    irregular = irregular_batch(B, d, N, 6, seed=4242)
    cases = [problem(data) + (None, None), problem(irregular) + (irregular["sd0"], irregular["sd1"])]
    for ci, args in enumerate(cases):
        got = batch.solve_batch(*args)
        ref = oracle.solve_batch(*args, nthreads=0)
        assert len(np.unique(ref["status"])) >= (1 if ci == 0 else 2)
        same(got, ref, ("K", "sd2", "u"), (ci,))


@pytest.mark.parametrize("B,d,N,seed", [(16384, 7, 120, 1), (16384, 4, 100, 2), (8192, 8, 80, 3)])
def test_near_parallel_rows_are_bit_exact(gpu, B, d, N, seed):
    """Adversarial for the certificates: one joint is a copy of another, scaled or tilted
    by 1e-14 .. 1e-6, so that two NON-twin constraint rows are parallel to that accuracy at every gridpoint and
    either can bind.  This is where the reference's absolute 1e-10 / 1e-8 classifications bite (it declares
    some of these problems infeasible); the default path must return the full iteration's bits, failures
    included."""
    args = near_parallel_family(B, d, N, seed)
    full = batch.solve_batch(*args, strict=True)
    assert (full["status"] == 1).sum() >= 1  # the reference itself trips over some of them
    for variant, sound in ((2, False), (3, False), (4, False), (2, True), (3, True)):
        fast = batch.solve_batch(*args, variant=variant, sound=sound)
        same(fast, full, ("K", "sd2", "u"), (variant, sound))


@pytest.mark.parametrize("B,d,N,seed", [(16384, 7, 60, 1), (16384, 4, 50, 2), (16384, 3, 40, 3), (8192, 8, 48, 4)])
def test_concurrent_rows_and_sliver_pivots_are_bit_exact(gpu, B, d, N, seed):
    """Aimed at what the certificates' margins (A)-(C) do not bound by themselves: an
    INTERMEDIATE pivot of the reference's iteration whose 1-D problem is a sliver -- rows visited earlier crossing
    the pivot row's line at almost the same point -- which the reference's arithmetic may declare empty although
    the LP has a well separated optimum elsewhere.  Generator: solve once, take a point P = (u_j, x_j) of the
    solution at a random stage j (it lies on the boundary of that stage's feasible polygon, where the scans'
    running optima pass), and move the acceleration limits of three joints so that their rows at s_j pass through P
    -- through P + an offset of 0 or 1e-8 .. 1e-2 -- to within 1e-13 .. 1e-8, each from a random side: three rows
    (with the original binding row: four) through one point at every scale between the solver's tolerances and the
    certificates' margins, in every visiting order; whole-path scalings 1e-3 .. 1e1 on top.

    What must hold since round 4: EVERY kernel family, with no flag, returns the full iteration's bits -- failures of the
    reference included.  (Rounds 2-3 shipped a faster default for families 2 and 3 that bounded the reference's last pivot
    only; on one trajectory in 57344 of this family (seed 4) it returned the LP's optimum where a sliver pivot ends the
    reference's run "infeasible".  The certificates now follow the reference's whole pivot trace: DESIGN.md section 3.1;
    tests/test_host_cert.py runs the same certificate source against the CPU restatement of the reference.)"""
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
    par = batch.constraint_params_batch(coef, data["breaks"], grid, data["vlim"], data["alim"])
    qs, qss = par["qs"][rows, j], par["qss"][rows, j]            # [B, d]: q'(s_j), q''(s_j)
    alim = data["alim"].copy()
    joints = np.argsort(rng.random((B, d)), axis=1)[:, :3]      # three distinct joints per trajectory
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
    args = (coef, data["breaks"], grid, data["vlim"], alim, None, sd1)
    full = batch.solve_batch(*args, strict=True)
    assert 0.02 < (full["status"] == 0).mean() < 0.999  # the family is hard: many of them fail in the reference too
    for variant in (4, 2, 3):
        if variant == 3 and d > 13:
            continue
        got = batch.solve_batch(*args, variant=variant)
        same(got, full, ("K", "sd2", "u"), (variant,))
        assert np.array_equal(batch.solve_batch(*args, variant=variant, sound=True)["K"], got["K"], equal_nan=True)  # the flag is a no-op
    # ... and `full` is not only the GPU's own full iteration: the first 512 trajectories against the CPU restatement of the
    # reference (oracle/, pinned to the reference's compiled solver), failures of the reference included
    from oracle import oracle as orc
    m = 512
    ref = orc.solve_batch(coef[:m], data["breaks"], grid, data["vlim"][:m], alim[:m], None, sd1[:m], nthreads=0)
    same({k: full[k][:m] for k in ("K", "sd2", "u", "status")}, ref, ("K", "sd2", "u"), "oracle")


def _tool(name):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("B,d,N,seed", [(768, 7, 60, 101), (768, 4, 50, 102), (512, 12, 40, 105)])
def test_sliver_family_against_the_references_own_compiled_solver(gpu, B, d, N, seed):
    """The one place the reference is known to FAIL -- an intermediate sliver pivot ends its run "infeasible" on an LP that
    has an optimum (cy_seidel_solverwrapper.pyx:127,:342,:353-355) -- against the reference ITSELF: its compiled
    cy_seidel_solverwrapper (oracle/_ref) under the reference's two passes (oracle/ref_solver_baseline.py), every kernel
    family and the default choice, K, sd, u and the failures bit for bit (a cut of tools/gpu_vs_reference_solver.py)."""
    rb = need_reference_solver()
    (coef, breaks, grid, vlim, alim, sd0, sd1), _ = _tool("gpu_sliver_hunt").family(B, d, N, seed)
    sd1 = np.round(np.asarray(sd1) * 1024) / 1024  # exact squares: ** in the reference's passes, sd * sd on the device
    ref = []
    for k in range(B):
        vel, acc = rb.constraint_tuples(coef[k], breaks, grid, vlim[k], alim[k])
        w = rb.make_wrapper([rb.PrecomputedConstraint(vel, False), rb.PrecomputedConstraint(acc, True)], None, grid)
        ref.append(rb.parameterization(w, 0.0, float(sd1[k])))
    nfail = sum(1 for x in ref if x[1] is None or np.isnan(x[1]).any())
    assert 0.05 * B < nfail < B  # the family does make the reference fail
    for variant in (0, 2, 3, 4):
        got = batch.solve_batch(coef, breaks, grid, vlim, alim, sd0, sd1, want_sd=True, variant=variant)
        for k in range(B):
            sdd, sd, K = ref[k]
            if sd is None:
                assert got["status"][k] != 0, (variant, k)
                continue
            assert np.array_equal(got["K"][k], K, equal_nan=True), (variant, k, "K")
            assert np.array_equal(got["sd"][k], sd, equal_nan=True), (variant, k, "sd")
            if not np.isnan(sd).any():
                assert np.array_equal(got["u"][k], sdd), (variant, k, "u")


@pytest.mark.parametrize("B,d,N,seed", [(1024, 7, 60, 31), (1024, 4, 50, 32), (512, 9, 40, 33)])
def test_a_valid_warm_start_of_the_lower_bound_lp_on_the_sliver_family(gpu, oracle, B, d, N, seed):
    """the lower-bound certificates follow the reference's COLD run.  With two distinct structural rows in
    the wrapper's active_c_up -- left by an earlier pass on the instance, carried in through tpr_problem.active -- the
    reference visits [up1, up0, ...] first: another trace, on which an intermediate sliver pivot may end its run where the
    cold run does not.  Kernel family 4 (the one that carries the state) must then iterate instead of certifying; here the
    state is seeded with random structural pairs on the sliver family and compared, state out included, with the CPU
    restatement's wrapper objects seeded the same way."""
    (coef, breaks, grid, vlim, alim, sd0, sd1), _ = _tool("gpu_sliver_hunt").family(B, d, N, seed)
    rng = np.random.default_rng(seed)
    nC = 2 + 4 * d
    active = np.zeros((B, 4), dtype=np.int32)
    active[:, 0] = rng.integers(0, nC, size=B)
    active[:, 1] = (active[:, 0] + rng.integers(1, nC, size=B)) % nC   # distinct structural rows: a valid warm start
    keep = rng.random(B) < 0.25
    active[keep, 2] = rng.integers(2, nC, size=keep.sum())              # some with a seeded upper-bound pair as well
    active[keep, 3] = (active[keep, 2] + 1 + rng.integers(0, nC - 3, size=keep.sum())) % nC
    seeded = active.copy()
    for variant in (4, 0):
        state = seeded.copy()
        got = batch.solve_batch(coef, breaks, grid, vlim, alim, sd0, sd1, active=state, variant=variant)
        for b in range(0, B, 2):
            w = oracle.Wrapper(coef[b], breaks, grid, vlim[b], alim[b])
            w.set_active(seeded[b])
            st, sdd, sd, xs, K = w.compute_parameterization(0.0, float(sd1[b]))
            assert st == got["status"][b], (variant, b)
            assert np.array_equal(K, got["K"][b], equal_nan=True), (variant, b, "K")
            if st == 0:
                assert np.array_equal(xs, got["sd2"][b]) and np.array_equal(sdd, got["u"][b]), (variant, b)
            assert np.array_equal(w.active(), state[b]), (variant, b, w.active(), state[b])

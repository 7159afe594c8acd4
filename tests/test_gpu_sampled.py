"""Any geometric path on the GPU: the sampled entries (tpr_sampled_rows_batch, the fused tpr_*_sampled_batch passes,
tpr_param_spline_samples_batch) against the numpy restatement of the rows (tests/sampled_ref.py), the dense-row passes on the
materialised rows, the CPU checker, the spline entries fed through their own samples, and the reference's stored results for
SimplePath / PolynomialPath / UnivariateSplineInterpolator / a trigonometric path (tests/golden/path_*.npz,
tools/make_golden_paths.py).  Every comparison is exact equality unless it says otherwise."""
import numpy as np
import pytest

import toppra_amd as ta
from tests import sampled_ref
from tests.helpers import assert_same
from tests.second_order_ref import batched_torque_model
from toppra_amd import batch
from toppra_amd.algorithm import BatchTOPPRA
from toppra_amd.solverwrapper import hipDenseSeidelWrapper, hipSampledSeidelWrapper

pytestmark = pytest.mark.gpu

ROWS = ("a", "b", "c", "low", "high", "deltas")
# dof and discretisation: 1 / 3 / 7 / 8 run on 8 lanes per trajectory, 9 / 16 on 16, 17 / 30 on 32 (30: the last that fits under
# Interpolation); 32 under Collocation (66 rows: 16 lanes, two dofs per slot column)
DOFS = [(1, True), (3, True), (7, True), (8, True), (9, True), (16, True), (17, True), (30, True), (32, False)]


def _problem(B, N, d, seed, per_traj_grid=False):
    """Random finite samples (not a path: the entries read nothing but the samples), some q' exactly 0 and of both signs."""
    rng = np.random.default_rng(seed)
    qs, qss = rng.standard_normal((B, N + 1, d)), rng.standard_normal((B, N + 1, d))
    qs[rng.random(qs.shape) < 0.08] = 0.0
    qs[rng.random(qs.shape) < 0.03] = -0.0
    vmax, amax = 1 + 2 * rng.random((B, d)), 2 + 3 * rng.random((B, d))
    vlim = np.stack([-vmax, vmax * (0.5 + rng.random((B, d)))], -1)
    alim = np.stack([-amax, amax * (0.5 + rng.random((B, d)))], -1)
    if per_traj_grid:
        grid = np.sort(rng.random((B, N + 1)), axis=1) + np.arange(N + 1) * 0.05
    else:
        grid = np.concatenate(([0.0], np.cumsum(0.5 + rng.random(N)))) / (N + 1)
    return grid, qs, qss, vlim, alim


def _blocks(rng, B, N, d):
    """One torque block (signed identity, dry friction, Collocation) and one dense-F block (per-trajectory F, Interpolation)."""
    w = [rng.standard_normal((B, N + 1, d)) for _ in range(3)]
    v = [rng.standard_normal((B, N + 1, 2)) for _ in range(3)]
    return [dict(w0=w[0], wa=w[1], wb=w[2], g=1 + rng.random(2 * d), friction=0.1 * rng.random((B, d)), interpolation=False),
            dict(w0=v[0], wa=v[1], wb=v[2], F=rng.standard_normal((B, 3, 2)), g=1 + rng.random((B, 3)), interpolation=True)]


def _cuda(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("d,interp", DOFS)
def test_sampled_rows_vs_restatement(gpu, d, interp):
    for k, (N, B) in enumerate([(1, 1), (2, 5), (7, 33), (40, 5), (40, 1)]):
        per_traj = k % 2 == 1
        grid, qs, qss, vlim, alim = _problem(B, N, d, 100 * d + k, per_traj)
        for vl, al in ((vlim, alim), (None, alim), (vlim, None)):
            want = sampled_ref.sampled_problem(grid, qs, qss, vl, al, interp)
            got = batch.sampled_rows_batch(grid, qs, qss, vl, al, interpolation=interp)
            for key in ROWS + ("xbound",):
                assert_same(got[key], want[key], "%s (N %d, B %d, vlim %s, alim %s)" % (key, N, B, vl is not None, al is not None))
        # with second-order blocks, where the stage still holds them (2 d + 6 more rows)
        nC = 2 + (4 if interp else 2) * d + 2 * d + 6
        if nC <= 122:
            blocks = _blocks(np.random.default_rng(k), B, N, d)
            want = sampled_ref.sampled_problem(grid, qs, qss, vlim, alim, interp, blocks)
            got = batch.sampled_rows_batch(grid, qs, qss, vlim, alim, blocks, interp)
            assert got["a"].shape[-1] == nC
            for key in ROWS:
                assert_same(got[key], want[key], key + " with blocks")
        else:
            blocks, got = [], batch.sampled_rows_batch(grid, qs, qss, vlim, alim, interpolation=interp)
        if k == 2:  # device tensors in, tensors out: with the blocks where the stage holds them, without at 30 / 32 dof
            tb = [{kk: (_cuda(vv) if isinstance(vv, np.ndarray) else vv) for kk, vv in blk.items()} for blk in blocks]
            dev = batch.sampled_rows_batch(_cuda(grid), _cuda(qs), _cuda(qss), _cuda(vlim), _cuda(alim), tb, interp)
            for key in ROWS + ("xbound",):
                assert dev[key].is_cuda
                assert_same(dev[key].cpu().numpy(), got[key], key + " (device tensors)")


def _passes(fn_kind, args, rows, interp, B, sd0, sd1, squared, active_s, active_d):
    """One pass through the sampled entry and through its dense twin on the materialised rows."""
    if fn_kind == "solve":
        return (batch.solve_sampled_batch(*args, sd0, sd1, interp, want_sd=True, squared=squared, active=active_s),
                batch.solve_dense_batch(*rows, sd0, sd1, want_sd=True, squared=squared, active=active_d))
    if fn_kind == "feasible":
        return batch.feasible_sets_sampled_batch(*args, interp, active=active_s), batch.feasible_sets_dense_batch(*rows, active=active_d)
    if fn_kind == "controllable":
        return (batch.controllable_sets_sampled_batch(*args, sd0, sd1, interp, squared=squared, active=active_s),
                batch.controllable_sets_dense_batch(*rows, sd0, sd1, squared=squared, active=active_d))
    if fn_kind == "reachable":
        return (batch.reachable_sets_sampled_batch(*args, sd0, sd1, interp, want_X=True, active=active_s, squared=squared),
                batch.reachable_sets_dense_batch(*rows, sd0, sd1, want_X=True, active=active_d, squared=squared))
    return (batch.solve_desired_duration_sampled_batch(*args, 3.0, sd0, sd1, 1e-5, interp, active=active_s, squared=squared),
            batch.solve_desired_duration_dense_batch(*rows, 3.0, sd0, sd1, 1e-5, active=active_d, squared=squared))


def _assert_pass(got, want, what):
    if isinstance(got, dict):
        assert sorted(got) == sorted(want)
        for key in got:
            assert_same(got[key], want[key], "%s: %s" % (what, key))
    elif isinstance(got, tuple):
        for j, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, "%s[%d]" % (what, j))
    else:
        assert_same(got, want, what)


@pytest.mark.parametrize("d,interp", DOFS)
def test_fused_passes_vs_dense_rows_and_checker(gpu, oracle, d, interp):
    """Every fused sampled pass = its *_dense_batch twin on the rows tpr_sampled_rows_batch materialised = the CPU checker's
    dense solve: K / X / L / sd2 / sd / u / status / alpha, NaN patterns and the warm-start state included."""
    lanes = 8 if 2 + (4 if interp else 2) * d <= 34 else (16 if 2 + (4 if interp else 2) * d <= 66 else 32)
    # one full block plus a partly idle one at 8 lanes (B = 33) and at 32 lanes (B = 9); small and odd shapes beside them
    shapes = [(1, 1), (2, 5), (7, 33 if lanes == 8 else 9), (40, 5)]
    for k, (N, B) in enumerate(shapes):
        grid, qs, qss, vlim, alim = _problem(B, N, d, 7000 + 100 * d + k, per_traj_grid=k == 1)
        if N >= 7:  # an infeasible trajectory beside feasible ones: an acceleration range of width 0 against a moving joint
            alim[B // 2, 0] = [1.0, 1.0]
            qs[B // 2, :, 0] = 1.0 + np.arange(N + 1)
        args = (grid, qs, qss, vlim, alim)
        mat = batch.sampled_rows_batch(*args, interpolation=interp)
        rows = tuple(mat[key] for key in ROWS)
        rng = np.random.default_rng(k)
        zeros = np.zeros(B)
        for sd0, sd1, squared in ((zeros, zeros, False), (0.05 * rng.random(B), 0.05 * rng.random(B), False),
                                  (0.002 * rng.random(B), 0.002 * rng.random(B), True)):
            got, want = _passes("solve", args, rows, interp, B, sd0, sd1, squared, None, None)
            _assert_pass(got, want, "solve (N %d, B %d)" % (N, B))
            chk = oracle.solve_dense_batch(*rows, np.sqrt(sd0) if squared else sd0, np.sqrt(sd1) if squared else sd1, want_X=True)
            if not squared:  # (the checker squares itself)
                for key in ("K", "sd2", "sd", "u", "status"):
                    assert_same(got[key], chk[key], "solve vs checker: " + key)
        if N >= 7:
            assert got["status"][B // 2] != 0 and (got["status"] == 0).any()
        assert_same(batch.feasible_sets_sampled_batch(*args, interp), chk["X"], "X vs checker")
        lo, hi = 0.02 * rng.random(B), 0.05 + 0.05 * rng.random(B)
        for kind in ("feasible", "controllable", "reachable", "sd"):
            got, want = _passes(kind, args, rows, interp, B, lo, hi if kind != "sd" else lo, False, None, None)
            _assert_pass(got, want, "%s (N %d, B %d)" % (kind, N, B))
        # passes chained on ONE warm-start state: feasible sets, reachable sets, solve, TOPPRAsd, controllable sets
        act_s, act_d = np.zeros((B, 4), np.int32), np.zeros((B, 4), np.int32)
        for kind in ("feasible", "reachable", "solve", "sd", "controllable"):
            got, want = _passes(kind, args, rows, interp, B, lo, hi if kind in ("controllable", "reachable") else lo, False, act_s, act_d)
            _assert_pass(got, want, "chained %s (N %d, B %d)" % (kind, N, B))
            assert np.array_equal(act_s, act_d), "warm-start state after " + kind
        assert act_s.any()
    # device tensors on the current stream
    targs = tuple(_cuda(v) for v in args)
    got = batch.solve_sampled_batch(*targs, interpolation=interp, want_sd=True)
    want = batch.solve_sampled_batch(*args, interpolation=interp, want_sd=True)
    for key in want:
        assert got[key].is_cuda
        assert_same(got[key].cpu().numpy(), want[key], "device tensors: " + key)


@pytest.mark.parametrize("d", [7, 12, 20])
def test_spline_batch_through_its_own_samples(gpu, d):
    """One shape per lane-group width: the sampled rows of tpr_path_eval_batch's samples are tpr_constraint_params_batch's rows,
    the sampled solve is the dense solve on them, the sampled spline parametrizer is tpr_param_spline_batch's generic variant."""
    B, N = 12, 25
    data = batch.make_synthetic_batch(B, d, N, seed=40 + d)
    sp = (data["coef"], data["breaks"], data["grid"])
    pe = batch.path_eval_batch(*sp)
    want = batch.constraint_params_batch(*sp, data["vlim"], data["alim"])
    got = batch.sampled_rows_batch(data["grid"], pe["qs"], pe["qss"], data["vlim"], data["alim"])
    for key in ("a", "b", "c", "low", "high", "xbound"):
        assert_same(got[key], want[key], key)
    deltas = np.diff(data["grid"])
    sol = batch.solve_sampled_batch(data["grid"], pe["qs"], pe["qss"], data["vlim"], data["alim"], want_sd=True)
    ref = batch.solve_dense_batch(want["a"], want["b"], want["c"], want["low"], want["high"], deltas, want_sd=True)
    for key in ref:
        assert_same(sol[key], ref[key], key)
    assert (sol["status"] == 0).all()
    a = batch.param_spline_samples_batch(data["grid"], pe["q"], pe["qs"], sol["sd"])
    b = batch.param_spline_batch(*sp, sol["sd"], variant=1)
    assert_same(a["counts"], b["counts"], "counts")
    assert_same(a["knot_times"], b["knot_times"], "knot_times")
    assert_same(a["coef"], b["coef"], "coef_t")


def test_param_spline_samples_ragged(gpu):
    """Dropped gridpoints (stretches of sd so large that the step takes < 1e-8 s), standing stretches and a NaN profile: counts,
    knot times and the coefficient table of the generic variant on the spline batch, exactly."""
    B, d, N = 9, 5, 40
    data = batch.make_synthetic_batch(B, d, N, seed=3)
    sp = (data["coef"], data["breaks"], data["grid"])
    pe = batch.path_eval_batch(*sp)
    rng = np.random.default_rng(5)
    sd = 0.2 + 3 * rng.random((B, N + 1))
    sd[:, 10:14] = 1e12
    sd[1, 20:23] = 0.0
    sd[2] = 1e12
    sd[3, 30:] = np.nan
    a = batch.param_spline_samples_batch(data["grid"], pe["q"], pe["qs"], sd)
    b = batch.param_spline_batch(*sp, sd, variant=1)
    assert (b["counts"][:2] < N + 1).all() and b["counts"][2] == 1
    assert_same(a["counts"], b["counts"], "counts")
    assert_same(a["knot_times"], b["knot_times"], "knot_times")
    assert_same(a["coef"], b["coef"], "coef_t")


FIXTURES = sampled_ref.fixtures()


def _fargs(f):
    return f["grid"], f["qs"][None], f["qss"][None], f["vlim"][None], f["alim"][None]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_stored_bits(gpu, name):
    """The reference's stored results from the stored samples: parameterizations, controllable / feasible / reachable sets,
    TOPPRAsd -- bit for bit; ParametrizeSpline within the bounds tests/test_gpu_param.py holds it to."""
    f = sampled_ref.load(name)
    args, interp = _fargs(f), f["interpolation"]
    for tag in ["zero", "pair"] + (["bad"] if "bad_pair" in f else []):
        s0, s1 = (0.0, 0.0) if tag == "zero" else f["bad_pair" if tag == "bad" else "pair"]
        got = batch.solve_sampled_batch(*args, np.array([s0]), np.array([s1]), interp, want_sd=True)
        assert int(got["status"][0]) == int(f[tag + "_status"]), tag
        for key, ref in (("K", "_K"), ("sd", "_sd"), ("u", "_u")):
            assert_same(got[key][0], f[tag + ref], "%s: %s" % (tag, key))
    lo, hi = (np.array([v]) for v in f["sets"])
    assert_same(batch.controllable_sets_sampled_batch(*args, lo, hi, interp)[0], f["K_set"], "K_set")
    assert_same(batch.feasible_sets_sampled_batch(*args, interp)[0], f["X"], "X")
    L, X = batch.reachable_sets_sampled_batch(*args, lo, hi, interp, want_X=True)
    assert_same(L[0], f["L"], "L")
    assert_same(X[0], f["X"], "X of the reachable-set pass")
    s0, s1 = f["sd_pair"]
    got = batch.solve_desired_duration_sampled_batch(*args, float(f["sd_desired"]), np.array([s0]), np.array([s1]), interpolation=interp)
    assert int(got["status"][0]) == int(f["sd_status"])
    for key in ("K", "sd", "u"):
        assert_same(got[key][0], f["sd_" + key], "TOPPRAsd: " + key)
    # ParametrizeSpline on the samples: 1e-12 relative on the duration, 1e-10 of the quantity's range on the samples
    sp = batch.param_spline_samples_batch(f["grid"], f["q"][None], f["qs"][None], f["traj_sd"][None])
    dur = sp["knot_times"][0, sp["counts"][0] - 1]
    print("%s: duration %r vs %r" % (name, dur, float(f["spline_duration"])))
    assert abs(dur - float(f["spline_duration"])) <= 1e-12 * float(f["spline_duration"])
    for order, key in enumerate(("spline_q", "spline_qd", "spline_qdd")):
        got = batch.ppoly_eval_batch(sp["coef"], sp["knot_times"], f["spline_ts"][None], order, sp["counts"])[0]
        dev, span = np.abs(got - f[key]).max(), np.ptp(f[key])
        print("%s: %s deviates by %.3g of a range of %.3g" % (name, key, dev, span))
        assert dev <= 1e-10 * span, key


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_through_the_drop_in_classes(gpu, oracle, name):
    """TOPPRA / TOPPRAsd built on the package's OWN path classes, as a user of the reference writes it: the results are the CPU
    checker's on rows from the path's own samples, and the stored ones where those samples are the stored samples bit for bit
    (another scipy / libm may evaluate a path differently: that comparison is skipped then, with the reason)."""
    f = sampled_ref.load(name)
    path = sampled_ref.make_path(f, ta)
    grid, interp = f["grid"], f["interpolation"]
    scheme = ta.constraint.DiscretizationType.Interpolation if interp else ta.constraint.DiscretizationType.Collocation

    def make(cls=ta.algorithm.TOPPRA):
        return cls([ta.constraint.JointVelocityConstraint(f["vlim"]), ta.constraint.JointAccelerationConstraint(f["alim"], scheme)],
                   path, gridpoints=grid)

    qs, qss = (np.asarray(path(grid, o), dtype=np.float64).reshape(len(grid), -1) for o in (1, 2))
    r = sampled_ref.sampled_problem(grid, qs[None], qss[None], f["vlim"][None], f["alim"][None], interp)
    rows = [r[k] for k in ROWS]
    inst = make()
    assert isinstance(inst.solver_wrapper, hipSampledSeidelWrapper)
    s0, s1 = (0.0, 0.0) if int(f["zero_status"]) == 0 else (float(f["pair"][0]), float(f["pair"][1]))
    sdd, sd, _, K = inst.compute_parameterization(s0, s1, return_data=True)
    chk = oracle.solve_dense_batch(*rows, np.array([s0]), np.array([s1]), want_X=True)
    assert_same(K, chk["K"][0], "K")
    assert_same(sd, chk["sd"][0], "sd")
    assert_same(sdd, chk["u"][0], "u")
    X = make().compute_feasible_sets()
    assert_same(X, chk["X"][0], "X")
    Kc = make().compute_controllable_sets(*f["sets"])
    L = make().compute_reachable_sets(*f["sets"])
    obj = make(ta.algorithm.TOPPRAsd)
    obj.set_desired_duration(float(f["sd_desired"]))
    sd_out = obj.compute_parameterization(float(f["sd_pair"][0]), float(f["sd_pair"][1]), return_data=True)
    chk_sd = oracle.solve_dense_batch_sd(*rows, float(f["sd_desired"]), np.array([f["sd_pair"][0]]), np.array([f["sd_pair"][1]]))
    assert_same(sd_out[1], chk_sd["sd"][0], "TOPPRAsd sd")
    assert_same(sd_out[0], chk_sd["u"][0], "TOPPRAsd u")
    for kind in ("ParametrizeSpline", "ParametrizeConstAccel"):
        traj = ta.algorithm.TOPPRA(inst.constraints, path, gridpoints=grid, parametrizer=kind).compute_trajectory(s0, s1)
        want = float(f["spline_duration" if kind == "ParametrizeSpline" else "accel_duration"])
        assert traj is not None and abs(traj.duration - want) <= 1e-9 * want
    assert len(ta.interpolator.propose_gridpoints(path, min_nb_points=20)) >= 20
    # controllable and reachable sets through the objects = the batch entries on the path's own samples
    sargs = (grid, qs[None], qss[None], f["vlim"][None], f["alim"][None])
    lo, hi = (np.array([v]) for v in f["sets"])
    assert_same(Kc, batch.controllable_sets_sampled_batch(*sargs, lo, hi, interp)[0], "K_set vs the batch entry")
    assert_same(L, batch.reachable_sets_sampled_batch(*sargs, lo, hi, interp)[0], "L vs the batch entry")
    # the single-LP compatibility entry on such a path: the values and the warm-start state of hipDenseSeidelWrapper on the
    # same constraints, call by call, and the state is the sampled wrapper's own (shared with its pass-level entries)
    mine = make().solver_wrapper
    theirs = hipDenseSeidelWrapper(mine.constraints, path, grid, solve_lp1d=1)
    N = len(grid) - 1
    for i, g, xb in ((N - 1, [0.0, -1.0], (np.nan, np.nan, 0.0, 0.0)), (N - 1, [0.0, 1.0], (np.nan, np.nan, 0.0, 0.0)),
                     (0, [-2 * (grid[1] - grid[0]), -1.0], (0.25, 0.25, np.nan, np.nan)), (N, [1e-9, 1.0], (np.nan,) * 4)):
        got = mine.solve_stagewise_optim(i, None, np.array(g), *xb)
        assert_same(got, theirs.solve_stagewise_optim(i, None, np.array(g), *xb), "solve_stagewise_optim at stage %d" % i)
        assert np.array_equal(mine._active, theirs._active)
    assert mine._active.any() and mine._dense._active is mine._active
    if not (np.array_equal(qs, f["qs"]) and np.array_equal(qss, f["qss"])):
        pytest.skip("this machine's scipy / numpy evaluates the path differently from the fixture's (max |dq'| %.3g): the stored "
                    "bits are compared from the stored samples in test_fixture_stored_bits" % np.abs(qs - f["qs"]).max())
    tag = "zero" if int(f["zero_status"]) == 0 else "pair"
    assert_same(K, f[tag + "_K"], "K vs stored")
    assert_same(sd, f[tag + "_sd"], "sd vs stored")
    assert_same(sdd, f[tag + "_u"], "u vs stored")
    assert_same(X, f["X"], "X vs stored")
    assert_same(Kc, f["K_set"], "K_set vs stored")
    assert_same(L, f["L"], "L vs stored")
    assert_same(sd_out[1], f["sd_sd"], "TOPPRAsd sd vs stored")
    assert_same(sd_out[0], f["sd_u"], "TOPPRAsd u vs stored")


def test_mixed_list_on_a_non_spline_path(gpu):
    """A torque constraint beside the limits on a SimplePath: the constraints no longer raise, and the dense wrapper serves it."""
    rng = np.random.default_rng(11)
    path = ta.SimplePath(np.array([0.0, 0.4, 1.0]), rng.standard_normal((3, 3)))
    grid = np.linspace(0, 1, 21)
    inv_dyn = lambda q, qd, qdd: 1.5 * qdd + 0.2 * np.sin(q) * (1 + qd * qd) + np.cos(q)  # noqa: E731
    cons = [ta.constraint.JointVelocityConstraint(2 * np.ones(3)), ta.constraint.JointAccelerationConstraint(4 * np.ones(3)),
            ta.constraint.JointTorqueConstraint(inv_dyn, np.stack([-8 * np.ones(3), 8 * np.ones(3)], -1), np.zeros(3))]
    inst = ta.algorithm.TOPPRA(cons, path, gridpoints=grid)
    assert isinstance(inst.solver_wrapper, hipDenseSeidelWrapper)
    sdd, sd, _ = inst.compute_parameterization(0, 0)
    assert sd is not None and np.isfinite(sd).all() and sd[0] == 0 and sd[-1] == 0


def test_from_path_samples_with_a_torque_constraint(gpu):
    """BatchTOPPRA.from_path_samples with a BatchJointTorqueConstraint: every pass equals the spline-built BatchTOPPRA of the same
    problem (its own samples handed over); without constraints the fused sampled passes equal the dense passes too."""
    B, d, N = 10, 4, 30
    data = batch.make_synthetic_batch(B, d, N, seed=77)
    rng = np.random.default_rng(8)
    model = batched_torque_model(1 + rng.random((B, d)), rng.random((B, d)), 0.1 * rng.random((B, d)))
    tau = np.stack([-30 * np.ones((B, d)), 30 * np.ones((B, d))], -1)
    make_con = lambda: [ta.constraint.BatchJointTorqueConstraint(model, tau, 0.05 * np.ones((B, d)))]  # noqa: E731
    sp = BatchTOPPRA(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"], constraints=make_con())
    pe = batch.path_eval_batch(data["coef"], data["breaks"], data["grid"])
    sm = BatchTOPPRA.from_path_samples(data["grid"], pe["q"], pe["qs"], pe["qss"], data["vlim"], data["alim"], constraints=make_con())
    for a, b in zip(sm.dense_rows(), sp.dense_rows()):
        assert_same(a, b, "dense rows")
    _assert_pass(sm.compute_parameterization(), sp.compute_parameterization(), "compute_parameterization")
    _assert_pass(sm.compute_parameterization_sd(4.0), sp.compute_parameterization_sd(4.0), "compute_parameterization_sd")
    _assert_pass(sm.compute_controllable_sets(0.0, 0.2), sp.compute_controllable_sets(0.0, 0.2), "controllable sets")
    _assert_pass(sm.compute_feasible_sets(), sp.compute_feasible_sets(), "feasible sets")
    _assert_pass(sm.compute_reachable_sets(0.0, 0.2), sp.compute_reachable_sets(0.0, 0.2), "reachable sets")
    # ParametrizeSpline: the generic fit on the same sd and samples -- knot times, counts and the coefficient table exactly
    ta_, res = sm.compute_trajectory(), sp.compute_parameterization()
    ref = batch.param_spline_batch(data["coef"], data["breaks"], data["grid"], res["sd"], variant=1)
    assert_same(ta_._sp["counts"], ref["counts"], "counts")
    assert_same(ta_._sp["knot_times"], ref["knot_times"], "knot_times")
    assert_same(ta_._sp["coef"], ref["coef"], "coef_t")
    assert_same(ta_.duration, ref["knot_times"][np.arange(B), ref["counts"] - 1], "duration")
    # without further constraints: the fused sampled passes against the materialised rows
    plain = BatchTOPPRA.from_path_samples(data["grid"], pe["q"], pe["qs"], pe["qss"], data["vlim"], data["alim"])
    rows = plain.dense_rows()
    _assert_pass(plain.compute_parameterization(), batch.solve_dense_batch(*rows, want_sd=True), "plain solve")
    _assert_pass(plain.compute_feasible_sets(), batch.feasible_sets_dense_batch(*rows), "plain X")
    traj = plain.compute_trajectory()
    assert (traj.status == 0).all() and np.isfinite(traj.duration).all()
    assert traj(np.linspace(0, 1, 5)[None] * traj.duration[:, None], 0).shape == (B, 5, d)

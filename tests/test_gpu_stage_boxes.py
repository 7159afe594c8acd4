"""First-order constraints of any kind on the GPU: tpr_stage_boxes_batch against the numpy restatement of the reference's fold
(tests/stage_boxes_ref.py: list order, the > / < spellings, the CPU oracle's velocity bound per gridpoint), every boxed sampled
pass against the CPU oracle's wrapper on the rows tpr_sampled_rows_batch writes with those boxes, and BatchTOPPRA with the new
constraint classes against the reference's stored results (tests/golden/boxes_*.npz, tools/make_golden_boxes.py).  Every
comparison is bit equality, status, NaN patterns and the sign of zeros included."""
import numpy as np
import pytest

import toppra_amd as ta
from tests import stage_boxes_ref as sbr
from tests.helpers import assert_same
from toppra_amd import batch
from toppra_amd.algorithm import BatchTOPPRA
from toppra_amd.constraint import BatchBoundConstraint, BatchJointVelocityConstraintVarying

pytestmark = pytest.mark.gpu
N = 30
ROWS = ("a", "b", "c")


def _cuda(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(got, want, what):
    assert_same(got, want, what)
    assert np.array_equal(np.signbit(got), np.signbit(want)), what + ": a zero's sign differs"


def _problem(B, d, seed, per_traj_grid=False, acc=True):
    """Random finite samples (the entries read nothing but the samples), some q' exactly +0 / -0; limits that vary along the
    path; an x cap and u bounds that bind on some stages."""
    rng = np.random.default_rng(seed)
    qs, qss = rng.standard_normal((B, N + 1, d)), rng.standard_normal((B, N + 1, d))
    qs[rng.random(qs.shape) < 0.08] = 0.0
    qs[rng.random(qs.shape) < 0.03] = -0.0
    vmax, amax = 1 + 2 * rng.random((B, d)), 2 + 3 * rng.random((B, d))
    vlim = np.stack([-vmax, vmax * (0.5 + rng.random((B, d)))], -1)
    alim = np.stack([-amax, amax * (0.5 + rng.random((B, d)))], -1) if acc else None
    if per_traj_grid:
        grid = np.sort(rng.random((B, N + 1)), axis=1) + np.arange(N + 1) * 0.05
    else:
        grid = np.concatenate(([0.0], np.cumsum(0.5 + rng.random(N)))) / (N + 1)
    vgrid = vlim[:, None] * (1 + 0.5 * np.sin(9 * np.broadcast_to(grid, (B, N + 1))))[:, :, None, None]
    xb = np.stack([np.zeros((B, N + 1)), np.where(rng.random((B, N + 1)) < 0.4, 0.02 + 0.2 * rng.random((B, N + 1)), 1e4)], -1)
    ub = np.stack([-(0.5 + rng.random((B, N + 1))), 0.5 + rng.random((B, N + 1))], -1)
    return {"grid": grid, "qs": qs, "qss": qss, "vlim": vlim, "alim": alim, "vgrid": vgrid, "xb": xb, "ub": ub, "B": B, "d": d}


# ---- 1. the box kernel ----------------------------------------------------------------------------------------------
def _extreme(p):
    """A handful of gridpoints carrying limits at the edge of the number range (the `extreme` family's kinds)."""
    vg = p["vgrid"].copy()
    vg[:, 2] = [-np.inf, np.inf]
    vg[:, 5, ::2] *= 1e38
    vg[:, 9, 1::2] *= 1e300
    vg[:, 13] = vg[:, 13, :, ::-1]           # an inverted pair
    vg[:, 17] *= 1e-30                        # the fp32 square underflows to 0
    vg[:, 21] *= 10.0 ** -21                  # ... or is subnormal
    vg[:, 25, 0] = [-np.inf, 1.0]             # one-sided
    vg[:, 27, :, 0] = 0.25 * vg[:, 27, :, 1]  # a velocity range that excludes 0
    return vg


def _source_lists(p):
    B, d = p["B"], p["d"]
    xb, ub, vg, vl = p["xb"], p["ub"], p["vgrid"], p["vlim"]
    # a +0.0 / -0.0 tie placed on purpose: both orders keep a different zero (a > b ? a : b keeps b on a tie)
    xa, xz = xb.copy(), xb.copy()
    xa[:, ::4, 0], xz[:, ::4, 0] = 0.0, -0.0
    xz[:, 1::4, 1], xa[:, 1::4, 1] = 0.0, -0.0
    ua, uz = ub.copy(), ub.copy()
    ua[:, ::3, 1], uz[:, ::3, 1] = 0.0, -0.0
    yield "vlim", [("vlim", vl)]
    yield "vlim shared", [("vlim", vl[0])]
    yield "vlim_grid", [("vlim_grid", vg)]
    yield "vlim_grid shared", [("vlim_grid", vg[0])]
    yield "xbound", [("xbound", xb)]
    yield "xbound shared", [("xbound", xb[0])]
    yield "ubound", [("ubound", ub)]
    yield "ubound shared", [("ubound", ub[0])]
    yield "tie x", [("xbound", xa), ("xbound", xz)]
    yield "tie x reversed", [("xbound", xz), ("xbound", xa)]
    yield "tie u", [("ubound", ua), ("ubound", uz[0])]
    yield "tie u reversed", [("ubound", uz[0]), ("ubound", ua)]
    yield "vlim, grid, x", [("vlim", vl), ("vlim_grid", vg), ("xbound", xa)]
    yield "x, grid, vlim", [("xbound", xa), ("vlim_grid", vg), ("vlim", vl)]
    yield "grid, u, x shared, vlim shared", [("vlim_grid", vg), ("ubound", ub), ("xbound", xz[0]), ("vlim", vl[0])]
    yield "extreme", [("vlim_grid", _extreme(p)), ("vlim", vl)]
    yield "extreme reversed", [("vlim", vl), ("vlim_grid", _extreme(p))]
    yield "eight", [("vlim", vl), ("vlim_grid", vg), ("xbound", xb), ("ubound", ub), ("xbound", xz), ("ubound", uz), ("vlim_grid", vg[0]), ("xbound", xa[0])]
    yield "none", []


@pytest.mark.parametrize("B,d", [(37, 3), (21, 9), (11, 17), (5, 32), (70, 7), (1, 1)])
def test_stage_boxes_vs_restatement(gpu, oracle, B, d):
    p = _problem(B, d, 10 * d + B)
    if B > 1:
        assert (p["qs"] == 0).any() and np.signbit(p["qs"][p["qs"] == 0]).any()
    for what, src in _source_lists(p):
        want = sbr.stage_boxes(oracle, p["qs"], src, B, N)
        got = batch.stage_boxes_batch(p["qs"], src)
        for g, w, name in zip(got, want, ("low", "high")):
            _bits(g, w, "%s: %s (B %d, d %d)" % (what, name, B, d))
        if what == "tie x":
            keep = got
        if what == "tie x reversed":  # the order decides which zero survives
            assert (np.signbit(keep[0]) != np.signbit(got[0])).any() and (np.signbit(keep[1]) != np.signbit(got[1])).any()
    if B > 1:  # the extreme limits alone: an underflowing square, no bound at all, a subnormal square
        xhi = batch.stage_boxes_batch(p["qs"], [("vlim_grid", _extreme(p))])[1][:, :, 1]
        assert (xhi == 0).any() and (xhi == 1e8).any() and ((xhi > 0) & (xhi < 1e-37)).any()
    # device tensors in, tensors out
    src = [("vlim", _cuda(p["vlim"])), ("vlim_grid", _cuda(p["vgrid"])), ("xbound", _cuda(p["xb"][0])), ("ubound", _cuda(p["ub"]))]
    want = batch.stage_boxes_batch(p["qs"], [(k, v.cpu().numpy()) for k, v in src])
    got = batch.stage_boxes_batch(_cuda(p["qs"]), src)
    for g, w in zip(got, want):
        assert g.is_cuda
        _bits(g.cpu().numpy(), w, "device tensors")


def test_stage_boxes_without_samples_and_across_tiles(gpu, oracle):
    """Bound-only sources need no samples; 300 x 31 gridpoints span many 256-gridpoint tiles with a partial last one."""
    p = _problem(300, 2, 5)
    src = [("ubound", p["ub"]), ("xbound", p["xb"][0])]
    want = sbr.stage_boxes(oracle, None, src, 300, N)
    for g, w in zip(batch.stage_boxes_batch(None, src, N=N), want):
        _bits(g, w, "no samples")
    src = [("vlim_grid", p["vgrid"]), ("vlim", p["vlim"][0])]
    for g, w in zip(batch.stage_boxes_batch(p["qs"], src), sbr.stage_boxes(oracle, p["qs"], src, 300, N)):
        _bits(g, w, "many tiles")


# ---- 2. the boxed passes against the oracle ---------------------------------------------------------------------------
def _oracle_wrappers(oracle, rows):
    for b in range(rows[0].shape[0]):
        yield oracle.DenseWrapper(*[np.ascontiguousarray(v[b]) for v in rows])


SHAPES = [(3, True, 37, True), (9, True, 21, False), (17, True, 11, True), (32, False, 5, False), (5, None, 5, True), (7, True, 70, False)]


@pytest.mark.parametrize("d,interp,B,per_traj", SHAPES)
def test_boxed_passes_vs_oracle(gpu, oracle, d, interp, B, per_traj):
    """8 / 16 / 32 lanes per trajectory with a partly idle second block, 32 dof on 16 lanes under Collocation, no acceleration
    constraint (nC = 2), and 70 trajectories for the reachable sets' lane kernel (more than one 64-lane block)."""
    p = _problem(B, d, 900 + d, per_traj, acc=interp is not None)
    interp = bool(interp)
    src = [("vlim", p["vlim"]), ("vlim_grid", p["vgrid"]), ("ubound", p["ub"]), ("xbound", p["xb"])]
    low, high = batch.stage_boxes_batch(p["qs"], src)
    for g, w in zip((low, high), sbr.stage_boxes(oracle, p["qs"], src, B, N)):
        _bits(g, w, "boxes")
    mat = batch.sampled_rows_batch(p["grid"], p["qs"], p["qss"], None, p["alim"], interpolation=interp)
    rows = tuple(mat[k] for k in ROWS) + (low, high, mat["deltas"])
    args = (p["grid"], p["qs"], p["qss"], p["alim"], low, high)
    rng = np.random.default_rng(d)
    sd0, sd1 = 0.05 * rng.random(B), 0.05 * rng.random(B)
    sd0[::5] = 1e5  # uncontrollable starts: outside the +-1e8 box itself
    for s0, s1 in ((np.zeros(B), np.zeros(B)), (sd0, sd1)):
        got = batch.solve_sampled_boxed_batch(*args, s0, s1, interp, want_sd=True)
        chk = oracle.solve_dense_batch(*rows, s0, s1, want_X=True)
        for key in ("status", "K", "sd2", "sd", "u"):
            assert_same(got[key], chk[key], "solve: " + key)
    assert (got["status"] == 1).any() and (got["status"][::5] == 1).all()
    # every shape, 32 dof on 16 lanes included, runs successful forward scans with a profile that moves (checked on the oracle)
    assert (chk["status"] == 0).any() and np.nanmax(chk["sd"]) > 0.1
    assert_same(batch.feasible_sets_sampled_boxed_batch(*args, interp), chk["X"], "X")
    lo, hi = 0.02 * rng.random(B), 0.05 + 0.05 * rng.random(B)
    K = batch.controllable_sets_sampled_boxed_batch(*args, lo, hi, interp)
    L, X = batch.reachable_sets_sampled_boxed_batch(*args, lo, hi, interp, want_X=True)
    for b, w in enumerate(_oracle_wrappers(oracle, rows)):
        assert_same(K[b], w.compute_controllable_sets(float(lo[b]), float(hi[b])), "K_set[%d]" % b)
    for b, w in enumerate(_oracle_wrappers(oracle, rows)):
        Lw, Xw = w.compute_reachable_sets(float(lo[b]), float(hi[b]))
        assert_same(L[b], Lw, "L[%d]" % b)
        assert_same(X[b], Xw, "X of the reachable pass [%d]" % b)
    got = batch.solve_desired_duration_sampled_boxed_batch(*args, 3.0, sd1, sd1, 1e-5, interp)
    chk = oracle.solve_dense_batch_sd(*rows, 3.0, sd1, sd1)
    for key in ("status", "K", "sd2", "sd", "u", "alpha"):
        assert_same(got[key], chk[key], "TOPPRAsd: " + key)
    # passes chained on ONE warm-start state, as on one wrapper object: feasible sets, reachable sets, solve, controllable sets
    act = np.zeros((B, 4), np.int32)
    Xc = batch.feasible_sets_sampled_boxed_batch(*args, interp, active=act)
    a1 = act.copy()
    Lc = batch.reachable_sets_sampled_boxed_batch(*args, lo, hi, interp, active=act)
    a2 = act.copy()
    sol = batch.solve_sampled_boxed_batch(*args, sd1, sd1, interp, want_sd=True, active=act)
    a3 = act.copy()
    Kc = batch.controllable_sets_sampled_boxed_batch(*args, lo, hi, interp, active=act)
    for b, w in enumerate(_oracle_wrappers(oracle, rows)):
        assert_same(Xc[b], w.compute_feasible_sets(), "chained X[%d]" % b)
        assert np.array_equal(a1[b], w.active()), ("state after the feasible sets", b)
        assert_same(Lc[b], w.compute_reachable_sets(float(lo[b]), float(hi[b]))[0], "chained L[%d]" % b)
        assert np.array_equal(a2[b], w.active()), ("state after the reachable sets", b)
        st, sdd, sd, xs, Kw = w.compute_parameterization(float(sd1[b]), float(sd1[b]))
        assert sol["status"][b] == st
        assert_same(sol["K"][b], Kw, "chained K[%d]" % b)
        if st != 1:
            assert_same(sol["sd2"][b], xs, "chained sd2[%d]" % b); assert_same(sol["u"][b], sdd, "chained u[%d]" % b)
        assert np.array_equal(a3[b], w.active()), ("state after the solve", b)
        assert_same(Kc[b], w.compute_controllable_sets(float(lo[b]), float(hi[b])), "chained K_set[%d]" % b)
        assert np.array_equal(act[b], w.active()), ("state after the controllable sets", b)
    assert act.any()
    # device tensors on the current stream
    targs = tuple(_cuda(v) for v in args)
    dev = batch.solve_sampled_boxed_batch(*targs, _cuda(sd1), _cuda(sd1), interp, want_sd=True)
    host = batch.solve_sampled_boxed_batch(*args, sd1, sd1, interp, want_sd=True)
    for key in host:
        assert dev[key].is_cuda
        assert_same(dev[key].cpu().numpy(), host[key], "device tensors: " + key)


# ---- 3. / 5. BatchTOPPRA on a spline table ----------------------------------------------------------------------------
@pytest.mark.parametrize("torch_in", [False, True])
def test_constant_grid_of_limits_gives_the_fused_path(gpu, torch_in):
    """The batch twin of test_varying_velocity_limits_with_a_constant_function_give_the_fused_path: limits that do not depend on
    s, given per gridpoint, return the bits of the fused compute_parameterization with the same vlim.  The callable is called
    once, with every gridpoint, and never again: the boxes are built once per object."""
    B, d = 37, 7
    data = batch.make_synthetic_batch(B, d, N, seed=77)
    conv = _cuda if torch_in else (lambda x: x)
    coef, breaks, grid, vlim, alim = (conv(data[k]) for k in ("coef", "breaks", "grid", "vlim", "alim"))
    want = BatchTOPPRA(coef, breaks, grid, vlim, alim).compute_parameterization(want_sd=True)
    calls = []

    def vlim_func(s):
        calls.append(tuple(s.shape))
        return vlim[:, None].expand(B, N + 1, d, 2) if torch_in else np.broadcast_to(vlim[:, None], (B, N + 1, d, 2))

    def shared(s):  # [N+1] gridpoints -> [N+1, d, 2]: one grid of limits for the whole batch
        calls.append(tuple(s.shape))
        return vlim[0].expand(N + 1, d, 2) if torch_in else np.broadcast_to(vlim[0], (N + 1, d, 2))
    host = lambda v: v.cpu().numpy() if torch_in else v  # noqa: E731
    with pytest.raises(ValueError, match="must return"):
        BatchTOPPRA(coef, breaks, grid, None, alim, constraints=[BatchJointVelocityConstraintVarying(vlim_func)]).compute_feasible_sets()
    calls.clear()
    inst = BatchTOPPRA(coef, breaks, grid, None, alim, constraints=[BatchJointVelocityConstraintVarying(vlim_func(grid[None].expand(B, N + 1) if torch_in else np.broadcast_to(grid, (B, N + 1))))])
    calls.clear()
    got = inst.compute_parameterization(want_sd=True)
    for key in ("status", "K", "sd2", "sd", "u"):
        assert_same(host(got[key]), host(want[key]), key)
    assert (host(got["status"]) == 0).all()
    # a callable, one grid of limits for the whole batch: trajectory 0's limits for everyone
    v0 = vlim[:1].expand(B, d, 2).contiguous() if torch_in else np.ascontiguousarray(np.broadcast_to(vlim[:1], (B, d, 2)))
    want0 = BatchTOPPRA(coef, breaks, grid, v0, alim)
    inst = BatchTOPPRA(coef, breaks, grid, None, alim, constraints=[BatchJointVelocityConstraintVarying(shared)])
    got = inst.compute_parameterization(want_sd=True)
    assert calls == [(N + 1,)]
    ref = want0.compute_parameterization(want_sd=True)
    for key in ("status", "K", "sd2", "sd", "u"):
        assert_same(host(got[key]), host(ref[key]), "callable: " + key)
    assert_same(host(inst.compute_feasible_sets()), host(want0.compute_feasible_sets()), "X")
    assert_same(host(inst.compute_controllable_sets(0.0, 0.1)), host(want0.compute_controllable_sets(0.0, 0.1)), "K_set")
    assert_same(host(inst.compute_reachable_sets(0.0, 0.1)), host(want0.compute_reachable_sets(0.0, 0.1)), "L")
    low, high = inst.stage_boxes()
    assert calls == [(N + 1,)] and tuple(low.shape) == (B, N + 1, 2)  # five passes, one call
    tr, tr0 = inst.compute_trajectory(), want0.compute_trajectory()
    assert_same(host(tr.duration), host(tr0.duration), "duration")
    assert calls == [(N + 1,)]


# ---- 4. the reference's stored bits through BatchTOPPRA ----------------------------------------------------------------
def _check_fixture(inst, f, host, what):
    B = f["qs"].shape[0]
    for tag, pair in (("zero", np.zeros((B, 2))), ("pair", f["pair"]), ("bad", np.broadcast_to(f["bad_pair"], (B, 2)))):
        out = inst.compute_parameterization(pair[:, 0].copy(), pair[:, 1].copy(), want_sd=True)
        assert np.array_equal(host(out["status"]), f[tag + "_status"]), (what, tag)
        for key in ("K", "sd", "u"):
            assert_same(host(out[key]), f[tag + "_" + key], "%s %s: %s" % (what, tag, key))
    assert_same(host(inst.compute_controllable_sets(*f["sets"])), f["K_set"], what + ": K_set")
    assert_same(host(inst.compute_feasible_sets()), f["X"], what + ": X")
    assert_same(host(inst.compute_reachable_sets(*f["sets"])), f["L"], what + ": L")
    out = inst.compute_parameterization_sd(f["sd_desired"])
    assert np.array_equal(host(out["status"]), f["sd_status"])
    for key in ("K", "sd", "u"):
        assert_same(host(out[key]), f["sd_" + key], "%s TOPPRAsd: %s" % (what, key))
    low, high = inst.stage_boxes()
    _bits(host(low), f["low_ref"], what + ": low_arr")
    _bits(host(high), f["high_ref"], what + ": high_arr")


@pytest.mark.parametrize("torch_in", [False, True])
@pytest.mark.parametrize("name", sbr.fixtures())
def test_fixture_stored_bits(gpu, name, torch_in):
    """[Varying, Acceleration], [Velocity, Varying, Acceleration, bound-only], [Acceleration (Collocation), bound-only] on the boxed
    entries and [Varying, Torque] on rows + boxes + the dense entries, from the spline table and from the stored samples."""
    f = sbr.load(name)
    cond = sbr.binding_conditions(f)  # a kernel that ignores a bound cannot pass
    assert cond["ok"] and min(cond.get("vary", [5])) >= 5 and min(cond.get("vary_box", [5])) >= 5 and min(cond.get("xcap", [5])) >= 5 and min(cond.get("ucap", [3])) >= 3
    conv = _cuda if torch_in else (lambda x: x)
    host = (lambda v: v.cpu().numpy()) if torch_in else (lambda v: v)
    vlim, alim, cons = sbr.batch_arguments(f, conv)
    inst = BatchTOPPRA(conv(f["coef"]), conv(f["breaks"]), conv(f["grid"]), vlim, alim, interpolation=f["interpolation"], constraints=cons)
    _check_fixture(inst, f, host, name + " (spline table)")
    # the output parametrizer reads sd only: durations against the existing entry on the stored sd
    traj = inst.compute_trajectory(parametrizer="ParametrizeSpline")
    sp = batch.param_spline_batch(f["coef"], f["breaks"], f["grid"], f["zero_sd"])
    want = sp["knot_times"][np.arange(4), sp["counts"] - 1]
    assert_same(host(traj.duration), want, name + ": duration")
    vlim, alim, cons = sbr.batch_arguments(f, conv)
    inst = BatchTOPPRA.from_path_samples(conv(f["grid"]), conv(f["q"]), conv(f["qs"]), conv(f["qss"]), vlim, alim,
                                         interpolation=f["interpolation"], constraints=cons)
    _check_fixture(inst, f, host, name + " (samples)")
    sp = batch.param_spline_samples_batch(f["grid"], f["q"], f["qs"], f["zero_sd"])
    assert_same(host(inst.compute_trajectory(parametrizer="ParametrizeSpline").duration), sp["knot_times"][np.arange(4), sp["counts"] - 1],
                name + ": duration from samples")


def test_mixed_list_order_and_callable_on_samples(gpu, oracle):
    """First-order constraints in any position among the second-order ones: the sources are [vlim, first-order in list order],
    the rows carry no velocity box of their own."""
    from tests.second_order_ref import batched_torque_model
    f = sbr.load("boxes_d_d7_N40")
    B, d = 4, 7
    model = batched_torque_model(f["mass"], f["grav"], f["cori"])
    tq = lambda: ta.constraint.BatchJointTorqueConstraint(model, np.stack([-f["taumax"], f["taumax"]], -1), f["fric"])  # noqa: E731
    vl = 1.5 * f["vlim0"]
    xb = np.stack([np.zeros((B, 41)), np.full((B, 41), 0.5)], -1)
    calls = []

    def vf(s):
        calls.append(s.shape)
        return f["vgrid"][0]
    lists = ([BatchBoundConstraint(xbound=xb), tq(), BatchJointVelocityConstraintVarying(vf)],
             [tq(), BatchBoundConstraint(xbound=xb), BatchJointVelocityConstraintVarying(f["vgrid"][:1].repeat(B, 0))])
    outs = []
    for cons in lists:
        inst = BatchTOPPRA.from_path_samples(f["grid"], f["q"], f["qs"], f["qss"], vl, None, constraints=cons)
        a, b, c, low, high, deltas = inst.dense_rows()
        want = sbr.stage_boxes(oracle, f["qs"], [("vlim", vl), ("xbound", xb), ("vlim_grid", f["vgrid"][0])], B, 40)
        _bits(low, want[0], "low"); _bits(high, want[1], "high")
        outs.append(inst.compute_parameterization(want_sd=True))
        chk = oracle.solve_dense_batch(a, b, c, low, high, deltas)
        for key in ("status", "K", "sd", "u"):
            assert_same(outs[-1][key], chk[key], key)
    assert calls == [(41,)]
    for key in outs[0]:
        assert_same(outs[0][key], outs[1][key], "list order of first- among second-order constraints: " + key)

"""The control-point kernels on the MI355X.  The yardstick of the bit-for-bit tests is the EXISTING tool kernels: a point (k, r)
is the tool of the chain cut after link k with tool = r, the build contracts nothing and the new kernels spell the tool kernels'
expressions in their order, so speeds, accelerations and both fused terms must equal the tool entries on the cut chain in every
bit, for every dof and point set of tests/control_points_cases.py.  Then the calling conventions, ``BatchPointAccelerationConstraint``
against the same limit through the batched callback route, ``BatchPointSpeedConstraint`` against a ``BatchBoundConstraint`` fed a
host-made bound, both beside every other chain constraint, accuracy against the numpy recursion, and the reference's fixtures.

Accuracy (B = 5, N = 40; the bound is 16 x the float64 reference's own error against np.longdouble, per case, point set and
quantity; profiles/control_points_accuracy.json holds the yardsticks, the bounds and the measured errors): measured on the
MI355X the kernels use at most 0.94 of a bound (the squared speed at 17 dof, set b; 0.87 for wb and 0.29 for wa, both at 32
dof, set b -- the bits of the tool kernels on the cut chains, so their share too), and at most 0.12 of the stored bound on the
reference's fixtures, whose sd they reproduce to 7.1e-15 / 6.3e-14 (tolerances 1.3e-9 / 4.9e-11)."""
import numpy as np
import pytest

from tests import chain_cases as cc, chain_ref, control_points_cases as cp, rigid_support as rs, second_order_ref as sor
from tests.helpers import golden

pytestmark = pytest.mark.gpu
FIXTURES = ("control_points_d6_N40", "control_points_d4_N30_colloc")
IDS = ["%d%s" % c for c in cp.CASES]


def _cut_chains(chain, links, offsets):
    """[(k, the SerialChain cut after link k with tool = r)] of the points, in their order."""
    d = len(chain["joint_type"])
    return [(k, chain_ref.serial_chain(cp.truncated(chain, k, r))) for k, r in zip(cp.resolved(d, links), offsets)]


def _stacked_tool_accelerations(cuts):
    """The batched callback of the route the constraint replaces: one launch of the tool kernel per point, on its cut chain."""
    def inv_dyn(q, qd, qdd):
        parts = [sc.tool_acceleration(q[..., :k + 1], qd[..., :k + 1], qdd[..., :k + 1])[..., :3] for k, sc in cuts]
        return np.concatenate(parts, -1) if isinstance(q, np.ndarray) else __import__("torch").cat(parts, -1)
    return inv_dyn


@pytest.mark.parametrize("d,which", cp.CASES, ids=IDS)
def test_every_point_equals_the_tool_kernels_on_the_cut_chain(gpu, d, which):
    chain, q, qs, qss = cc.case(d)
    links, offsets = cp.point_set(d, which)
    sc, pts = chain_ref.serial_chain(chain), cp.control_points(d, which)
    P, zero = len(links), np.zeros_like(q)
    speed2 = sc.point_speeds(q, qs, pts)
    acc = sc.point_accelerations(q, qs, qss, pts)
    wa, wb = sc.point_acceleration_terms(q, qs, qss, pts)
    assert speed2.shape == (cc.B, cc.N + 1, P) and acc.shape == wa.shape == wb.shape == (cc.B, cc.N + 1, P, 3)
    for p, (k, cut) in enumerate(_cut_chains(chain, links, offsets)):
        qk, qsk, qssk = q[..., :k + 1], qs[..., :k + 1], qss[..., :k + 1]  # (non-contiguous views)
        assert not qk.flags["C_CONTIGUOUS"] or k + 1 == d
        assert np.array_equal(speed2[..., p], cut.tool_velocity_norm(qk, qsk)), (p, k, "speed")
        assert np.array_equal(acc[..., p, :], cut.tool_acceleration(qk, qsk, qssk)[..., :3]), (p, k, "acc")
        ta, tb = cut.tool_acceleration_terms(qk, qsk, qssk)
        assert np.array_equal(wa[..., p, :], ta[..., :3]) and np.array_equal(wb[..., p, :], tb[..., :3]), (p, k, "terms")
    # each fused term equals the single evaluation on the same arguments
    assert np.array_equal(wb, acc) and np.array_equal(wa, sc.point_accelerations(q, zero, qs, pts))
    w0 = sc.point_accelerations(q, zero, zero, pts)
    assert not w0.any() and not np.signbit(w0).any()
    assert not wa[2].any() and not np.signbit(wa[2]).any() and not speed2[2].any()  # the trajectory that stands still
    # the bound of the whole set is one array: (0, min_p limit_p / speed2_p), +inf where every point stands still
    from toppra_amd import batch
    limit = np.random.default_rng(d).uniform(0.1, 1.0, (cc.B, P))
    again, xbound = batch.chain_points_speed_batch(sc, q, qs, pts, limit)
    assert np.array_equal(again, speed2) and not xbound[..., 0].any()
    with np.errstate(divide="ignore"):
        assert np.array_equal(xbound[..., 1], np.min(limit[:, None, :] / speed2, -1))
    assert np.all(np.isposinf(xbound[2, :, 1]))
    if which == "b" and d > 1:  # the point at the chain's own tool: the tool constraint's bound
        assert np.array_equal(batch.chain_points_speed_batch(sc, q, qs, cp.ControlPoints([-1], [chain["tool"]]), limit[:, 1:2])[1],
                              batch.chain_tool_bound_batch(sc, q, qs, limit[:, 1])[1])


@pytest.mark.parametrize("d,which", [(1, "c"), (7, "b"), (9, "d"), (32, "c")], ids=["1c", "7b", "9d", "32c"])
def test_device_tensors_and_views_give_the_host_call_s_bits(gpu, d, which):
    """torch tensors on the device, contiguous and as a non-contiguous view, a flattened shape, a single point."""
    torch, dev = rs.torch_device()
    chain, q, qs, qss = cc.case(d)
    sc, pts = chain_ref.serial_chain(chain), cp.control_points(d, which)
    P = pts.count
    host = sc.point_acceleration_terms(q, qs, qss, pts)
    speed2 = sc.point_speeds(q, qs, pts)
    tq, tqs, tqss = (torch.from_numpy(np.array(v)).to(dev) for v in (q, qs, qss))
    for got, want in zip(sc.point_acceleration_terms(tq, tqs, tqss, pts), host):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    got = sc.point_speeds(tq, tqs, pts)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), speed2)
    wide = [torch.repeat_interleave(t, 2, dim=1) for t in (tq, tqs, tqss)]
    views = [w[:, ::2] for w in wide]
    assert not views[0].is_contiguous()
    assert np.array_equal(sc.point_accelerations(*views, pts).cpu().numpy(), host[1])
    assert np.array_equal(sc.point_speeds(views[0], views[1], pts).cpu().numpy(), speed2)
    for got, want in zip(sc.point_acceleration_terms(*views, pts), host):
        assert np.array_equal(got.cpu().numpy(), want)
    flat = sc.point_accelerations(tq.reshape(-1, d), tqs.reshape(-1, d), tqss.reshape(-1, d), pts)
    assert tuple(flat.shape) == (cc.B * (cc.N + 1), P, 3) and np.array_equal(flat.cpu().numpy(), host[1].reshape(-1, P, 3))
    flat = sc.point_speeds(tq.reshape(-1, d), tqs.reshape(-1, d), pts)
    assert tuple(flat.shape) == (cc.B * (cc.N + 1), P) and np.array_equal(flat.cpu().numpy(), speed2.reshape(-1, P))
    assert np.array_equal(sc.point_accelerations(q[1, 3], qs[1, 3], qss[1, 3], pts), host[1][1, 3])
    one = sc.point_acceleration_terms(q[1, 3], qs[1, 3], qss[1, 3], pts)
    assert one[0].shape == (P, 3) and np.array_equal(one[0], host[0][1, 3]) and np.array_equal(one[1], host[1][1, 3])
    assert np.array_equal(sc.point_speeds(q[1, 3], qs[1, 3], pts), speed2[1, 3])
    # a device limit, [B, P]
    from toppra_amd import batch
    limit = np.random.default_rng(d).uniform(0.1, 1.0, (cc.B, P))
    xb = batch.chain_points_speed_batch(sc, tq, tqs, pts, torch.from_numpy(limit).to(dev))[1]
    assert np.array_equal(xb.cpu().numpy(), batch.chain_points_speed_batch(sc, q, qs, pts, limit)[1])


def _peak(chain, links, offsets, args):
    """max |wb| per point [P] over the problem's gridpoints, from the CPU reference."""
    q, qs, qss = sor.path_samples(*args[:3])
    return np.abs(cp.point_accelerations(chain, links, offsets, q, qs, qss)).max((0, 1, 3))


def _signed_identity(P):
    F = np.zeros((6 * P, 3 * P))
    for p in range(P):
        F[6 * p:6 * p + 3, 3 * p:3 * p + 3], F[6 * p + 3:6 * p + 6, 3 * p:3 * p + 3] = np.eye(3), -np.eye(3)
    return F


@pytest.mark.parametrize("scheme", ["Collocation", "Interpolation"])
@pytest.mark.parametrize("source", ["spline", "samples"])
@pytest.mark.parametrize("per_traj", [False, True])
def test_the_acceleration_constraint_equals_the_callback_route(gpu, scheme, source, per_traj):
    """Against BatchSecondOrderConstraint(callback, F, g), the callback stacking the cut chains' tool accelerations: the dense
    rows and all five passes, bit for bit; the limits leave every trajectory feasible."""
    from toppra_amd import constraint
    d, which = 7, "b"
    chain = cc.case(d)[0]
    links, offsets = cp.point_set(d, which)
    sc, pts = chain_ref.serial_chain(chain), cp.control_points(d, which)
    P = pts.count
    data, args = rs.problem(d)
    # positive on both sides (standing still satisfies it) and a generous multiple of each point's largest |wb|
    hi = 2.0 * _peak(chain, links, offsets, args)[:, None] * (1.0 + np.random.default_rng(9).random((cc.B, P, 3) if per_traj else (P, 3)))
    linear = np.stack([-1.5 * hi, hi], -1)  # [P, 3, 2] or [B, P, 3, 2]
    DT = getattr(constraint.DiscretizationType, scheme)
    ours = constraint.BatchPointAccelerationConstraint(sc, pts, linear=linear, discretization_scheme=DT)
    F = _signed_identity(P)
    g = np.concatenate((linear[..., 1], -linear[..., 0]), -1).reshape(linear.shape[:-3] + (6 * P,))
    assert np.array_equal(ours.F, F) and np.array_equal(ours.g, g)
    out = rs.compare(source, data, args, ours, _stacked_tool_accelerations(_cut_chains(chain, links, offsets)), F, g, DT)
    assert out["rows"][0].shape[-1] == 2 + 4 * d + (12 if scheme == "Interpolation" else 6) * P


def test_a_dense_F_equals_the_callback_route(gpu):
    """Five rows that mix the points: a one-sided polytope over all nine components."""
    from toppra_amd import constraint
    d, which = 7, "b"
    chain = cc.case(d)[0]
    links, offsets = cp.point_set(d, which)
    sc, pts = chain_ref.serial_chain(chain), cp.control_points(d, which)
    data, args = rs.problem(d)
    F = np.random.default_rng(11).uniform(-1.0, 1.0, (5, 3 * pts.count))
    g = 2.0 * np.abs(F).reshape(5, pts.count, 3).sum(-1) @ _peak(chain, links, offsets, args)
    ours = constraint.BatchPointAccelerationConstraint(sc, pts, F=F, g=g)
    theirs = constraint.BatchSecondOrderConstraint(_stacked_tool_accelerations(_cut_chains(chain, links, offsets)), F, g)
    results = [rs.run_passes(rs.instance("spline", data, args, [con])) for con in (ours, theirs)]
    rs.same(results[0], results[1], "constraint vs callback")
    assert np.all(results[0]["compute_parameterization"]["status"] == 0)


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("limits", ["scalar", "per_point", "per_traj"])
def test_the_speed_constraint_equals_a_host_made_bound(gpu, kind, limits):
    """Against BatchBoundConstraint(xbound = (0, min_p limit_p / s_p)) with the bound computed on the host from point_speeds:
    stage_boxes() and every pass, bit for bit."""
    from toppra_amd import algorithm, batch, constraint
    d, which = 7, "b"
    chain = cc.case(d)[0]
    sc, pts = chain_ref.serial_chain(chain), cp.control_points(d, which)
    P = pts.count
    data, args = rs.problem(d, seed=6)
    limit = {"scalar": 0.2, "per_point": np.array([0.05, 0.4, 0.1]),
             "per_traj": np.random.default_rng(3).uniform(0.05, 0.8, (cc.B, P))}[limits]
    pe = batch.path_eval_batch(*args[:3])
    speed2 = sc.point_speeds(pe["q"], pe["qs"], pts)
    with np.errstate(divide="ignore"):
        hi = np.min(np.broadcast_to(limit, (cc.B, P))[:, None, :] / speed2, -1)
    xbound = np.stack([np.zeros_like(hi), hi], -1)
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v  # noqa: E731
    ours_limit = limit
    if kind == "torch":
        torch, dev = rs.torch_device()
        args = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in args)
        xbound = torch.from_numpy(xbound).to(dev)
        if limits == "per_traj":
            ours_limit = torch.from_numpy(limit).to(dev)
    ours = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchPointSpeedConstraint(sc, pts, ours_limit)])
    theirs = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchBoundConstraint(xbound=xbound)])
    for a, b in zip(ours.stage_boxes(), theirs.stage_boxes()):
        assert np.array_equal(host(a), host(b))
    results = []
    for inst in (ours, theirs):
        out = rs.run_passes(inst)
        results.append({k: ({n: host(x) for n, x in v.items()} if isinstance(v, dict) else [host(x) for x in v] if isinstance(v, (tuple, list))
                            else host(v)) for k, v in out.items()})
    rs.same(results[0], results[1], "constraint vs host-made bound")
    assert np.all(results[0]["compute_parameterization"]["status"] == 0)
    high = host(ours.stage_boxes()[1])
    assert (high[..., 1] < sor.velocity_box(host(pe["qs"]), data["vlim"])[1][..., 1]).any(), "the speed limit tightens no box"
    # the set's bound is the tightest of its points': no single point gives these boxes
    single = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchPointSpeedConstraint(
        sc, cp.ControlPoints([int(pts.links[0])], [pts.offsets[0]]), 0.2)]).stage_boxes()[1]
    if limits == "scalar":
        assert np.all(high <= host(single)) and (high < host(single)).any()


def test_a_standstill_stage_leaves_the_box(gpu):
    """q' = 0 at a gridpoint: every point stands still, each bound is +inf and the stage keeps the 1e8 of the box; a point on link 0
    of a chain whose first joint does not move stands still alone and drops out of the minimum."""
    from toppra_amd import algorithm, constraint
    d = 3
    chain, q, qs, qss = cc.case(d)
    sc, pts = chain_ref.serial_chain(chain), cp.control_points(d, "b")
    qs = np.array(qs)
    qs[:, 7] = 0.0
    qs[:, 9, 0] = 0.0  # link 0 at rest at stage 9: a point on it gives +inf there, the others bound the stage
    grid = np.linspace(0.0, 1.0, cc.N + 1)
    alim = np.tile([-50.0, 50.0], (cc.B, d, 1))
    inst = algorithm.BatchTOPPRA.from_path_samples(grid, q, qs, qss, None, alim, constraints=[constraint.BatchPointSpeedConstraint(sc, pts, 0.25)])
    low, high = inst.stage_boxes()
    assert np.all(high[:, 7, 1] == 1e8) and np.all(high[2, :, 1] == 1e8)  # the stage; the trajectory that stands still
    assert np.all(high[[0, 1, 3, 4], 8, 1] < 1e8) and np.all(low[..., 1] == 0.0)
    base = cp.ControlPoints([0, -1], [[0.1, 0.2, 0.3], chain["tool"]])
    speed2 = sc.point_speeds(q, qs, base)
    assert not speed2[:, 9, 0].any() and np.all(speed2[[0, 1, 3, 4], 9, 1] > 0)
    high = algorithm.BatchTOPPRA.from_path_samples(grid, q, qs, qss, None, alim,
                                                   constraints=[constraint.BatchPointSpeedConstraint(sc, base, 0.25)]).stage_boxes()[1]
    assert np.array_equal(high[[0, 1, 3, 4], 9, 1], 0.25 / speed2[[0, 1, 3, 4], 9, 1])


def test_beside_the_other_chain_constraints(gpu):
    """[torque, tool acceleration, point acceleration, wrench, tool speed, point speed] of one chain in one list: every pass
    runs, the dense rows hold each block with the rows of that constraint alone, the boxes are those of the two speed limits."""
    from toppra_amd import algorithm, batch, constraint
    from toppra_amd.chain import Payload
    d, which = 7, "b"
    chain = cc.case(d)[0]
    links, offsets = cp.point_set(d, which)
    sc, pts = chain_ref.serial_chain(chain), cp.control_points(d, which)
    data, args = rs.problem(d, seed=8)
    pe = batch.path_eval_batch(*args[:3])
    taumax = np.abs(sc.torque_terms(pe["q"], pe["qs"], pe["qss"])[0]).max() + 20.0
    body = Payload(0.5, com=(0.0, 0.0, 0.05))
    wrench = sc.tool_wrench_terms(pe["q"], pe["qs"], pe["qss"], body)
    fmax = 3.0 * max(np.abs(w[..., :3]).max() for w in wrench)
    tool_peak = np.abs(sc.tool_acceleration_terms(pe["q"], pe["qs"], pe["qss"])[1][..., :3]).max()
    makers = [lambda: constraint.BatchJointTorqueConstraint(sc, np.tile([-taumax, taumax], (d, 1)), np.zeros(d)),
              lambda: constraint.BatchCartesianAccelerationConstraint(sc, linear=2.0 * tool_peak),
              lambda: constraint.BatchPointAccelerationConstraint(sc, pts, linear=2.0 * _peak(chain, links, offsets, args)),
              lambda: constraint.BatchToolWrenchConstraint(sc, body, force=fmax)]
    speeds = lambda: [constraint.BatchCartesianVelocityNormConstraint(sc, 0.3), constraint.BatchPointSpeedConstraint(sc, pts, 0.2)]  # noqa: E731
    inst = algorithm.BatchTOPPRA(*args, constraints=[m() for m in makers[:2]] + speeds()[:1] + [m() for m in makers[2:]] + speeds()[1:])
    out = rs.run_passes(inst)
    rs.passes_ran(out)
    first = 2 + 4 * d
    widths = [2 * d, 12, 12 * pts.count, 12]  # (torque: Collocation; the others: Interpolation)
    assert out["rows"][0].shape[-1] == first + sum(widths)
    at = first
    for make, width in zip(makers, widths):
        alone = algorithm.BatchTOPPRA(*args, constraints=[make()]).dense_rows()
        for k in range(3):
            assert np.array_equal(out["rows"][k][..., at:at + width], alone[k][..., first:]), (at, k)
        at += width
    low, high = algorithm.BatchTOPPRA(*args, constraints=speeds()).stage_boxes()
    assert np.array_equal(out["rows"][3], low) and np.array_equal(out["rows"][4], high)


@pytest.mark.parametrize("d,which", cp.CASES, ids=IDS)
def test_kernels_against_the_numpy_reference(gpu, d, which):
    """Within 16 x the float64 reference's own error against np.longdouble, per case and quantity (the metric of chain_cases)."""
    chain, q, qs, qss = cc.case(d)
    sc, pts = chain_ref.serial_chain(chain), cp.control_points(d, which)
    ref = cp.reference(d, which)
    wa, wb = sc.point_acceleration_terms(q, qs, qss, pts)
    for name, val in (("speed2", sc.point_speeds(q, qs, pts)), ("wa", wa), ("wb", wb)):
        err, bound = cc.metric(val, ref[name], ref[name + "_mag"]), cp.bound(d, which, name)
        print("ACCURACY case %d%s %s error %.3g bound %.3g fraction %.2f" % (d, which, name, err, bound, err / bound if bound else 0.0))
        assert err <= bound, (d, which, name, err, bound)


@pytest.mark.parametrize("name", FIXTURES)
def test_against_the_reference_s_fixtures(gpu, name):
    """wa / wb within the stored accuracy bound, the constraint's rows within the allowance composed from it, low / high and
    return codes equal, sd within the stored end-to-end tolerance (tools/make_control_points_golden.py)."""
    from toppra_amd import constraint
    from toppra_amd.chain import ControlPoints
    fx = golden(name)
    chain = rs.fixture_chain(fx)
    sc, pts = chain_ref.serial_chain(chain), ControlPoints(fx["links"], fx["offsets"])
    B, d, P = fx["coef"].shape[0], fx["coef"].shape[3], len(fx["links"])
    q, qs, qss = sor.path_samples(fx["coef"], fx["breaks"], fx["grid"])
    ev = cp.evaluations(q, qs, qss)
    mags = {k: cp.point_accelerations(chain, fx["links"], fx["offsets"], *ev[k], absolute=True).reshape(B, -1, 3 * P) for k in ("wa", "wb")}
    got = dict(zip(("wa", "wb"), (w.reshape(B, -1, 3 * P) for w in sc.point_acceleration_terms(q, qs, qss, pts))))
    rs.fixture_accuracy(name, fx, got, mags)
    interp, DT = rs.fixture_scheme(fx)
    con = constraint.BatchPointAccelerationConstraint(sc, pts, linear=fx["linear"], discretization_scheme=DT)
    assert np.array_equal(con.F, fx["F"]) and np.array_equal(con.g, fx["g"])
    rows = rs.fixture_solve(name, fx, con, interp)
    # The rows' allowance, composed as for the tool-acceleration fixtures (tests/test_gpu_tool_accel.py) through the rows' own
    # assembly: w0 is an exact zero on both sides, a = F wa may be off by |F| (bound_wa mag_wa), b = F wb alike, under
    # Interpolation the second half by the same sums of its parts; c = -g has no allowance from the kernels.  On top, 4 eps of the
    # row with its VALUES in absolute value: every row of F has a single non-zero entry, so its dot product rounds nothing.
    F, g = np.abs(fx["F"]), np.broadcast_to(fx["g"], (B, fx["g"].shape[-1]))  # (one of the fixtures shares its limits)
    deltas = np.broadcast_to(np.diff(fx["grid"]), (B, len(fx["grid"]) - 1))
    zero_w, zero_g, eps = np.zeros_like(fx["wa"]), np.zeros_like(g), np.finfo(np.float64).eps
    bw = {k: fx["acc_bound"][i] * mags[k] for i, k in enumerate(("wa", "wb"))}
    allow = [np.abs(r) for r in sor.block_rows(zero_w, bw["wa"], bw["wb"], np.abs(qs), deltas, F, zero_g, None, interp)[:2]]
    size = [np.abs(r) for r in sor.block_rows(zero_w, np.abs(fx["wa"]), np.abs(fx["wb"]), np.abs(qs), deltas, F, zero_g, None, interp)[:2]]
    tiled = np.tile(np.abs(g), 2 if interp else 1)[:, None, :]
    allow.append(np.zeros_like(tiled))
    size.append(tiled)
    for k, stored, al, sz in zip("abc", (fx["rows_a"], fx["rows_b"], fx["rows_c"]), allow, size):
        block = rows["abc".index(k)][:, :, 2 + 4 * d:]
        tol = np.broadcast_to(al + 4 * eps * sz, block.shape)
        bad = np.abs(block - stored) > tol
        worst = float(np.max(np.abs(block - stored)[tol > 0] / tol[tol > 0]))
        print("ACCURACY fixture %s rows_%s error_over_allowance %.3g" % (name, k, worst))
        assert not bad.any(), (name, k, worst)


def test_entries_refuse_a_bad_chain_before_any_launch(gpu):
    """The tool entries' refusals hold for the new ones: a dof outside 1..32, a NULL chain array, an unknown joint type, a
    joint_type array on the device, more than 2^31 - 1 points -- the buffers handed over are a few doubles long."""
    import ctypes
    from toppra_amd import _capi
    lib = _capi.load()
    sc = chain_ref.serial_chain(cc.case(3)[0])
    one = np.zeros(6)
    p = one.ctypes.data
    pts = cp.ControlPoints([0, 2], np.zeros((2, 3))).c_struct(sc)
    x = ctypes.byref(pts)
    BADARG, UNSUPPORTED = -1, -3

    def calls(model, B=2, N=1):
        m = ctypes.byref(model)
        return (lib.tpr_chain_points_speed_batch(m, x, B, N, p, p, p, p, p, 0, None),
                lib.tpr_chain_points_acceleration_batch(m, x, B * (N + 1), p, p, p, p, 0, None),
                lib.tpr_chain_points_acceleration_terms_batch(m, x, B, N, p, p, p, p, p, 0, None))

    def model(**kw):
        m, keep = sc.c_struct(one)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    assert calls(model(d=0)) == (BADARG,) * 3 and calls(model(d=33)) == (BADARG,) * 3
    for field in ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity", "tool"):
        assert calls(model(**{field: None})) == (BADARG,) * 3, field
    codes = np.array([0, 2, 1], dtype=np.int32)
    assert calls(model(joint_type=codes.ctypes.data)) == (BADARG,) * 3
    torch, dev = rs.torch_device()
    on_device = torch.zeros(3, dtype=torch.int32, device=dev)
    assert calls(model(joint_type=on_device.data_ptr())) == (BADARG,) * 3
    assert calls(model(), B=1 << 20, N=(1 << 11) - 1) == (UNSUPPORTED,) * 3  # 2^31 points
    assert lib.tpr_chain_points_acceleration_batch(ctypes.byref(model()), x, -1, p, p, p, p, 0, None) == BADARG
    # ... and the valid call on the same model still runs
    assert np.isfinite(sc.point_accelerations(np.zeros(3), np.zeros(3), np.zeros(3), cp.ControlPoints([0, 2], np.zeros((2, 3))))).all()

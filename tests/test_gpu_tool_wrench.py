"""The tool-wrench kernels on the MI355X: the single and the fused entry against the numpy reference (tests/tool_wrench_ref.py)
within the accuracy bound of tests/tool_wrench_cases.py, the fused outputs against the single entry bit for bit, the exact zeros,
the calling conventions, ``BatchToolWrenchConstraint`` against the same limit fed through the batched callback route, the
reference's fixtures, and the constraint in one list with the torque, the tool-speed and the tool-acceleration limit.

Accuracy (B = 5, N = 40; the bound is 16 x the float64 reference's own error against np.longdouble, per case and quantity;
profiles/tool_wrench_accuracy.json holds the yardsticks, the bounds and the measured errors): measured on the MI355X the kernels
use at most 0.27 of a bound (wb and the single evaluation, at 32 dof; 0.19 for wa, 0.08 for w0), and at most 0.12 of the stored
bound on the reference's fixtures, whose sd they reproduce to 5.3e-15 / 2.7e-13 (tolerances 3.8e-9 / 3.3e-12)."""
import numpy as np
import pytest

from tests import chain_cases as cc, chain_ref, rigid_support as rs, second_order_ref as sor, tool_wrench_cases as tw, tool_wrench_ref as twr
from tests.helpers import golden

pytestmark = pytest.mark.gpu
FIXTURES = ("tool_wrench_d6_N40", "tool_wrench_d4_N30_colloc")
NAMES = ("w0", "wa", "wb")
I3, Z3 = np.eye(3), np.zeros((3, 3))
F_BOTH = np.block([[I3, Z3], [-I3, Z3], [Z3, I3], [Z3, -I3]])
GRAVITY = np.array([0.3, -0.2, -9.81])


@pytest.mark.parametrize("d", tw.DOFS)
def test_kernels_against_the_numpy_reference(gpu, d):
    """Both entries, from numpy arrays; each fused output equals the single evaluation on the same arguments in every bit."""
    chain, q, qs, qss = cc.case(d)
    sc, obj = chain_ref.serial_chain(chain), twr.payload_of(tw.PAYLOAD, chain)
    w0, wa, wb = sc.tool_wrench_terms(q, qs, qss, obj)
    single = sc.tool_wrench(q, qs, qss, obj)
    assert w0.shape == wa.shape == wb.shape == single.shape == (cc.B, cc.N + 1, 6)
    rs.check(tw, d, {"w0": w0, "wa": wa, "wb": wb, "wrench": single})
    zero = np.zeros_like(q)
    assert np.array_equal(w0, sc.tool_wrench(q, zero, zero, obj)) and np.array_equal(wa, sc.tool_wrench(q, zero, qs, obj))
    assert np.array_equal(wb, single)
    for v in (w0, wa, wb):  # a zero leaves as +0, so equal values are equal bits
        assert not np.signbit(v[v == 0]).any()
    assert np.array_equal(wa[2], w0[2])  # the trajectory that stands still: level 1 on an exactly zero q' is level 0
    if not chain["gravity"].any():
        assert not w0.any() and not np.signbit(w0).any()
    else:
        assert np.all(np.abs(w0[..., :3]).max(-1) > 0)


@pytest.mark.parametrize("d", (3, 8, 17))
def test_at_rest_the_force_is_the_weight(gpu, d):
    """Gravity on, the contact frame's origin at the centre of mass: |f| = m |gravity| to the bound and the moment is zero."""
    chain, q, qs, qss = cc.case(d)
    assert chain["gravity"].any()
    centred = dict(tw.PAYLOAD, origin=tw.PAYLOAD["com"])
    sc = chain_ref.serial_chain(chain)
    zero = np.zeros_like(q)
    w0 = sc.tool_wrench_terms(q, qs, qss, twr.payload_of(centred, chain))[0]
    ref, mag = twr.tool_wrench(chain, centred, q, zero, zero), twr.tool_wrench(chain, centred, q, zero, zero, absolute=True)
    bound = tw.BOUND_FACTOR * cc._own_error(ref, twr.tool_wrench(chain, centred, q, zero, zero, dtype=np.longdouble), mag)
    err = cc.metric(w0, ref, mag)
    weight = tw.PAYLOAD["mass"] * np.linalg.norm(chain["gravity"])
    off = np.abs(np.linalg.norm(w0[..., :3], axis=-1) - weight)
    allow = bound * np.linalg.norm(mag[..., :3], axis=-1) + 4 * np.finfo(np.float64).eps * weight
    print("d %d: error %.3g, bound %.3g; | |f| - m |g| | at most %.3g of its allowance" % (d, err, bound, float((off / allow).max())))
    assert err <= bound and np.all(off <= allow)
    assert not w0[..., 3:].any() and not np.signbit(w0[..., 3:]).any()


@pytest.mark.parametrize("d", (2, 8))
def test_a_zero_payload_gives_positive_zeros(gpu, d):
    from toppra_amd.chain import Payload
    chain, q, qs, qss = cc.case(d)
    sc = chain_ref.serial_chain(chain)
    nothing = Payload(0.0, com=(0.1, -0.2, 0.3), frame_rotation=tw.PAYLOAD["rot"], frame_origin=(0.0, 0.1, 0.0))
    for v in sc.tool_wrench_terms(q, qs, qss, nothing) + (sc.tool_wrench(q, qs, qss, nothing),):
        assert not v.any() and not np.signbit(v).any()


@pytest.mark.parametrize("d", tw.DOFS)
def test_device_tensors_and_views_give_the_host_call_s_bits(gpu, d):
    """torch tensors on the device, contiguous and as a non-contiguous view, a flattened shape, a single point."""
    torch, dev = rs.torch_device()
    chain, q, qs, qss = cc.case(d)
    sc, obj = chain_ref.serial_chain(chain), twr.payload_of(tw.PAYLOAD, chain)
    host = sc.tool_wrench_terms(q, qs, qss, obj)
    tq, tqs, tqss = (torch.from_numpy(np.array(v)).to(dev) for v in (q, qs, qss))
    for got, want in zip(sc.tool_wrench_terms(tq, tqs, tqss, obj), host):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    wide = [torch.repeat_interleave(t, 2, dim=1) for t in (tq, tqs, tqss)]
    views = [w[:, ::2] for w in wide]
    assert not views[0].is_contiguous()
    assert np.array_equal(sc.tool_wrench(*views, obj).cpu().numpy(), host[2])
    for got, want in zip(sc.tool_wrench_terms(*views, obj), host):
        assert np.array_equal(got.cpu().numpy(), want)
    flat = sc.tool_wrench(tq.reshape(-1, d), tqs.reshape(-1, d), tqss.reshape(-1, d), obj)
    assert tuple(flat.shape) == (cc.B * (cc.N + 1), 6) and np.array_equal(flat.cpu().numpy(), host[2].reshape(-1, 6))
    assert np.array_equal(sc.tool_wrench(q[1, 3], qs[1, 3], qss[1, 3], obj), host[2][1, 3])
    one = sc.tool_wrench_terms(q[1, 3], qs[1, 3], qss[1, 3], obj)
    assert all(np.array_equal(one[k], host[k][1, 3]) for k in range(3))


def _case7():
    """The 7-dof chain under gravity (the shared case has it switched off), its SerialChain and the payload."""
    chain = dict(cc.case(7)[0], gravity=GRAVITY)
    return chain, chain_ref.serial_chain(chain), twr.payload_of(tw.PAYLOAD, chain)


def _peak(chain, args):
    """Per component, the largest of |w0|, |wa|, |wb| over the problem's gridpoints, from the CPU reference: limits above it
    hold at rest (F w0 < g) with room, so every trajectory is feasible."""
    q, qs, qss = sor.path_samples(*args[:3])
    return np.max([np.abs(twr.tool_wrench(chain, tw.PAYLOAD, *a)).max((0, 1)) for a in list(tw.evaluations(q, qs, qss).values())[:3]], 0)


def _compare(source, data, args, ours, F, g, DT):
    """The constraint against BatchSecondOrderConstraint(chain.tool_wrench with the payload bound, F, g): rows and all five passes."""
    sc, obj = ours.chain, ours.payload
    return rs.compare(source, data, args, ours, lambda q, qd, qdd: sc.tool_wrench(q, qd, qdd, obj), F, g, DT)


@pytest.mark.parametrize("scheme", ["Collocation", "Interpolation"])
@pytest.mark.parametrize("source", ["spline", "samples"])
@pytest.mark.parametrize("per_traj", [False, True])
def test_the_constraint_equals_the_callback_route(gpu, scheme, source, per_traj):
    """A dense F -- five rows that mix force and moment -- with a shared or a per-trajectory g."""
    from toppra_amd import constraint
    d = 7
    chain, sc, obj = _case7()
    data, args = rs.problem(d)
    rng = np.random.default_rng(11)
    F = rng.uniform(-1.0, 1.0, (5, 6))
    g = 1.5 * (np.abs(F) @ _peak(chain, args))
    if per_traj:
        g = g * (1.0 + rng.random((cc.B, 5)))
    DT = getattr(constraint.DiscretizationType, scheme)
    out = _compare(source, data, args, constraint.BatchToolWrenchConstraint(sc, obj, F=F, g=g, discretization_scheme=DT), F, g, DT)
    assert out["rows"][0].shape[-1] == 2 + 4 * d + (10 if scheme == "Interpolation" else 5)


@pytest.mark.parametrize("per_traj", [False, True])
def test_force_and_moment_boxes_equal_their_explicit_rows(gpu, per_traj):
    from toppra_amd import constraint
    d = 7
    chain, sc, obj = _case7()
    data, args = rs.problem(d)
    peak = _peak(chain, args)
    hi = 1.5 * peak[:3] * (1.0 + np.random.default_rng(9).random((cc.B, 3) if per_traj else 3))
    force, moment = np.stack([-1.25 * hi, hi], -1), 2.0 * peak[3:].max()
    g = np.concatenate((force[..., 1], -force[..., 0], np.broadcast_to(moment, force.shape[:-2] + (6,))), -1)
    DT = constraint.DiscretizationType.Interpolation
    ours = constraint.BatchToolWrenchConstraint(sc, obj, force=force, moment=moment)
    assert np.array_equal(ours.F, F_BOTH) and np.array_equal(ours.g, g)
    _compare("spline", data, args, ours, F_BOTH, g, DT)


def _fixture_payload(fx):
    return {k: fx["payload_" + k] for k in ("mass", "com", "inertia", "rot", "origin")}


@pytest.mark.parametrize("name", FIXTURES)
def test_against_the_reference_s_fixtures(gpu, name):
    """w0 / wa / wb within the stored accuracy bound, return codes equal, sd within the stored end-to-end tolerance
    (tools/make_tool_wrench_golden.py)."""
    from toppra_amd import constraint
    fx = golden(name)
    chain, payload = rs.fixture_chain(fx), _fixture_payload(fx)
    sc, obj = chain_ref.serial_chain(chain), twr.payload_of(payload, chain)
    q, qs, qss = sor.path_samples(fx["coef"], fx["breaks"], fx["grid"])
    ev = tw.evaluations(q, qs, qss)
    got = dict(zip(NAMES, sc.tool_wrench_terms(q, qs, qss, obj)))
    rs.fixture_accuracy(name, fx, got, {k: twr.tool_wrench(chain, payload, *ev[k], absolute=True) for k in NAMES})
    interp, DT = rs.fixture_scheme(fx)
    if "mu" in fx:
        con = constraint.BatchToolWrenchConstraint.surface_contact(sc, obj, float(fx["mu"]), tuple(fx["half_extents"]), discretization_scheme=DT)
        assert np.array_equal(con.F, fx["F"]) and np.array_equal(np.broadcast_to(con.g, fx["g"].shape), fx["g"])
    else:
        con = constraint.BatchToolWrenchConstraint(sc, obj, F=fx["F"], g=fx["g"], discretization_scheme=DT)
    rs.fixture_solve(name, fx, con, interp)


def test_beside_the_other_chain_constraints(gpu):
    """[torque on the arm that carries the object, tool acceleration, tool wrench, tool speed] in one list: 2 + 28 + 14 + 12 + 24 =
    80 rows per stage; every pass runs, the rows are finite, every trajectory is feasible."""
    from toppra_amd import algorithm, batch, constraint
    d = 7
    chain, sc, obj = _case7()
    loaded = sc.with_payload(obj)
    data, args = rs.problem(d, seed=8)
    pe = batch.path_eval_batch(*args[:3])
    taumax = np.abs(loaded.torque_terms(pe["q"], pe["qs"], pe["qss"])[0]).max() + 20.0
    acc = np.abs(sc.tool_acceleration_terms(pe["q"], pe["qs"], pe["qss"])[1][..., :3]).max()
    peak = _peak(chain, args)
    cons = [constraint.BatchJointTorqueConstraint(loaded, np.tile([-taumax, taumax], (d, 1)), np.zeros(d)),
            constraint.BatchCartesianAccelerationConstraint(sc, linear=2.0 * acc),
            constraint.BatchToolWrenchConstraint(sc, obj, force=1.5 * peak[:3].max(), moment=1.5 * peak[3:].max()),
            constraint.BatchCartesianVelocityNormConstraint(sc, 0.3)]
    inst = algorithm.BatchTOPPRA(*args, constraints=cons)
    out = rs.run_passes(inst)
    assert out["rows"][0].shape[-1] == 2 + 4 * d + 2 * d + 12 + 24 <= 122
    rs.passes_ran(out)
    # the wrench block is the last one, with the rows of that constraint alone
    alone = algorithm.BatchTOPPRA(*args, constraints=[cons[2]]).dense_rows()
    for k in range(3):
        assert np.array_equal(out["rows"][k][..., -24:], alone[k][..., -24:])


def test_entries_refuse_bad_arguments_before_any_launch(gpu):
    """TPR_E_BADARG for a NULL chain, payload or buffer, a negative or non-finite mass, any non-finite payload entry, a dof outside
    1..32, negative counts; TPR_E_UNSUPPORTED for more than 2^31 - 1 points -- each before anything is launched: the buffers handed
    over with the refused calls are a few doubles long."""
    import ctypes
    from toppra_amd import _capi
    lib = _capi.load()
    sc, obj = chain_ref.serial_chain(cc.case(3)[0]), twr.payload_of(tw.PAYLOAD, None)
    one = np.zeros(6)
    p = one.ctypes.data
    BADARG, UNSUPPORTED = -1, -3
    model, keep = sc.c_struct(one)
    m = ctypes.byref(model)

    def calls(body, chain=m, B=2, N=1):
        b = None if body is None else ctypes.byref(body)
        return (lib.tpr_chain_tool_wrench_batch(chain, b, B * (N + 1), p, p, p, p, 0, None),
                lib.tpr_chain_tool_wrench_terms_batch(chain, b, B, N, p, p, p, p, p, p, 0, None))

    assert calls(None) == (BADARG,) * 2 and b"payload" in lib.tpr_last_error()
    assert calls(obj.c_struct(sc), chain=None) == (BADARG,) * 2
    for bad in (-1.0, np.nan, np.inf):
        body = obj.c_struct(sc)
        body.mass = bad
        assert calls(body) == (BADARG,) * 2, bad
    for field, size in (("com", 3), ("inertia", 6), ("rot", 9), ("origin", 3)):
        for k in (0, size - 1):
            body = obj.c_struct(sc)
            getattr(body, field)[k] = np.nan
            assert calls(body) == (BADARG,) * 2 and b"finite" in lib.tpr_last_error(), (field, k)
    body = obj.c_struct(sc)
    bad_model, keep2 = sc.c_struct(one)
    bad_model.d = 33
    assert calls(body, chain=ctypes.byref(bad_model)) == (BADARG,) * 2
    assert calls(body, B=1 << 20, N=(1 << 11) - 1) == (UNSUPPORTED,) * 2  # 2^31 points
    b = ctypes.byref(body)
    assert lib.tpr_chain_tool_wrench_batch(m, b, -1, p, p, p, p, 0, None) == BADARG
    assert lib.tpr_chain_tool_wrench_terms_batch(m, b, -1, 1, p, p, p, p, p, p, 0, None) == BADARG
    assert lib.tpr_chain_tool_wrench_terms_batch(m, b, 1, -1, p, p, p, p, p, p, 0, None) == BADARG
    for k in range(4):  # q, qd, qdd, wrench
        a = [p] * 4
        a[k] = None
        assert lib.tpr_chain_tool_wrench_batch(m, b, 2, *a, 0, None) == BADARG, k
    for k in range(6):  # q, qs, qss, w0, wa, wb
        a = [p] * 6
        a[k] = None
        assert lib.tpr_chain_tool_wrench_terms_batch(m, b, 1, 1, *a, 0, None) == BADARG, k
    # ... and the valid call on the same model still runs
    assert np.isfinite(sc.tool_wrench(np.zeros(3), np.zeros(3), np.zeros(3), obj)).all()

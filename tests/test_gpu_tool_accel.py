"""The tool-acceleration kernels on the MI355X: the single and the fused entry against the numpy reference
(tests/tool_accel_ref.py) within the accuracy bound of tests/tool_accel_cases.py, the fused outputs against the single entry bit
for bit, the calling conventions, ``BatchCartesianAccelerationConstraint`` against the same limit fed through the batched
callback route, the reference's fixtures, and the constraint in one list with the torque and the tool-speed limit.

Accuracy (B = 5, N = 40; the bound is 16 x the float64 reference's own error against np.longdouble, per case and quantity;
profiles/tool_accel_accuracy.json holds the yardsticks, the bounds and the measured errors): measured on the MI355X the kernels
use at most 0.47 of a bound (wb and the single evaluation, at 7 dof; 0.38 for wa, at 3 dof), and at most 0.27 of the stored
bound on the reference's fixtures, whose sd they reproduce to 7.8e-16 / 3.8e-13 (tolerances 1.6e-10 / 8.0e-12)."""
import numpy as np
import pytest

from tests import chain_cases as cc, chain_ref, rigid_support as rs, second_order_ref as sor, tool_accel_cases as tc, tool_accel_ref as tar
from tests.helpers import golden

pytestmark = pytest.mark.gpu
FIXTURES = ("tool_accel_d6_N40", "tool_accel_d3_N30_colloc")
I3, Z3 = np.eye(3), np.zeros((3, 3))
F_LINEAR, F_BOTH = np.block([[I3, Z3], [-I3, Z3]]), np.block([[I3, Z3], [-I3, Z3], [Z3, I3], [Z3, -I3]])


@pytest.mark.parametrize("d", tc.DOFS)
def test_kernels_against_the_numpy_reference(gpu, d):
    """Both entries, from numpy arrays; each fused output equals the single evaluation on the same arguments in every bit."""
    chain, q, qs, qss = cc.case(d)
    sc = chain_ref.serial_chain(chain)
    wa, wb = sc.tool_acceleration_terms(q, qs, qss)
    acc = sc.tool_acceleration(q, qs, qss)
    assert wa.shape == wb.shape == acc.shape == (cc.B, cc.N + 1, 6)
    rs.check(tc, d, {"wa": wa, "wb": wb, "acc": acc})
    zero = np.zeros_like(q)
    assert np.array_equal(wa, sc.tool_acceleration(q, zero, qs)) and np.array_equal(wb, acc)
    assert np.all(wa[2] == 0.0)  # the trajectory that stands still
    w0 = sc.tool_acceleration(q, zero, zero)
    assert not w0.any() and not np.signbit(w0).any() and not np.signbit(wa[2]).any()
    # gravity is not part of it: the same chain under another gravity gives the same bits
    other = chain_ref.serial_chain(dict(chain, gravity=np.array([1.0, -2.0, 3.0])))
    assert np.array_equal(other.tool_acceleration(q, qs, qss), acc)


@pytest.mark.parametrize("d", tc.DOFS)
def test_device_tensors_and_views_give_the_host_call_s_bits(gpu, d):
    """torch tensors on the device, contiguous and as a non-contiguous view, a flattened shape, a single point."""
    torch, dev = rs.torch_device()
    chain, q, qs, qss = cc.case(d)
    sc = chain_ref.serial_chain(chain)
    host = sc.tool_acceleration_terms(q, qs, qss)
    tq, tqs, tqss = (torch.from_numpy(np.array(v)).to(dev) for v in (q, qs, qss))
    for got, want in zip(sc.tool_acceleration_terms(tq, tqs, tqss), host):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    wide = [torch.repeat_interleave(t, 2, dim=1) for t in (tq, tqs, tqss)]
    views = [w[:, ::2] for w in wide]
    assert not views[0].is_contiguous()
    assert np.array_equal(sc.tool_acceleration(*views).cpu().numpy(), host[1])
    for got, want in zip(sc.tool_acceleration_terms(*views), host):
        assert np.array_equal(got.cpu().numpy(), want)
    flat = sc.tool_acceleration(tq.reshape(-1, d), tqs.reshape(-1, d), tqss.reshape(-1, d))
    assert tuple(flat.shape) == (cc.B * (cc.N + 1), 6) and np.array_equal(flat.cpu().numpy(), host[1].reshape(-1, 6))
    assert np.array_equal(sc.tool_acceleration(q[1, 3], qs[1, 3], qss[1, 3]), host[1][1, 3])
    one = sc.tool_acceleration_terms(q[1, 3], qs[1, 3], qss[1, 3])
    assert np.array_equal(one[0], host[0][1, 3]) and np.array_equal(one[1], host[1][1, 3])


def _peak(chain, args):
    """max |wb| of the linear and of the angular part over the problem's gridpoints, from the CPU reference."""
    q, qs, qss = sor.path_samples(*args[:3])
    wb = np.abs(tar.tool_acceleration(chain, q, qs, qss))
    return wb[..., :3].max(), wb[..., 3:].max()


def _compare(source, data, args, ours, F, g, DT):
    """The constraint against BatchSecondOrderConstraint(chain.tool_acceleration, F, g): the dense rows and all five passes."""
    return rs.compare(source, data, args, ours, ours.chain.tool_acceleration, F, g, DT)


@pytest.mark.parametrize("scheme", ["Collocation", "Interpolation"])
@pytest.mark.parametrize("source", ["spline", "samples"])
@pytest.mark.parametrize("per_traj", [False, True])
def test_the_constraint_equals_the_callback_route(gpu, scheme, source, per_traj):
    from toppra_amd import constraint
    d = 7
    chain = cc.case(d)[0]
    sc = chain_ref.serial_chain(chain)
    data, args = rs.problem(d)
    # positive on both sides (standing still satisfies it) and a generous multiple of the largest |wb|
    hi = 2.0 * _peak(chain, args)[0] * (1.0 + np.random.default_rng(9).random((cc.B, 3) if per_traj else 3))
    linear = np.stack([-1.5 * hi, hi], -1)  # [3, 2] or [B, 3, 2]
    DT = getattr(constraint.DiscretizationType, scheme)
    ours = constraint.BatchCartesianAccelerationConstraint(sc, linear=linear, discretization_scheme=DT)
    out = _compare(source, data, args, ours, F_LINEAR, np.concatenate((linear[..., 1], -linear[..., 0]), -1), DT)
    assert out["rows"][0].shape[-1] == 2 + 4 * d + (12 if scheme == "Interpolation" else 6)


def test_linear_and_angular_limits_equal_the_callback_route(gpu):
    from toppra_amd import constraint
    d = 7
    chain = cc.case(d)[0]
    sc = chain_ref.serial_chain(chain)
    data, args = rs.problem(d)
    lin, ang = _peak(chain, args)
    DT = constraint.DiscretizationType.Interpolation
    ours = constraint.BatchCartesianAccelerationConstraint(sc, linear=2.0 * lin, angular=3.0 * ang)
    _compare("spline", data, args, ours, F_BOTH, np.array([2.0 * lin] * 6 + [3.0 * ang] * 6), DT)


def test_a_dense_F_equals_the_callback_route(gpu):
    """Five rows that mix the linear and the angular part: a tilted, one-sided polytope."""
    from toppra_amd import constraint
    d = 7
    chain = cc.case(d)[0]
    sc = chain_ref.serial_chain(chain)
    data, args = rs.problem(d)
    F = np.random.default_rng(11).uniform(-1.0, 1.0, (5, 6))
    g = 2.0 * (np.abs(F[:, :3]).sum(-1) * _peak(chain, args)[0] + np.abs(F[:, 3:]).sum(-1) * _peak(chain, args)[1])
    DT = constraint.DiscretizationType.Interpolation
    _compare("spline", data, args, constraint.BatchCartesianAccelerationConstraint(sc, F=F, g=g), F, g, DT)


@pytest.mark.parametrize("name", FIXTURES)
def test_against_the_reference_s_fixtures(gpu, name):
    """wa / wb within the stored accuracy bound, the constraint's rows within the allowance composed from it, low / high and
    return codes equal, sd within the stored end-to-end tolerance (tools/make_tool_accel_golden.py)."""
    from toppra_amd import constraint
    fx = golden(name)
    chain = rs.fixture_chain(fx)
    sc = chain_ref.serial_chain(chain)
    B, d = fx["coef"].shape[0], fx["coef"].shape[3]
    q, qs, qss = sor.path_samples(fx["coef"], fx["breaks"], fx["grid"])
    ev = tc.evaluations(q, qs, qss)
    mags = {k: tar.tool_acceleration(chain, *ev[k], absolute=True) for k in ("wa", "wb")}
    got = dict(zip(("wa", "wb"), sc.tool_acceleration_terms(q, qs, qss)))
    rs.fixture_accuracy(name, fx, got, mags)
    interp, DT = rs.fixture_scheme(fx)
    con = constraint.BatchCartesianAccelerationConstraint(sc, linear=fx["linear"], angular=fx.get("angular"), discretization_scheme=DT)
    assert np.array_equal(con.F, fx["F"]) and np.array_equal(con.g, fx["g"])
    rows = rs.fixture_solve(name, fx, con, interp)
    # The rows' allowance, composed as for the torque fixtures (tests/test_gpu_chain.py) through the rows' own assembly: w0 is an
    # exact zero on both sides and contributes nothing, so a = F wa may be off by |F| (bound_wa mag_wa), b = F wb alike, and
    # under Interpolation the second half a_{i+1} + 2 delta_i b_{i+1}, b_{i+1} by the same sums of its parts; c = F 0 - g = -g
    # has no allowance from the kernels.  On top, 4 eps of the row with its VALUES in absolute value for the assembly's own
    # roundings: every row of F has a single non-zero entry, so its dot product rounds nothing.
    F, g = np.abs(fx["F"]), fx["g"]
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
        print("%s rows %s: largest error / allowance %.3g" % (name, k, worst))
        assert not bad.any(), (name, k, worst)


def test_beside_the_other_chain_constraints(gpu):
    """[torque, tool acceleration, tool speed] of one chain in one list: every pass runs, the dense rows hold the torque block
    and then the acceleration block, each with the rows of that constraint alone."""
    from toppra_amd import algorithm, batch, constraint
    d = 7
    chain = cc.case(d)[0]
    sc = chain_ref.serial_chain(chain)
    data, args = rs.problem(d, seed=8)
    pe = batch.path_eval_batch(*args[:3])
    taumax = np.abs(sc.torque_terms(pe["q"], pe["qs"], pe["qss"])[0]).max() + 20.0
    torque = lambda: constraint.BatchJointTorqueConstraint(sc, np.tile([-taumax, taumax], (d, 1)), np.zeros(d))  # noqa: E731
    accel = lambda: constraint.BatchCartesianAccelerationConstraint(sc, linear=2.0 * _peak(chain, args)[0])  # noqa: E731
    inst = algorithm.BatchTOPPRA(*args, constraints=[torque(), accel(), constraint.BatchCartesianVelocityNormConstraint(sc, 0.3)])
    out = rs.run_passes(inst)
    rs.passes_ran(out)
    first, nt, na = 2 + 4 * d, 2 * d, 12  # (x_next pair and acceleration block; torque: Collocation; tool acceleration: Interpolation)
    assert out["rows"][0].shape[-1] == first + nt + na
    alone_t = algorithm.BatchTOPPRA(*args, constraints=[torque()]).dense_rows()
    alone_a = algorithm.BatchTOPPRA(*args, constraints=[accel()]).dense_rows()
    for k in range(3):
        assert np.array_equal(out["rows"][k][..., first:first + nt], alone_t[k][..., first:])
        assert np.array_equal(out["rows"][k][..., first + nt:], alone_a[k][..., first:])
    # the tool-speed limit went into the boxes: those of the list that holds it alone
    low, high = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchCartesianVelocityNormConstraint(sc, 0.3)]).stage_boxes()
    assert np.array_equal(out["rows"][3], low) and np.array_equal(out["rows"][4], high)


def test_entries_refuse_bad_arguments_before_any_launch(gpu):
    """TPR_E_BADARG for a NULL array, a dof outside 1..32, an unknown joint type, a joint_type array on the device, a NULL
    buffer, negative counts; TPR_E_UNSUPPORTED for more than 2^31 - 1 points -- each before anything is launched: the buffers
    handed over with the refused calls are a few doubles long."""
    import ctypes
    from toppra_amd import _capi
    lib = _capi.load()
    sc = chain_ref.serial_chain(cc.case(3)[0])
    one = np.zeros(6)
    p = one.ctypes.data
    BADARG, UNSUPPORTED = -1, -3

    def calls(model, B=2, N=1):
        m = ctypes.byref(model)
        return (lib.tpr_chain_tool_acceleration_batch(m, B * (N + 1), p, p, p, p, 0, None),
                lib.tpr_chain_tool_acceleration_terms_batch(m, B, N, p, p, p, p, p, 0, None))

    def model(**kw):
        m, keep = sc.c_struct(one)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    assert calls(model(d=0)) == (BADARG,) * 2 and calls(model(d=33)) == (BADARG,) * 2
    for field in ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity", "tool"):
        assert calls(model(**{field: None})) == (BADARG,) * 2, field
    codes = np.array([0, 2, 1], dtype=np.int32)
    assert calls(model(joint_type=codes.ctypes.data)) == (BADARG,) * 2
    assert b"joint type" in lib.tpr_last_error()
    torch, dev = rs.torch_device()
    on_device = torch.zeros(3, dtype=torch.int32, device=dev)
    assert calls(model(joint_type=on_device.data_ptr())) == (BADARG,) * 2
    assert b"host array" in lib.tpr_last_error()
    assert calls(model(), B=1 << 20, N=(1 << 11) - 1) == (UNSUPPORTED,) * 2  # 2^31 points
    m = ctypes.byref(model())
    assert lib.tpr_chain_tool_acceleration_batch(m, -1, p, p, p, p, 0, None) == BADARG
    assert lib.tpr_chain_tool_acceleration_terms_batch(m, -1, 1, p, p, p, p, p, 0, None) == BADARG
    assert lib.tpr_chain_tool_acceleration_terms_batch(m, 1, -1, p, p, p, p, p, 0, None) == BADARG
    assert lib.tpr_chain_tool_acceleration_batch(None, 2, p, p, p, p, 0, None) == BADARG
    assert lib.tpr_chain_tool_acceleration_terms_batch(None, 1, 1, p, p, p, p, p, 0, None) == BADARG
    for k in range(4):  # q, qd, qdd, acc
        a = [p] * 4
        a[k] = None
        assert lib.tpr_chain_tool_acceleration_batch(m, 2, *a, 0, None) == BADARG, k
    for k in range(5):  # q, qs, qss, wa, wb
        a = [p] * 5
        a[k] = None
        assert lib.tpr_chain_tool_acceleration_terms_batch(m, 1, 1, *a, 0, None) == BADARG, k
    # ... and the valid call on the same model still runs
    assert np.isfinite(sc.tool_acceleration(np.zeros(3), np.zeros(3), np.zeros(3))).all()

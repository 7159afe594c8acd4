"""The chain kernels on the MI355X: inverse dynamics, the fused torque terms and the tool velocity against the numpy reference
(tests/chain_ref.py) within the measured accuracy bound of tests/chain_cases.py, the fused kernel against the single one bit
for bit, a SerialChain inside the torque constraints against the same chain as a callback, the reference's fixtures, and
the tool-speed constraint through the stage boxes.

Measured on the MI355X (B = 5, N = 40; error / bound, the bound being 16 x the float64 reference's own error against
np.longdouble): at most 0.43 over w0 / wa / wb (32 dof), 0.66 over the tool velocity (32 dof, S = None)."""
import numpy as np
import pytest

from tests import chain_cases as cc, chain_ref, rigid_support as rs, second_order_ref as sor
from tests.helpers import golden

pytestmark = pytest.mark.gpu
FIXTURES = ("chain_torque_d6_N40", "chain_torque_d3_N30_interp")
PASSES = ("compute_parameterization", "compute_parameterization_sd", "compute_feasible_sets", "compute_controllable_sets",
          "compute_reachable_sets")


@pytest.mark.parametrize("d", cc.DOFS)
def test_kernels_against_the_numpy_reference(gpu, d):
    """All three entries, from numpy arrays; each fused output equals the single evaluation on the same arguments."""
    chain, q, qs, qss = cc.case(d)
    sc = chain_ref.serial_chain(chain)
    fused = sc.torque_terms(q, qs, qss)
    rs.check(cc, d, dict(zip(("w0", "wa", "wb"), fused)))
    for got, args in zip(fused, cc.evaluations(q, qs, qss).values()):
        assert np.array_equal(got, sc.inverse_dynamics(*args))
    rs.check(cc, d, {"vsv": sc.tool_velocity_norm(q, qs), "vsv_S": sc.tool_velocity_norm(q, qs, cc.S_FULL)})
    assert np.all(sc.tool_velocity_norm(q, qs)[2] == 0.0)  # the trajectory that stands still


@pytest.mark.parametrize("d", cc.DOFS)
def test_device_tensors_and_views_give_the_host_call_s_bits(gpu, d):
    """torch tensors on the device, contiguous and as a non-contiguous view, any leading shape: the values of the numpy call."""
    torch, dev = rs.torch_device()
    chain, q, qs, qss = cc.case(d)
    sc = chain_ref.serial_chain(chain)
    host = sc.torque_terms(q, qs, qss)
    tq, tqs, tqss = (torch.from_numpy(np.array(v)).to(dev) for v in (q, qs, qss))
    for got, want in zip(sc.torque_terms(tq, tqs, tqss), host):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    # every second gridpoint of a twice as long run: strided views
    wide = [torch.repeat_interleave(t, 2, dim=1) for t in (tq, tqs, tqss)]
    views = [w[:, ::2] for w in wide]
    assert not views[0].is_contiguous()
    assert np.array_equal(sc.inverse_dynamics(*views).cpu().numpy(), host[2])
    assert np.array_equal(sc.inverse_dynamics(tq.reshape(-1, d), tqs.reshape(-1, d), tqss.reshape(-1, d)).cpu().numpy(),
                          host[2].reshape(-1, d))
    assert np.array_equal(sc.inverse_dynamics(q[1, 3], qs[1, 3], qss[1, 3]), host[2][1, 3])
    assert np.array_equal(sc.tool_velocity_norm(views[0], views[1]).cpu().numpy(), sc.tool_velocity_norm(q, qs))
    S = torch.from_numpy(cc.S_FULL).to(dev)
    assert np.array_equal(sc.tool_velocity_norm(tq, tqs, S).cpu().numpy(), sc.tool_velocity_norm(q, qs, cc.S_FULL))


@pytest.mark.parametrize("scheme", ["Collocation", "Interpolation"])
@pytest.mark.parametrize("source", ["spline", "samples"])
@pytest.mark.parametrize("per_traj", [False, True])
def test_a_chain_in_the_torque_constraint_equals_its_callback(gpu, scheme, source, per_traj):
    """BatchJointTorqueConstraint(chain, ...) against inv_dyn=chain.inverse_dynamics: the dense rows and every pass are equal."""
    from toppra_amd import algorithm, constraint
    d = 7
    chain, q, _, _ = cc.case(d)
    sc = chain_ref.serial_chain(chain)
    data, args = rs.problem(d)
    hold = np.abs(cc.reference(d)["w0"]).max() + 5.0
    rng = np.random.default_rng(9)
    taumax = hold * (1.0 + rng.random((cc.B, d) if per_traj else d))
    taulim, fric = np.stack([-taumax, taumax], -1), 0.05 * rng.random(d)
    DT = getattr(constraint.DiscretizationType, scheme)
    results = []
    for inv_dyn in (sc, sc.inverse_dynamics):
        cons = [constraint.BatchJointTorqueConstraint(inv_dyn, taulim, fric, discretization_scheme=DT)]
        results.append(rs.run_passes(rs.instance(source, data, args, cons)))
    rs.same(results[0], results[1], "chain vs callback")
    assert np.isfinite(results[0]["rows"][0]).all()
    if source == "spline":  # the second-order spelling of the same constraint takes a chain as well, and builds the same rows
        so = constraint.BatchSecondOrderConstraint.joint_torque_constraint(sc, taulim, fric, discretization_scheme=DT)
        rs.same(algorithm.BatchTOPPRA(*args, constraints=[so]).dense_rows(), results[0]["rows"], "second-order spelling")


@pytest.mark.parametrize("name", FIXTURES)
def test_against_the_reference_s_fixtures(gpu, name):
    """w0 / wa / wb and the torque rows within the stored accuracy bound, return codes equal, sd within the stored end-to-end
    tolerance (measured on the CPU: tools/make_chain_golden.py)."""
    from toppra_amd import constraint
    fx = golden(name)
    chain = rs.fixture_chain(fx)
    sc = chain_ref.serial_chain(chain)
    B, d = fx["coef"].shape[0], fx["coef"].shape[3]
    q, qs, qss = sor.path_samples(fx["coef"], fx["breaks"], fx["grid"])
    mags = {k: chain_ref.rnea(chain, *args, absolute=True) for k, args in cc.evaluations(q, qs, qss).items()}
    got = dict(zip(("w0", "wa", "wb"), sc.torque_terms(q, qs, qss)))
    rs.fixture_accuracy(name, fx, got, mags)
    interp, DT = rs.fixture_scheme(fx, "torque_scheme")
    rows = rs.fixture_solve(name, fx, constraint.BatchJointTorqueConstraint(sc, fx["taulim"], fx["fric"], discretization_scheme=DT), interp)
    # The rows' allowance, composed from the per-quantity bounds through the rows' own assembly: a = wa - w0 may be off by
    # bound_wa mag_wa + bound_w0 mag_w0, b = wb - w0 alike, c = w0 + friction sign(q') - g by bound_w0 mag_w0, and under
    # Interpolation the second half a_{i+1} + 2 delta_i b_{i+1}, b_{i+1}, c_{i+1} by the same sums of its parts.  On top, the
    # assembly itself rounds at most three times per entry on either side (a difference, a product, a sum), each by half an ulp
    # of a partial result no larger than the row with its VALUES in absolute value: 4 eps of that.
    g = np.concatenate((fx["taulim"][..., 1], -fx["taulim"][..., 0]), -1)
    deltas = np.broadcast_to(np.diff(fx["grid"]), (B, len(fx["grid"]) - 1))
    zero_g, eps = np.zeros_like(g), np.finfo(np.float64).eps
    bw = {k: fx["acc_bound"][i] * mags[k] for i, k in enumerate(("w0", "wa", "wb"))}
    allow = [np.abs(r) for r in sor.block_rows(-bw["w0"], bw["wa"], bw["wb"], np.abs(qs), deltas, None, zero_g, None, interp)[:2]]
    allow.append(np.abs(sor.block_rows(bw["w0"], bw["w0"], bw["w0"], np.abs(qs), deltas, None, zero_g, None, interp)[2]))
    size = [np.abs(r) for r in sor.block_rows(-np.abs(fx["w0"]), np.abs(fx["wa"]), np.abs(fx["wb"]), np.abs(qs), deltas, None, zero_g, None, interp)[:2]]
    size_c = np.abs(sor.block_rows(np.abs(fx["w0"]), np.abs(fx["w0"]), np.abs(fx["w0"]), np.abs(qs), deltas, None, zero_g, np.abs(fx["fric"]), interp)[2])
    tiled = np.tile(np.abs(g), 2 if interp else 1)
    size.append(size_c + (tiled[:, None, :] if g.ndim == 2 else tiled))
    for k, stored, al, sz in zip("abc", (fx["rows_a"], fx["rows_b"], fx["rows_c"]), allow, size):
        block = rows["abc".index(k)][:, :, 2 + 4 * d:]
        tol = al + 4 * eps * sz
        worst = float(np.max(np.abs(block - stored) / tol))
        print("%s rows %s: largest error / allowance %.3g" % (name, k, worst))
        assert worst <= 1.0, (name, k, worst)


@pytest.mark.parametrize("S", [None, "full"])
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_tool_speed_constraint(gpu, S, kind):
    from toppra_amd import algorithm, batch, constraint
    d = 7
    chain, _, _, _ = cc.case(d)
    sc = chain_ref.serial_chain(chain)
    data, args = rs.problem(d, seed=6)
    S = None if S is None else cc.S_FULL
    limit = np.array([0.05, 0.1, 0.2, 0.4, 0.8])
    if kind == "torch":
        torch, dev = rs.torch_device()
        args = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in args)
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else v  # noqa: E731
    pe = batch.path_eval_batch(*args[:3])
    q, qs = pe["q"], pe["qs"]
    # vSv against the reference within the accuracy bound measured on these inputs
    vsv, xbound = batch.chain_tool_bound_batch(sc, q, qs, limit if kind == "numpy" else torch.from_numpy(limit).to(dev),
                                               S if S is None or kind == "numpy" else torch.from_numpy(S).to(dev))
    qh, qsh = host(q), host(qs)
    ref, mag = chain_ref.tool_vsv(chain, qh, qsh, S), chain_ref.tool_vsv(chain, qh, qsh, S, absolute=True)
    bound = cc.BOUND_FACTOR * cc._own_error(ref, chain_ref.tool_vsv(chain, qh, qsh, S, dtype=np.longdouble), mag)
    err = cc.metric(host(vsv), ref, mag)
    print("tool speed, S %s: error %.3g, bound %.3g" % ("given" if S is not None else "None", err, bound))
    assert err <= bound
    assert np.array_equal(host(xbound)[..., 0], np.zeros_like(ref)) and np.array_equal(host(xbound)[..., 1], limit[:, None] / host(vsv))
    if S is not None:  # the angular part takes part: another value than the linear speed's
        assert not np.allclose(host(vsv), host(batch.chain_tool_bound_batch(sc, q, qs)))
    # the constraint's boxes are those of a BatchBoundConstraint fed with the kernel's own bound, bit for bit
    con = constraint.BatchCartesianVelocityNormConstraint(sc, limit, S)
    inst = algorithm.BatchTOPPRA(*args, constraints=[con])
    other = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchBoundConstraint(xbound=xbound)])
    for a, b in zip(inst.stage_boxes(), other.stage_boxes()):
        assert np.array_equal(host(a), host(b))
    low, high = (host(v) for v in inst.stage_boxes())
    assert (high[..., 1] < sor.velocity_box(qsh, data["vlim"])[1][..., 1]).any(), "the tool-speed limit tightens no box"
    # The parameterization respects the limit at every gridpoint: x <= fl(limit / vSv) with the kernel's vSv, whose error
    # against the reference is at most bound x magnitude; the division, the square root, its square and the product round
    # once each (4 eps).
    out = inst.compute_parameterization()
    assert np.all(host(out["status"]) == 0)
    sd = host(out["sd"])
    # (the issue's vSv sd^2 <= limit (1 + bound) with the bound in the metric's terms: an error of bound x magnitude is a
    # relative error of bound x magnitude / value; it must stay of rounding size, or this check would mean nothing)
    slack = bound * mag / ref + 4 * np.finfo(np.float64).eps
    assert slack.max() < 1e-9, slack.max()
    assert np.all(ref * sd ** 2 <= limit[:, None] * (1.0 + slack))
    free = host(algorithm.BatchTOPPRA(*args).compute_parameterization()["sd"])
    assert (sd < free).any() and np.all(sd <= free * (1 + 1e-9)), "the limit changes no parameterization"


def test_a_standstill_stage_leaves_the_box(gpu):
    """q' = 0 at a gridpoint: vSv = 0, the bound is +inf and the stage keeps the 1e8 of the box."""
    from toppra_amd import algorithm, constraint
    d = 3
    chain, q, qs, qss = cc.case(d)
    sc = chain_ref.serial_chain(chain)
    qs = np.array(qs)
    qs[:, 7] = 0.0
    grid = np.linspace(0.0, 1.0, cc.N + 1)
    inst = algorithm.BatchTOPPRA.from_path_samples(grid, q, qs, qss, None, np.tile([-50.0, 50.0], (cc.B, d, 1)),
                                                   constraints=[constraint.BatchCartesianVelocityNormConstraint(sc, 0.25)])
    low, high = inst.stage_boxes()
    assert np.all(high[:, 7, 1] == 1e8) and np.all(high[2, :, 1] == 1e8)  # the stage; the trajectory that stands still
    assert np.all(high[[0, 1, 3, 4], 8, 1] < 1e8) and np.all(low[..., 1] == 0.0)


def test_chained_with_the_other_constraints(gpu):
    """List order [vlim, varying velocity limits, tool speed, bound, torque]: the boxes of the same list with the tool speed given
    as its bound, through the dense pass."""
    from toppra_amd import algorithm, batch, constraint
    d = 7
    chain, _, _, _ = cc.case(d)
    sc = chain_ref.serial_chain(chain)
    data, args = rs.problem(d, seed=8)
    pe = batch.path_eval_batch(*args[:3])
    _, xbound = batch.chain_tool_bound_batch(sc, pe["q"], pe["qs"], 0.3)
    vgrid = np.broadcast_to(2.0 * data["vlim"][:, None], (cc.B, cc.N + 1, d, 2)).copy()
    ub = np.tile([-40.0, 40.0], (cc.N + 1, 1))
    taumax = np.abs(sc.torque_terms(pe["q"], pe["qs"], pe["qss"])[0]).max() + 20.0
    torque = lambda: constraint.BatchJointTorqueConstraint(sc, np.tile([-taumax, taumax], (d, 1)), np.zeros(d))  # noqa: E731
    a = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchJointVelocityConstraintVarying(vgrid),
                                                  constraint.BatchCartesianVelocityNormConstraint(sc, 0.3),
                                                  constraint.BatchBoundConstraint(ubound=ub), torque()])
    b = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchJointVelocityConstraintVarying(vgrid),
                                                  constraint.BatchBoundConstraint(xbound=xbound),
                                                  constraint.BatchBoundConstraint(ubound=ub), torque()])
    rs.same(a.dense_rows(), b.dense_rows(), "rows")
    rs.same(a.compute_parameterization(), b.compute_parameterization(), "parameterization")
    assert np.all(a.compute_parameterization()["status"] == 0)


def test_fail_first_surface():
    """What the parent commit lacks: the module, the constraint taking a chain, the exports.  (No GPU work.)"""
    import toppra_amd
    from toppra_amd import _capi, chain, constraint
    assert toppra_amd.SerialChain is chain.SerialChain
    sc = chain_ref.serial_chain(cc.case(3)[0])
    con = constraint.BatchJointTorqueConstraint(sc, np.tile([-1.0, 1.0], (3, 1)), np.zeros(3))
    con.check(2, 10, 3)
    assert hasattr(constraint, "BatchCartesianVelocityNormConstraint")
    lib = _capi.load()
    for name in ("tpr_chain_bytes", "tpr_chain_inverse_dynamics_batch", "tpr_chain_torque_terms_batch", "tpr_chain_tool_velocity_batch"):
        assert name in _capi.EXPORTS and hasattr(lib, name)


def test_entries_refuse_bad_arguments_before_any_launch(gpu):
    """TPR_E_BADARG for a NULL array, a dof outside 1..32, an unknown joint type, a joint_type array on the device, a NULL
    buffer; TPR_E_UNSUPPORTED for more than 2^31 - 1 points -- each before anything is launched: the buffers handed over
    with the refused calls are one double long."""
    import ctypes
    from toppra_amd import _capi
    lib = _capi.load()
    sc = chain_ref.serial_chain(cc.case(3)[0])
    one = np.zeros(3)
    p = one.ctypes.data
    BADARG, UNSUPPORTED = -1, -3

    def calls(model, B=2, N=1):
        m = ctypes.byref(model)
        return (lib.tpr_chain_inverse_dynamics_batch(m, B * (N + 1), p, p, p, p, 0, None),
                lib.tpr_chain_torque_terms_batch(m, B, N, p, p, p, p, p, p, 0, None),
                lib.tpr_chain_tool_velocity_batch(m, B, N, p, p, None, None, p, None, 0, None))

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
    assert b"joint type" in lib.tpr_last_error()
    torch, dev = rs.torch_device()
    on_device = torch.zeros(3, dtype=torch.int32, device=dev)
    assert calls(model(joint_type=on_device.data_ptr())) == (BADARG,) * 3
    assert b"host array" in lib.tpr_last_error()
    assert calls(model(), B=1 << 20, N=(1 << 11) - 1) == (UNSUPPORTED,) * 3  # 2^31 points
    m = ctypes.byref(model())
    assert lib.tpr_chain_inverse_dynamics_batch(m, 2, p, None, p, p, 0, None) == BADARG
    assert lib.tpr_chain_torque_terms_batch(m, 1, 1, p, p, p, p, None, p, 0, None) == BADARG
    assert lib.tpr_chain_tool_velocity_batch(m, 1, 1, p, p, None, None, None, None, 0, None) == BADARG  # neither vSv nor xbound
    assert lib.tpr_chain_tool_velocity_batch(m, 1, 1, p, p, None, None, p, p, 0, None) == BADARG     # xbound without limit
    # ... and the valid call on the same model still runs
    assert np.isfinite(sc.inverse_dynamics(one, one, one)).all()

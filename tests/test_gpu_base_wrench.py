"""The base-reaction kernels on the MI355X: the single and the fused entry against the numpy reference (tests/base_wrench_ref.py)
within the accuracy bound of tests/base_wrench_cases.py on every chain dof and every tree shape, the fused outputs against the
single entry bit for bit, the exact zeros, a chain against the tree of its links, a forest against the sum of its chains, the
joint-0 identity against the tree kernels' inverse dynamics, the calling conventions, ``BatchBaseWrenchConstraint`` against the same
limit fed through the batched callback route, the constraint beside a torque limit on the same robot, the reference's fixtures,
and the C entries' refusals.

Accuracy (the bound is 16 x the float64 reference's own error against np.longdouble, per case and quantity;
profiles/base_wrench_accuracy.json holds the yardsticks, the bounds and the measured errors): measured on the MI355X the kernels
use at most 0.35 of a bound over the 16 cases, and at most 0.10 of the stored bound on the reference's fixtures, whose sd they
reproduce to 3.1e-15 / 1.9e-13 (tolerances 1.3e-9 / 4.8e-12)."""
import ctypes

import numpy as np
import pytest

from tests import base_wrench_cases as bw, base_wrench_ref as bwr, chain_cases as cc, chain_ref, second_order_ref as sor
from tests import rigid_support as rs, tree_cases as tc, tree_ref
from tests.helpers import golden

pytestmark = pytest.mark.gpu
FIXTURES = ("base_wrench_torso_d15_N30", "base_wrench_d4_N30_colloc")
NAMES = ("w0", "wa", "wb")
I3, Z3 = np.eye(3), np.zeros((3, 3))
F_BOTH = np.block([[I3, Z3], [-I3, Z3], [Z3, I3], [Z3, -I3]])
GRAVITY = np.array([0.0, 0.0, -9.81])
BADARG, UNSUPPORTED = -1, -3


@pytest.mark.parametrize("key", bw.CASES)
def test_kernels_against_the_numpy_reference(gpu, key):
    """(1) - (3) Both entries, from numpy arrays; each fused output equals the single evaluation on the same arguments in every
    bit; no negative zero; without gravity w0 is +0 (the platform's weight is its mass times that zero); the trajectory that
    stands still has wa == w0."""
    robot, q, qs, qss = bw.case(key)
    model, mount = bwr.robot_of(robot), bwr.mount_of(bw.MOUNT)
    w0, wa, wb = model.base_wrench_terms(q, qs, qss, mount)
    single = model.base_wrench(q, qs, qss, mount)
    assert w0.shape == wa.shape == wb.shape == single.shape == q.shape[:2] + (6,)
    rs.check(bw, key, {"w0": w0, "wa": wa, "wb": wb, "wrench": single}, label="%s")
    zero = np.zeros_like(q)
    assert np.array_equal(w0, model.base_wrench(q, zero, zero, mount)) and np.array_equal(wa, model.base_wrench(q, zero, qs, mount))
    assert np.array_equal(wb, single)
    for v in (w0, wa, wb):  # a zero leaves as +0, so equal values are equal bits
        assert not np.signbit(v[v == 0]).any()
    assert np.array_equal(wa[bw.still(key)], w0[bw.still(key)])
    if not robot["gravity"].any():
        assert not w0.any() and not np.signbit(w0).any()  # (the platform's weight is its mass times a zero gravity)
    else:
        assert np.all(np.abs(w0[..., :3]).max(-1) > 0)


@pytest.mark.parametrize("key", (2, 9, "skip", "roots"))
def test_without_gravity_and_platform_w0_is_a_positive_zero(gpu, key):
    robot, q, qs, qss = bw.case(key)
    robot = dict(robot, gravity=np.zeros(3))
    model = bwr.robot_of(robot)
    for mount in (None, bwr.mount_of(dict(bw.MOUNT, mass=0.0))):
        w0, wa, wb = model.base_wrench_terms(q, qs, qss, mount)
        assert not w0.any() and not np.signbit(w0).any()
        assert wa.any() and wb.any()
        assert not wa[bw.still(key)].any() and not np.signbit(wa[bw.still(key)]).any()


@pytest.mark.parametrize("d", bw.DOFS)
def test_a_chain_and_the_tree_of_its_links_are_bit_equal(gpu, d):
    """(4) SerialChain and KinematicTree.from_chain(chain): one kernel, one parent table."""
    from toppra_amd.chain import KinematicTree
    chain, q, qs, qss = bw.case(d)
    sc, mount = chain_ref.serial_chain(chain), bwr.mount_of(bw.MOUNT)
    tree = KinematicTree.from_chain(sc)
    for a, b in zip(sc.base_wrench_terms(q, qs, qss, mount), tree.base_wrench_terms(q, qs, qss, mount)):
        assert np.array_equal(a, b)
    assert np.array_equal(sc.base_wrench(q, qs, qss), tree.base_wrench(q, qs, qss))


def test_the_forest_is_the_sum_of_its_chains(gpu):
    """(4) "roots": two 9-link chains on one base.  The platform is counted once."""
    robot, q, qs, qss = bw.case("roots")
    halves = []
    for part, mount in ((slice(0, 9), bw.MOUNT), (slice(9, 18), dict(bw.MOUNT, mass=0.0))):
        chain = {k: (np.asarray(v)[part] if k in ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia") else v)
                 for k, v in robot.items() if k != "parent"}
        chain["tool"] = np.zeros(3)
        halves.append(chain_ref.serial_chain(chain).base_wrench_terms(q[..., part], qs[..., part], qss[..., part], bwr.mount_of(mount)))
    whole = bwr.robot_of(robot).base_wrench_terms(q, qs, qss, bwr.mount_of(bw.MOUNT))
    ref = bw.reference("roots")
    for name, got, a, b in zip(NAMES, whole, *halves):
        err, bound = bw.metric(a + b, np.asarray(got), ref[name + "_mag"]), bw.bound("roots", name)
        print("roots %s: sum of the chains vs the forest %.3g, bound %.3g" % (name, err, bound))
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("key", ("vee", "nested", "torso", "y18", "comb32"))
def test_joint_0_identity_against_the_tree_kernels(gpu, key):
    """(5) With the mount at joint 0's origin the reaction about (along) joint 0's axis is joint 0's torque (force), both from the
    GPU.  The allowance is the sum of the two quantities' bounds, each on its own all-absolute magnitude."""
    from toppra_amd.chain import Mount
    robot, q, qs, qss = bw.case(key)
    model = bwr.robot_of(robot)
    at0 = {"rot": np.eye(3), "origin": robot["trans"][0], "mass": 0.0, "com": np.zeros(3)}
    axis = robot["rot"][0] @ robot["axis"][0]
    part = slice(0, 3) if int(robot["joint_type"][0]) == 1 else slice(3, 6)
    w = model.base_wrench(q, qs, qss, Mount(origin=robot["trans"][0]))
    tau = model.inverse_dynamics(q, qs, qss)[..., 0]
    mag = bwr.base_wrench(robot, q, qs, qss, at0, absolute=True)
    ref = bwr.base_wrench(robot, q, qs, qss, at0)
    b_w = bw.BOUND_FACTOR * cc._own_error(ref, bwr.base_wrench(robot, q, qs, qss, at0, dtype=np.longdouble), mag)
    allow = b_w * (mag[..., part] @ np.abs(axis)) + tc.bound(key, "wb") * tc.reference(key)["wb_mag"][..., 0]
    off = np.abs(w[..., part] @ axis - tau)
    print("%s: |axis . w - tau_0| at most %.3g of its allowance" % (key, float(np.max(off / allow))))
    assert np.all(off <= allow)


@pytest.mark.parametrize("key", (1, 7, 32, "nested", "comb32"))
def test_device_tensors_and_views_give_the_host_call_s_bits(gpu, key):
    """(6) torch tensors on the device, contiguous and as a non-contiguous view, a flattened shape, a single point."""
    torch, dev = rs.torch_device()
    robot, q, qs, qss = bw.case(key)
    d = q.shape[-1]
    model, mount = bwr.robot_of(robot), bwr.mount_of(bw.MOUNT)
    host = model.base_wrench_terms(q, qs, qss, mount)
    tq, tqs, tqss = (torch.from_numpy(np.array(v)).to(dev) for v in (q, qs, qss))
    for got, want in zip(model.base_wrench_terms(tq, tqs, tqss, mount), host):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    wide = [torch.repeat_interleave(t, 2, dim=1) for t in (tq, tqs, tqss)]
    views = [w[:, ::2] for w in wide]
    assert not views[0].is_contiguous()
    assert np.array_equal(model.base_wrench(*views, mount).cpu().numpy(), host[2])
    for got, want in zip(model.base_wrench_terms(*views, mount), host):
        assert np.array_equal(got.cpu().numpy(), want)
    flat = model.base_wrench(tq.reshape(-1, d), tqs.reshape(-1, d), tqss.reshape(-1, d), mount)
    assert tuple(flat.shape) == (q.shape[0] * q.shape[1], 6) and np.array_equal(flat.cpu().numpy(), host[2].reshape(-1, 6))
    assert np.array_equal(model.base_wrench(q[1, 3], qs[1, 3], qss[1, 3], mount), host[2][1, 3])
    one = model.base_wrench_terms(q[1, 3], qs[1, 3], qss[1, 3], mount)
    assert all(np.array_equal(one[k], host[k][1, 3]) for k in range(3))


# ---- the constraint ---------------------------------------------------------------------------------------------------------

def _robot(kind):
    """A robot dict under gravity along -z: the 7-dof chain, or the torso with two 7-dof arms."""
    base = cc.case(7)[0] if kind == "chain" else tc.case("torso")[0]
    return dict(base, gravity=GRAVITY)


def _peak(robot, mount, args):
    """Per component, the largest of |w0|, |wa|, |wb| over the problem's gridpoints, from the CPU reference: limits above it
    hold at rest (F w0 < g) with room, so every trajectory is feasible."""
    q, qs, qss = sor.path_samples(*args[:3])
    return np.max([np.abs(bwr.base_wrench(robot, *a, mount=mount)).max((0, 1)) for a in list(bw.evaluations(q, qs, qss).values())[:3]], 0)


def _compare(source, data, args, ours, F, g, DT):
    """The constraint against BatchSecondOrderConstraint(robot.base_wrench with the mount bound, F, g): rows and all five passes."""
    robot, mount = ours.robot, ours.mount
    return rs.compare(source, data, args, ours, lambda q, qd, qdd: robot.base_wrench(q, qd, qdd, mount), F, g, DT)


@pytest.mark.parametrize("scheme", ["Collocation", "Interpolation"])
@pytest.mark.parametrize("source", ["spline", "samples"])
@pytest.mark.parametrize("kind,per_traj", [("chain", False), ("tree", True)])
def test_the_constraint_equals_the_callback_route(gpu, scheme, source, kind, per_traj):
    """(7) Force and moment boxes with g from the CPU reference's peaks, shared or per trajectory."""
    from toppra_amd import constraint
    robot = _robot(kind)
    d = len(robot["mass"])
    model, mount = bwr.robot_of(robot), bwr.mount_of(bw.MOUNT)
    data, args = rs.problem(d)
    peak = _peak(robot, bw.MOUNT, args)
    hi = 1.5 * peak[:3] * (1.0 + np.random.default_rng(9).random((cc.B, 3) if per_traj else 3))
    force, moment = np.stack([-1.25 * hi, hi], -1), 2.0 * peak[3:].max()
    g = np.concatenate((force[..., 1], -force[..., 0], np.broadcast_to(moment, force.shape[:-2] + (6,))), -1)
    DT = getattr(constraint.DiscretizationType, scheme)
    ours = constraint.BatchBaseWrenchConstraint(model, mount, force=force, moment=moment, discretization_scheme=DT)
    assert np.array_equal(ours.F, F_BOTH) and np.array_equal(ours.g, g)
    out = _compare(source, data, args, ours, F_BOTH, g, DT)
    assert out["rows"][0].shape[-1] == 2 + 4 * d + (24 if scheme == "Interpolation" else 12)


def _cart(robot, args):
    """A platform and a footprint, chosen on the CPU, under which standing still lies inside the contact cone with room: the
    platform is heavy and low, the footprint reaches beyond the robot's static moment."""
    from toppra_amd.constraint import BatchToolWrenchConstraint
    mount = {"rot": np.eye(3), "origin": np.array([0.0, 0.0, -0.5]), "mass": 40.0 * robot["mass"].sum(), "com": np.array([0.0, 0.0, -0.4])}
    q, _, _ = sor.path_samples(*args[:3])
    w0 = bwr.base_wrench(robot, q, np.zeros_like(q), np.zeros_like(q), mount)
    half = tuple(4.0 * np.abs(w0[..., [4, 3]] / w0[..., 2:3]).max((0, 1)) + 0.05)
    mu = 0.6
    F, g = BatchToolWrenchConstraint.surface_contact_rows(mu, half)
    slack = np.einsum("mk,bnk->bnm", F, w0)
    assert np.all(slack < 0) and np.all(w0[..., 2] > 0), "standing still must lie strictly inside the cone at every gridpoint"
    return mount, mu, half, F, g


@pytest.mark.parametrize("kind,source", [("chain", "samples"), ("tree", "spline")])
def test_the_contact_cone_equals_the_callback_route(gpu, kind, source):
    """(7) surface_contact on a cart: F w0 < 0 at every gridpoint is asserted on the CPU before anything launches."""
    from toppra_amd import constraint
    robot = _robot(kind)
    d = len(robot["mass"])
    data, args = rs.problem(d, seed=6)
    mount, mu, half, F, g = _cart(robot, args)
    DT = constraint.DiscretizationType.Interpolation
    ours = constraint.BatchBaseWrenchConstraint.surface_contact(bwr.robot_of(robot), mu, half, mount=bwr.mount_of(mount))
    assert np.array_equal(ours.F, F) and np.array_equal(ours.g, g)
    out = _compare(source, data, args, ours, F, g, DT)
    assert out["rows"][0].shape[-1] == 2 + 4 * d + 32 <= 122


def test_beside_a_torque_constraint_on_the_same_robot(gpu):
    """(8) [torque on the torso's 15 joints, base reaction box] under Interpolation: 2 + 60 + 30 + 24 = 116 rows per stage, within
    the 122; every pass runs, the rows are finite, every trajectory is feasible; the wrench block is the last one."""
    from toppra_amd import algorithm, batch, constraint
    robot = _robot("tree")
    d = len(robot["mass"])
    model, mount = bwr.robot_of(robot), bwr.mount_of(bw.MOUNT)
    data, args = rs.problem(d, seed=8)
    pe = batch.path_eval_batch(*args[:3])
    taumax = np.abs(model.torque_terms(pe["q"], pe["qs"], pe["qss"])[0]).max() + 20.0
    peak = _peak(robot, bw.MOUNT, args)
    cons = [constraint.BatchJointTorqueConstraint(model, np.tile([-taumax, taumax], (d, 1)), np.zeros(d)),
            constraint.BatchBaseWrenchConstraint(model, mount, force=1.5 * peak[:3].max(), moment=1.5 * peak[3:].max())]
    inst = algorithm.BatchTOPPRA(*args, constraints=cons)
    out = rs.run_passes(inst)
    assert out["rows"][0].shape[-1] == 2 + 4 * d + 2 * d + 24 == 116 <= 122
    rs.passes_ran(out)
    alone = algorithm.BatchTOPPRA(*args, constraints=[cons[1]]).dense_rows()
    for k in range(3):
        assert np.array_equal(out["rows"][k][..., -24:], alone[k][..., -24:])


@pytest.mark.parametrize("name", FIXTURES)
def test_against_the_reference_s_fixtures(gpu, name):
    """(9) w0 / wa / wb within the stored accuracy bound, return codes equal, sd within the stored end-to-end tolerance
    (tools/make_base_wrench_golden.py)."""
    from toppra_amd import constraint
    fx = golden(name)
    robot = rs.fixture_tree(fx)
    mount = {k: fx["mount_" + k] for k in ("rot", "origin", "mass", "com")}
    model, frame = tree_ref.kinematic_tree(robot), bwr.mount_of(mount)
    q, qs, qss = sor.path_samples(fx["coef"], fx["breaks"], fx["grid"])
    ev = bw.evaluations(q, qs, qss)
    got = dict(zip(NAMES, model.base_wrench_terms(q, qs, qss, frame)))
    rs.fixture_accuracy(name, fx, got, {k: bwr.base_wrench(robot, *ev[k], mount=mount, absolute=True) for k in NAMES})
    interp, DT = rs.fixture_scheme(fx)
    if "mu" in fx:
        con = constraint.BatchBaseWrenchConstraint.surface_contact(model, float(fx["mu"]), tuple(fx["half_extents"]), mount=frame,
                                                                   discretization_scheme=DT)
        assert np.array_equal(con.F, fx["F"]) and np.array_equal(np.broadcast_to(con.g, fx["g"].shape), fx["g"])
    else:
        con = constraint.BatchBaseWrenchConstraint(model, frame, F=fx["F"], g=fx["g"], discretization_scheme=DT)
    rs.fixture_solve(name, fx, con, interp)


# ---- the entries' refusals --------------------------------------------------------------------------------------------------

def test_entries_refuse_bad_arguments_before_any_launch(gpu):
    """(10) In their order -- the links as a chain, the parent table, the fork count, the mount, the pointers; the terms entry B / N
    first -- each before anything is launched: the buffers handed over with the refused calls are a few doubles long."""
    from toppra_amd import _capi
    from toppra_amd.chain import Mount
    lib = _capi.load()
    sc = chain_ref.serial_chain(cc.case(3)[0])
    buf = np.zeros(64)
    p = buf.ctypes.data
    model, keep = sc.c_struct(buf)
    m = ctypes.byref(model)
    table = np.array([-1, 0, 1], dtype=np.int32)
    good = Mount(origin=(0.1, 0.0, 0.0), mass=2.0).c_struct()

    def calls(chain=m, parent=table, mount=good, B=2, N=1, q=p, out=p):
        t = None if parent is None else parent.ctypes.data
        f = None if mount is None else ctypes.byref(mount)
        single = lib.tpr_tree_base_wrench_batch(chain, t, f, B * (N + 1), q, p, p, out, 0, None), lib.tpr_last_error()
        terms = lib.tpr_tree_base_wrench_terms_batch(chain, t, f, B, N, q, p, p, out, out, out, 0, None), lib.tpr_last_error()
        return single, terms

    def refused(result, code, text):
        for rc, msg in result:
            assert rc == code and text in msg, (rc, msg)

    def bad_mount(**change):
        frame = Mount(origin=(0.1, 0.0, 0.0), mass=2.0).c_struct()
        for field, (k, v) in change.items():
            if field == "mass":
                frame.mass = v
            else:
                getattr(frame, field)[k] = v
        return frame

    nan_mount = bad_mount(com=(1, np.nan))
    # the order: each call is bad in the named way AND in every way that is checked later
    refused(calls(chain=None, parent=None, mount=nan_mount, q=None), BADARG, b"null chain")
    wrong = np.array([-1, 0, 2], dtype=np.int32)
    refused(calls(parent=wrong, mount=nan_mount, q=None), BADARG, b"the parent of link 2 is 2, outside -1 .. 1")
    refused(calls(parent=None, mount=nan_mount, q=None), BADARG, b"null parent")
    sc11 = chain_ref.serial_chain(chain_ref.random_chain(11, 5))
    model11, keep11 = sc11.c_struct(buf)
    five = np.array([-1, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4], dtype=np.int32)
    refused(calls(chain=ctypes.byref(model11), parent=five, mount=nan_mount, q=None), UNSUPPORTED, b"the tree has 5 forks")
    refused(calls(mount=nan_mount, q=None), BADARG, b"every entry of the mount must be finite")
    refused(calls(q=None), BADARG, b"are required")
    refused(calls(out=None), BADARG, b"are required")
    # the mount's own refusals
    for field, size in (("rot", 9), ("origin", 3), ("com", 3)):
        for k in (0, size - 1):
            for bad in (np.nan, np.inf):
                refused(calls(mount=bad_mount(**{field: (k, bad)})), BADARG, b"finite")
    for bad in (np.nan, -np.inf):
        refused(calls(mount=bad_mount(mass=(0, bad))), BADARG, b"finite")
    refused(calls(mount=bad_mount(mass=(0, -1.0))), BADARG, b"the mount's mass must be >= 0")
    refused(calls(mount=bad_mount(rot=(0, 1.001))), BADARG, b"orthonormal")
    refused(calls(mount=bad_mount(rot=(8, -1.0))), BADARG, b"orthonormal")  # (a reflection)
    refused(calls(mount=bad_mount(rot=(1, 1e-9))), BADARG, b"orthonormal")
    # sizes
    assert lib.tpr_tree_base_wrench_terms_batch(None, None, None, -1, 1, p, p, p, p, p, p, 0, None) == BADARG and b"B >= 0" in lib.tpr_last_error()
    assert lib.tpr_tree_base_wrench_terms_batch(m, table.ctypes.data, None, 1, -1, p, p, p, p, p, p, 0, None) == BADARG
    assert lib.tpr_tree_base_wrench_batch(m, table.ctypes.data, None, -1, p, p, p, p, 0, None) == BADARG
    refused(calls(B=1 << 20, N=(1 << 11) - 1), UNSUPPORTED, b"2^31 - 1")
    bad_model, keep2 = sc.c_struct(buf)
    bad_model.d = 33
    refused(calls(chain=ctypes.byref(bad_model)), BADARG, b"dof must be in")
    # ... a null mount is the base frame, and the valid call on the same model still runs
    tree = tree_ref.kinematic_tree(dict(cc.case(3)[0], parent=table))
    z = np.zeros(3)
    assert np.array_equal(sc.base_wrench(z, z, z), tree.base_wrench(z, z, z, Mount())) and np.isfinite(sc.base_wrench(z, z, z)).all()
    w = np.zeros(6)
    assert lib.tpr_tree_base_wrench_batch(m, table.ctypes.data, None, 1, p, p, p, w.ctypes.data, 0, None) == 0
    assert np.array_equal(w, sc.base_wrench(z, z, z))


def test_python_refuses_shape_errors_before_any_launch(gpu):
    robot, q, qs, qss = bw.case("vee")
    model = bwr.robot_of(robot)
    with pytest.raises(ValueError, match="dof"):
        model.base_wrench(q[..., :2], qs[..., :2], qss[..., :2])
    with pytest.raises(ValueError, match="shape of q"):
        model.base_wrench_terms(q, qs[:, :5], qss)
    with pytest.raises(ValueError, match="Mount"):
        model.base_wrench(q, qs, qss, bw.MOUNT)

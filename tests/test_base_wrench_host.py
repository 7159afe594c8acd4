"""The base reaction without a GPU: the numpy reference (tests/base_wrench_ref.py) against routes of its own -- the joint-0
identity against tests/tree_ref.py's inverse dynamics, the weight at rest, a moved mount origin, relabelled arms -- each within
the bound of tests/base_wrench_cases.py's method, and the surface of ``Mount`` / ``BatchBaseWrenchConstraint`` and of the C
entries: every refusal happens before anything is launched (this machine has no GPU: a launch would raise ToppraHipError instead
of the expected error)."""
import ctypes

import numpy as np
import pytest

from tests import base_wrench_cases as bw, base_wrench_ref as bwr, chain_cases as cc, chain_ref, tree_cases as tc, tree_ref

BADARG = -1
SINGLE_ROOT = tuple(k for k in bw.CASES if k != "roots")


def _bound_of(robot, mount, args):
    """(reference, magnitude, bound) of one evaluation: 16 x the float64 reference's own error against np.longdouble."""
    ref, mag = bwr.base_wrench(robot, *args, mount=mount), bwr.base_wrench(robot, *args, mount=mount, absolute=True)
    return ref, mag, bw.BOUND_FACTOR * cc._own_error(ref, bwr.base_wrench(robot, *args, mount=mount, dtype=np.longdouble), mag)


# ---- the reference against routes of its own ---------------------------------------------------------------------------------

@pytest.mark.parametrize("key", SINGLE_ROOT)
def test_reference_joint_0_identity(key):
    """With the mount at joint 0's origin, the reaction along / about joint 0's axis is joint 0's force / torque: everything
    beyond the joint hangs on it.  Each side within its own bound of the other, on the all-absolute magnitude of the projection."""
    robot, q, qs, qss = bw.case(key)
    rnea = tree_ref.rnea if "parent" in robot else chain_ref.rnea
    at0 = {"rot": np.eye(3), "origin": robot["trans"][0], "mass": 0.0, "com": np.zeros(3)}
    axis = robot["rot"][0] @ robot["axis"][0]
    part = slice(0, 3) if int(robot["joint_type"][0]) == 1 else slice(3, 6)
    for name in ("w0", "wb"):
        args = bw.evaluations(q, qs, qss)[name]
        ref, mag, b_w = _bound_of(robot, at0, args)
        tau, tau_mag = rnea(robot, *args)[..., 0], rnea(robot, *args, absolute=True)[..., 0]
        b_tau = bw.BOUND_FACTOR * cc._own_error(rnea(robot, *args), rnea(robot, *args, dtype=np.longdouble), rnea(robot, *args, absolute=True))
        got, got_mag = ref[..., part] @ axis, mag[..., part] @ np.abs(axis)
        allow = b_w * got_mag + b_tau * tau_mag
        print("%s %s: |axis . w - tau_0| at most %.3g of its allowance" % (key, name, float(np.max(np.abs(got - tau)[allow > 0] / allow[allow > 0])) if (allow > 0).any() else 0.0))
        assert np.all(np.abs(got - tau) <= allow), (key, name)


@pytest.mark.parametrize("key", (3, 8, "torso", "nested"))
def test_reference_at_rest_carries_the_weight_at_the_centre_of_mass(key):
    """f = -(sum m + mb) gravity, and n is that force at the total centre of mass, in base axes about the base origin."""
    robot, q, _, _ = bw.case(key)
    robot = dict(robot, gravity=np.array([0.3, -0.2, -9.81]))
    plain = dict(bwr.NO_MOUNT, mass=bw.MOUNT["mass"], com=bw.MOUNT["com"])
    zero = np.zeros_like(q)
    ref, mag, bound = _bound_of(robot, plain, (q, zero, zero))
    total = robot["mass"].sum() + plain["mass"]
    f = -total * robot["gravity"]
    assert np.all(np.abs(ref[..., :3] - f) <= bound * mag[..., :3] + 4 * np.finfo(float).eps * np.abs(f))
    # the links' centres of mass in base coordinates, by a walk of its own
    parent, d = bwr.parents_of(robot), len(robot["mass"])
    R, p = [None] * d, [None] * d
    com = plain["mass"] * np.broadcast_to(plain["com"], q.shape[:-1] + (3,)).copy()
    for i in range(d):
        Rp = np.broadcast_to(np.eye(3), q.shape[:-1] + (3, 3)) if parent[i] < 0 else R[parent[i]]
        pp = np.zeros(q.shape[:-1] + (3,)) if parent[i] < 0 else p[parent[i]]
        k, qi = robot["axis"][i], q[..., i]
        if int(robot["joint_type"][i]) == 1:
            E = np.broadcast_to(robot["rot"][i], q.shape[:-1] + (3, 3))
            r = robot["trans"][i] + qi[..., None] * (robot["rot"][i] @ k)
        else:
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            rod = np.eye(3) + np.sin(qi)[..., None, None] * K + (1 - np.cos(qi))[..., None, None] * (K @ K)
            E, r = robot["rot"][i] @ rod, robot["trans"][i]
        R[i], p[i] = Rp @ E, pp + np.einsum("...ij,...j->...i", Rp, np.broadcast_to(r, q.shape[:-1] + (3,)))
        com = com + robot["mass"][i] * (p[i] + np.einsum("...ij,j->...i", R[i], robot["com"][i]))
    want = np.cross(com / total, f)
    assert np.all(np.abs(ref[..., 3:] - want) <= bound * mag[..., 3:] + 64 * np.finfo(float).eps * mag[..., 3:])


@pytest.mark.parametrize("key", (7, "skip", "roots"))
def test_reference_moving_the_mount_origin(key):
    """The moment about a point moved by delta changes by -delta x f (base axes)."""
    robot, q, qs, qss = bw.case(key)
    delta = np.array([0.25, -0.4, 0.15])
    here, there = dict(bwr.NO_MOUNT), dict(bwr.NO_MOUNT, origin=delta)
    a, mag_a, b_a = _bound_of(robot, here, (q, qs, qss))
    b, mag_b, b_b = _bound_of(robot, there, (q, qs, qss))
    assert np.array_equal(a[..., :3], b[..., :3])
    shift = np.cross(delta, a[..., :3])
    allow = b_a * mag_a[..., 3:] + b_b * mag_b[..., 3:] + 4 * np.finfo(float).eps * np.abs(np.cross(np.abs(delta), mag_a[..., :3]))
    assert np.all(np.abs(b[..., 3:] - (a[..., 3:] - shift)) <= allow)


def test_reference_relabelling_the_torso_s_arms():
    """The torso with its arms numbered the other way round (links 1-7 <-> 8-14): the same robot, the same reaction to the bound."""
    robot, q, qs, qss = bw.case("torso")
    perm = np.array([0] + list(range(8, 15)) + list(range(1, 8)))
    other = {k: (np.asarray(v)[perm] if k in ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia") else v) for k, v in robot.items()}
    other["parent"] = np.array(tc.SHAPES["torso"], dtype=np.int32)  # (the shape is symmetric: the table stays)
    args = tuple(a[..., perm] for a in (q, qs, qss))
    a, mag_a, b_a = _bound_of(robot, bw.MOUNT, (q, qs, qss))
    b, mag_b, b_b = _bound_of(other, bw.MOUNT, args)
    assert np.all(np.abs(a - b) <= b_a * mag_a + b_b * mag_b)
    assert b_a > 0 and b_b > 0


def test_a_chain_is_the_tree_of_its_links():
    chain, q, qs, qss = bw.case(7)
    as_tree = dict(chain, parent=np.arange(7) - 1)
    assert np.array_equal(bwr.base_wrench(chain, q, qs, qss, bw.MOUNT), bwr.base_wrench(as_tree, q, qs, qss, bw.MOUNT))


def test_the_bounds_are_positive_where_anything_is_summed():
    for key in bw.CASES:
        robot = bw.case(key)[0]
        for name in ("wa", "wb"):
            assert bw.bound(key, name) > 0, (key, name)
        assert (bw.bound(key, "w0") > 0) == bool(robot["gravity"].any())  # (without gravity nothing is summed: w0 is an exact zero)


# ---- Mount, the constraint, the entries -------------------------------------------------------------------------------------

def test_the_new_symbols_are_exported():
    import toppra_amd as ta
    from toppra_amd import _capi, batch, chain, constraint
    lib = _capi.load()
    for name in ("tpr_mount_bytes", "tpr_tree_base_wrench_batch", "tpr_tree_base_wrench_terms_batch"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert lib.tpr_mount_bytes() == 16 * 8 == ctypes.sizeof(_capi.tpr_mount)
    for cls in (chain.SerialChain, chain.KinematicTree):
        assert hasattr(cls, "base_wrench") and hasattr(cls, "base_wrench_terms")
    assert hasattr(batch, "base_wrench_batch") and hasattr(batch, "base_wrench_terms_batch")
    assert issubclass(constraint.BatchBaseWrenchConstraint, constraint._BatchChainRows)
    assert ta.Mount is chain.Mount and ta.BatchBaseWrenchConstraint is constraint.BatchBaseWrenchConstraint
    assert "Mount" in ta.__all__ and "BatchBaseWrenchConstraint" in ta.__all__


def test_mount_validation_and_defaults():
    from toppra_amd.chain import Mount
    m = Mount()
    assert np.array_equal(m.rotation, np.eye(3)) and not m.origin.any() and m.mass == 0.0 and not m.com.any()
    frame = m.c_struct()
    assert list(frame.rot) == list(np.eye(3).ravel()) and list(frame.origin) == [0.0] * 3 and frame.mass == 0.0
    m = bwr.mount_of(bw.MOUNT)
    frame = m.c_struct(None)
    assert list(frame.rot) == bw.MOUNT["rot"].ravel().tolist() and list(frame.origin) == bw.MOUNT["origin"].tolist()
    assert frame.mass == bw.MOUNT["mass"] and list(frame.com) == bw.MOUNT["com"].tolist()
    with pytest.raises(ValueError, match="mass must be >= 0"):
        Mount(mass=-1.0)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="not finite"):
            Mount(mass=bad)
        with pytest.raises(ValueError, match="not finite"):
            Mount(origin=(0.0, bad, 0.0))
        with pytest.raises(ValueError, match="not finite"):
            Mount(com=(bad, 0.0, 0.0))
        with pytest.raises(ValueError, match="not finite"):
            Mount(rotation=np.diag([1.0, bad, 1.0]))
    with pytest.raises(ValueError, match=r"origin must have shape \[3\]"):
        Mount(origin=(0.0, 1.0))
    with pytest.raises(ValueError, match=r"com must have shape \[3\]"):
        Mount(com=np.zeros((3, 1)))
    with pytest.raises(ValueError, match=r"rotation must have shape \[3, 3\]"):
        Mount(rotation=np.ones(3))
    with pytest.raises(ValueError, match="orthonormal"):
        Mount(rotation=np.eye(3) * 1.001)
    with pytest.raises(ValueError, match="orthonormal"):
        Mount(rotation=np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError, match="not an array of numbers"):
        Mount(origin="floor")


def _robots():
    return chain_ref.serial_chain(chain_ref.random_chain(3, 5)), tree_ref.kinematic_tree(tree_ref.random_tree([-1, 0, 0], 5))


def _problem(B=3, d=3, N=10):
    from toppra_amd import batch
    data = batch.make_synthetic_batch(B, d, N, seed=3)
    return data, (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])


def test_rows_per_stage_and_the_rows_of_each_spelling():
    from toppra_amd import constraint
    C, DT = constraint.BatchBaseWrenchConstraint, constraint.DiscretizationType
    mount = bwr.mount_of(bw.MOUNT)
    for robot in _robots():
        assert C(robot, force=0.5).get_discretization_type() == DT.Interpolation
        assert C(robot, force=0.5).rows_per_stage(3) == 12 and C(robot, mount, force=0.5, moment=2.0).rows_per_stage(3) == 24
        assert C(robot, mount, moment=2.0, discretization_scheme=DT.Collocation).rows_per_stage(3) == 6
        assert C(robot, F=np.ones((5, 6)), g=np.ones(5)).rows_per_stage(3) == 10
        assert C(robot, None, F=np.ones((4, 11, 5, 6)), g=np.ones((4, 5)), discretization_scheme=DT.Collocation).rows_per_stage(3) == 5
        con = C.surface_contact(robot, 0.5, (0.3, 0.2), mount=mount, normal_force_min=3.0)
        F, g = constraint.BatchToolWrenchConstraint.surface_contact_rows(0.5, (0.3, 0.2), 3.0)
        assert np.array_equal(con.F, F) and np.array_equal(con.g, g) and con.rows_per_stage(3) == 34 and con.mount is mount
        assert C.surface_contact(robot, 0.5, (0.3, 0.2)).mount.mass == 0.0
        lim = np.stack([-np.arange(1.0, 13.0).reshape(4, 3), np.arange(2.0, 14.0).reshape(4, 3)], -1)  # [B = 4, 3, 2]
        con = C(robot, mount, force=0.5, moment=lim)
        assert con.g.shape == (4, 12) and np.array_equal(con.g[1], [0.5] * 6 + [5.0, 6.0, 7.0, 4.0, 5.0, 6.0])
        con.check(4, 10, 3)
    assert "F w(q, 0, 0) <= g" in C.__doc__


def test_the_constraint_refuses_before_any_launch():
    from toppra_amd import algorithm, constraint
    C = constraint.BatchBaseWrenchConstraint
    sc3, tree3 = _robots()
    sc4 = chain_ref.serial_chain(chain_ref.random_chain(4, 5))
    data, args = _problem()
    with pytest.raises(ValueError, match="SerialChain or KinematicTree"):
        C(lambda q, qd, qdd: q, force=0.5)
    with pytest.raises(ValueError, match="Mount"):
        C(sc3, bw.MOUNT, force=0.5)
    with pytest.raises(ValueError, match="no limit given"):
        C(tree3)
    with pytest.raises(ValueError, match="not both"):
        C(sc3, force=0.5, F=np.ones((2, 6)), g=np.ones(2))
    with pytest.raises(ValueError, match="not both"):
        C.surface_contact(tree3, 0.5, (0.1, 0.1), force=10.0)
    with pytest.raises(ValueError, match="together"):
        C(sc3, F=np.ones((2, 6)))
    with pytest.raises(ValueError, match=r"force must be a scalar or have shape \[3, 2\]"):
        C(sc3, force=np.ones(3))
    with pytest.raises(ValueError, match="above its upper"):
        C(tree3, moment=-0.5)
    with pytest.raises(ValueError, match=r"\[m, 6\]"):
        C(sc3, F=np.ones((2, 3)), g=np.ones(2))
    with pytest.raises(ValueError, match="not finite"):
        C(sc3, F=np.ones((2, 6)), g=np.array([1.0, np.nan]))
    for bad in dict(mu=0.0), dict(half_extents=(0.1, 0.0)), dict(normal_force_min=-1.0):
        with pytest.raises(ValueError):
            C.surface_contact(sc3, **dict(dict(mu=0.5, half_extents=(0.1, 0.1)), **bad))
    with pytest.raises(ValueError, match="has 4 joints"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc4, force=0.5)])
    with pytest.raises(ValueError, match="per trajectory for 5"):
        algorithm.BatchTOPPRA(*args, constraints=[C(tree3, force=np.tile([-1.0, 1.0], (5, 3, 1)))])
    with pytest.raises(ValueError, match="leading shape"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, F=np.ones((5, 2, 6)), g=np.ones(2))])
    qs = np.random.default_rng(0).standard_normal((3, 11, 3))
    with pytest.raises(ValueError, match="path positions"):
        algorithm.BatchTOPPRA.from_path_samples(data["grid"], None, qs, qs, data["vlim"], data["alim"], constraints=[C(tree3, force=0.5)])
    with pytest.raises(NotImplementedError, match="BatchTOPPRA"):
        C(sc3, force=0.5).compute_constraint_params(None, None)
    with pytest.raises(NotImplementedError, match="BatchBaseWrenchConstraint and BatchToolWrenchConstraint are supported"):
        algorithm.BatchTOPPRA(*args, constraints=[constraint.JointAccelerationConstraint(data["alim"][0])])
    # a valid list passes the constructor, beside a torque limit on the same robot (its launches come later, on first use)
    taulim = np.stack([-np.ones(3), np.ones(3)], -1)
    inst = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchJointTorqueConstraint(tree3, taulim, np.zeros(3)),
                                                     C.surface_contact(tree3, 0.5, (0.3, 0.2), mount=bwr.mount_of(bw.MOUNT))])
    assert len(inst.constraints) == 2


def test_array_entries_refuse_wrong_shapes_before_any_launch():
    from toppra_amd import batch
    q = np.zeros((2, 5, 3))
    for robot in _robots():
        with pytest.raises(ValueError, match="dof"):
            batch.base_wrench_batch(robot, np.zeros((2, 5, 4)), np.zeros((2, 5, 4)), np.zeros((2, 5, 4)))
        with pytest.raises(ValueError, match="shape of q"):
            batch.base_wrench_batch(robot, q, q, np.zeros((2, 4, 3)))
        with pytest.raises(ValueError, match="shape of q"):
            batch.base_wrench_terms_batch(robot, q, np.zeros((2, 4, 3)), q, bwr.mount_of(bw.MOUNT))
        with pytest.raises(ValueError, match="Mount"):
            batch.base_wrench_batch(robot, q, q, q, bw.MOUNT)


def _c_calls(model, parent, mount, B=2, N=1, q=True):
    from toppra_amd import _capi
    lib = _capi.load()
    p = np.zeros(64)
    _c_calls.keep = p
    ptr = p.ctypes.data
    m = None if model is None else ctypes.byref(model)
    t = None if parent is None else parent.ctypes.data
    f = None if mount is None else ctypes.byref(mount)
    first = ptr if q else None
    single = lib.tpr_tree_base_wrench_batch(m, t, f, B * (N + 1), first, ptr, ptr, ptr, 0, None), lib.tpr_last_error()
    terms = lib.tpr_tree_base_wrench_terms_batch(m, t, f, B, N, first, ptr, ptr, ptr, ptr, ptr, 0, None), lib.tpr_last_error()
    return single, terms


def test_entries_refuse_in_their_order_without_a_device():
    """What an entry decides before it looks for a device: the terms entry refuses B < 0 or N < 0 first, as its siblings do; valid
    early arguments reach the device check, which refuses with "tpr_init" -- nothing computes without a GPU."""
    from toppra_amd import _capi
    sc = chain_ref.serial_chain(chain_ref.random_chain(3, 5))
    model, keep = sc.c_struct(np.zeros(1))
    parent = np.array([-1, 0, 1], dtype=np.int32)
    mount = bwr.mount_of(bw.MOUNT).c_struct()
    lib = _capi.load()
    p = np.zeros(64).ctypes.data
    for B, N in ((-1, 1), (1, -1)):
        assert lib.tpr_tree_base_wrench_terms_batch(None, None, None, B, N, None, p, p, p, p, p, 0, None) == BADARG
        msg = lib.tpr_last_error()
        assert b"B >= 0, N >= 0" in msg and b"tpr_tree_base_wrench_terms_batch" in msg, msg
    if _capi.device_count() == 0:  # (with a device the calls would be valid and run)
        for (rc, msg) in _c_calls(model, parent, mount) + _c_calls(model, parent, None):
            assert rc < 0 and b"tpr_init" in msg, msg
        q = np.zeros((2, 5, 3))
        for robot in _robots():
            with pytest.raises(_capi.ToppraHipError):
                robot.base_wrench(q, q, q)
            with pytest.raises(_capi.ToppraHipError):
                robot.base_wrench_terms(q, q, q, bwr.mount_of(bw.MOUNT))

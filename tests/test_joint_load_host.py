"""Joint loads without a GPU: the numpy reference (tests/joint_load_ref.py) against first principles -- a leaf section against
single-body Newton-Euler, the weight of the subtree at rest, the joint's own torque against tests/tree_ref.py --, the link-local
restatement against the accuracy bound (the measurement behind the kernels' recipe), ``bearing_rows`` and
``on_axes``, and the surface of ``JointSections`` / ``BatchJointLoadConstraint`` and of the C entries: every refusal happens
before anything is launched (this machine has no GPU: a launch would raise ToppraHipError instead of the expected error)."""
import ctypes

import numpy as np
import pytest

from tests import base_wrench_ref as bwr, chain_cases as cc, chain_ref, joint_load_cases as jc, joint_load_ref as jr
from tests import tree_cases as tc, tree_ref

BADARG = -1
EPS = np.finfo(float).eps


def _bound_of(robot, sec, args):
    """(reference, magnitude, bound) of one evaluation: 16 x the float64 reference's own error against np.longdouble."""
    ref, mag = jr.joint_wrenches(robot, *args, sections=sec), jr.joint_wrenches(robot, *args, sections=sec, absolute=True)
    return ref, mag, jc.BOUND_FACTOR * cc._own_error(ref, jr.joint_wrenches(robot, *args, sections=sec, dtype=np.longdouble), mag)


def _link_frames(robot, q):
    """(R [d][..., 3, 3], p [d][..., 3]) of every link in base coordinates, by a walk of its own."""
    parent, d = bwr.parents_of(robot), len(robot["mass"])
    R, p = [None] * d, [None] * d
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
    return R, p


# ---- the reference against first principles -----------------------------------------------------------------------------------

def _link_motion(robot, q, qd, qdd):
    """(R, w, wd, a) of every link in base axes -- a is the link origin's acceleration with the base at -gravity --, by a walk of
    its own on whole arrays."""
    parent, d = bwr.parents_of(robot), len(robot["mass"])
    R, p = _link_frames(robot, q)
    lead = q.shape[:-1]
    w, wd, a = [None] * d, [None] * d, [None] * d
    for i in range(d):
        up = parent[i]
        Rp = np.broadcast_to(np.eye(3), lead + (3, 3)) if up < 0 else R[up]
        w0, wd0 = (np.zeros(lead + (3,)), np.zeros(lead + (3,))) if up < 0 else (w[up], wd[up])
        a0 = np.broadcast_to(-np.asarray(robot["gravity"], dtype=float), lead + (3,)) if up < 0 else a[up]
        r = p[i] - (0.0 if up < 0 else p[up])
        z = np.einsum("...ij,j->...i", Rp, robot["rot"][i] @ robot["axis"][i])
        vi, ai = qd[..., i, None], qdd[..., i, None]
        a[i] = a0 + np.cross(wd0, r) + np.cross(w0, np.cross(w0, r))
        if int(robot["joint_type"][i]) == 1:
            w[i], wd[i] = w0, wd0
            a[i] = a[i] + z * ai + 2.0 * vi * np.cross(w0, z)
        else:
            w[i], wd[i] = w0 + z * vi, wd0 + z * ai + vi * np.cross(w0, z)
    return R, w, wd, a


@pytest.mark.parametrize("key", (1, 7, 9, "vee", "nested", "torso"))
def test_reference_leaf_section_is_single_body_newton_euler(key):
    """A leaf carries nothing but itself: f = m a_c and, about the link's origin, n = I wd + w x I w + c x f, with the link's
    motion from a second walk; both in the link's axes."""
    robot, q, qs, qss = jc.case(key)
    robot = dict(robot, gravity=np.array([0.3, -0.2, -9.81]))
    leaf = tc.leaves_of(bwr.parents_of(robot))[-1]
    sec = jr.default_sections([leaf])
    ref, mag, bound = _bound_of(robot, sec, (q, qs, qss))
    R, w, wd, a = _link_motion(robot, q, qs, qss)
    Rl, m, I = R[leaf], robot["mass"][leaf], robot["inertia"][leaf]
    c = np.einsum("...ij,j->...i", Rl, robot["com"][leaf])
    f = m * (a[leaf] + np.cross(wd[leaf], c) + np.cross(w[leaf], np.cross(w[leaf], c)))
    Il = np.array([[I[0], I[3], I[4]], [I[3], I[1], I[5]], [I[4], I[5], I[2]]])
    Iw = Rl @ Il @ np.swapaxes(Rl, -1, -2)
    mul = lambda M, v: np.einsum("...ij,...j->...i", M, v)  # noqa: E731
    n = mul(Iw, wd[leaf]) + np.cross(w[leaf], mul(Iw, w[leaf])) + np.cross(c, f)
    want = np.concatenate((mul(np.swapaxes(Rl, -1, -2), f), mul(np.swapaxes(Rl, -1, -2), n)), -1)[..., None, :]
    assert np.all(np.abs(ref - want) <= bound * mag + 64 * EPS * mag), key


@pytest.mark.parametrize("key", (3, 8, "vee", "nested", "torso", "comb32"))
def test_reference_at_rest_carries_the_subtree_s_weight(key):
    """At rest the force of every section is -(subtree mass) gravity in section axes, to the reference's own rounding; for a fork
    the subtree is every child branch."""
    robot, q, _, _ = jc.case(key)
    robot = dict(robot, gravity=np.array([0.3, -0.2, -9.81]))
    parents, sec = bwr.parents_of(robot), jc.sections(key)
    zero = np.zeros_like(q)
    ref, mag, bound = _bound_of(robot, sec, (q, zero, zero))
    R, _ = _link_frames(robot, q)
    for k, link in enumerate(sec["link"].tolist()):
        sub = [i for i in range(len(parents)) if link in tc.path_to(parents, i)]
        weight = -robot["mass"][sub].sum() * robot["gravity"]
        want = np.einsum("ji,...j->...i", sec["rot"][k], np.einsum("...ji,j->...i", R[link], weight))
        assert np.all(np.abs(ref[..., k, :3] - want) <= bound * mag[..., k, :3] + 16 * EPS * mag[..., k, :3]), (key, link)


@pytest.mark.parametrize("key", jc.CASES)
def test_default_sections_reproduce_the_joint_torques(key):
    """axis . n (revolute) / axis . f (prismatic) of a default section on every joint is tree_ref's torque: the same world-frame
    recursion, projected in the link's frame instead of the world's -- each side within its own bound."""
    robot, q, qs, qss = jc.case(key)
    d = q.shape[-1]
    as_tree = dict(robot, parent=np.array(bwr.parents_of(robot), dtype=np.int32))
    sec = jr.default_sections(range(d))
    prismatic = np.asarray(robot["joint_type"]) == 1
    part = lambda x: np.where(prismatic[:, None], x[..., :3], x[..., 3:])  # noqa: E731
    for name in ("w0", "wb"):
        args = jc.evaluations(q, qs, qss)[name]
        ref, mag, b_w = _bound_of(robot, sec, args)
        tau, tau_mag = tree_ref.rnea(as_tree, *args), tree_ref.rnea(as_tree, *args, absolute=True)
        b_tau = jc.BOUND_FACTOR * cc._own_error(tau, tree_ref.rnea(as_tree, *args, dtype=np.longdouble), tau_mag)
        got = np.einsum("...dk,dk->...d", part(ref), robot["axis"])
        allow = b_w * np.einsum("...dk,dk->...d", part(mag), np.abs(robot["axis"])) + b_tau * tau_mag
        assert np.all(np.abs(got - tau) <= allow), (key, name)


def test_a_chain_is_the_tree_of_its_links():
    chain, q, qs, qss = jc.case(7)
    as_tree = dict(chain, parent=np.arange(7) - 1)
    sec = jc.sections(7)
    assert np.array_equal(jr.joint_wrenches(chain, q, qs, qss, sec), jr.joint_wrenches(as_tree, q, qs, qss, sec))
    assert np.array_equal(jr.local_joint_wrenches(chain, q, qs, qss, sec), jr.local_joint_wrenches(as_tree, q, qs, qss, sec))


def test_the_cases_hold_what_they_must():
    for key in jc.CASES:
        parents = bwr.parents_of(jc.case(key)[0])
        links = jc.sections(key)["link"].tolist()
        d = len(parents)
        assert 0 in links and links.count(d - 1) == 2 or d == 1 and links == [0, 0], (key, links)
        for j in tc.forks_of(parents):
            assert j in links and any(parents[i] == j and i != j + 1 for i in links), (key, j)
        assert all(1 <= len(s) <= jc.MAX_SECTIONS for s in jc.section_sets(key))
        assert sum(len(s) for s in jc.section_sets(key)) == len(links)
        for name in ("wa", "wb"):
            assert jc.bound(key, name) > 0, (key, name)
        assert (jc.bound(key, "w0") > 0) == bool(jc.case(key)[0]["gravity"].any())


def test_the_restatement_stays_within_the_recipe_s_share_of_the_bounds():
    """The measurement behind the kernels' recipe (the plain link-local recursion, tree_rnea's with (f, n) kept): the float64
    restatement of that order against the bounds, on every case and quantity.  Where gravity acts -- the part the other recipe
    would treat differently -- every quantity stays within HALF its bound (measured: at most 0.42, the 17-dof chain's wb).
    Without gravity the weight's share is an exact zero and the two recipes are the same arithmetic: there the restatement must
    hold the bound itself (measured: at most 0.55, the 32-dof chain's wb -- the figure is the link-local recursion's dynamic
    part, which the base-reaction kernels share).  profiles/joint_load_accuracy.json records every fraction."""
    assert jc.RECIPE == "A"
    for key in jc.CASES:
        gravity = bool(jc.case(key)[0]["gravity"].any())
        for name, frac in jc.restatement_fractions(key).items():
            print("%s %s: %.3f of the bound" % (key, name, frac))
            if jc.bound(key, name) == 0:
                assert frac == 0.0, (key, name)
            else:
                assert frac <= (jc.RECIPE_A_SHARE if gravity else 1.0), (key, name, frac)
    assert jc.worst_restatement(True) <= jc.RECIPE_A_SHARE


# ---- bearing_rows, on_axes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sides", (3, 4, 6, 8, 11))
def test_bearing_rows_are_the_inscribed_polygon(sides):
    from toppra_amd.constraint import BatchJointLoadConstraint as C
    count, tilting, radial, axial = 2, np.array([3.0, 0.7]), np.array([40.0, 9.0]), np.array([5.0, 2.0])
    F, g = C.bearing_rows(count, tilting, axial, radial, sides)
    assert F.shape == (count * (2 * sides + 2), 6 * count) and g.shape == (F.shape[0],)
    per = 2 * sides + 2
    for k in range(count):
        rows = slice(per * k, per * (k + 1))
        other = [c for c in range(6 * count) if c // 6 != k]
        assert not F[rows][:, other].any() and not F[rows, 6 * k + 5].any()  # (the moment about the axis is left to the torque limit)
        for at, lim, first in ((3, tilting[k], 0), (0, radial[k], sides)):
            A, b = F[per * k + first:per * k + first + sides, 6 * k + at:6 * k + at + 2], g[per * k + first:per * k + first + sides]
            # every vertex of the polygon (two neighbouring rows tight) lies on or inside the circle of the data sheet
            for j in range(sides):
                pair = [j, (j + 1) % sides]
                v = np.linalg.solve(A[pair], b[pair])
                assert np.hypot(*v) <= lim * (1 + 4 * EPS), (sides, k, j)
                assert np.all(A @ v <= b * (1 + 4 * EPS) + 4 * EPS * lim)
            # points within the inner circle satisfy every row
            t = np.linspace(0.0, 2 * np.pi, 97)
            inner = lim * np.cos(np.pi / sides) * np.stack([np.cos(t), np.sin(t)])
            assert np.all(A @ inner <= b[:, None] * (1 + 4 * EPS))
        ax = F[per * k + 2 * sides:per * (k + 1)]
        assert np.array_equal(ax[:, 6 * k + 2], [1.0, -1.0]) and np.count_nonzero(ax) == 2 and np.array_equal(g[per * k + 2 * sides:per * (k + 1)], [axial[k]] * 2)
    # parts left out
    F, g = C.bearing_rows(3, axial=2.0)
    assert F.shape == (6, 18) and np.array_equal(g, [2.0] * 6)
    F, g = C.bearing_rows(1, tilting=1.0, sides=sides)
    assert F.shape == (sides, 6) and not F[:, :3].any()
    for bad in (dict(), dict(tilting=-1.0), dict(axial=[1.0, 2.0]), dict(radial=np.nan), dict(tilting=1.0, sides=2)):
        with pytest.raises(ValueError):
            C.bearing_rows(1, **bad)


def test_on_axes_frames():
    from toppra_amd.chain import JointSections
    for robot in (chain_ref.serial_chain(cc.case(9)[0]), tree_ref.kinematic_tree(tc.case("torso")[0])):
        joints = [0, 3, 5, -1]
        offs = np.array([0.0, 0.1, -0.2, 0.05])
        sec = JointSections.on_axes(robot, joints, offs)
        links = sec.on(robot)
        assert links.tolist() == [0, 3, 5, robot.dof - 1]
        for k, i in enumerate(links.tolist()):
            R, a = sec.rotations[k], robot.axes[i]
            assert np.all(np.abs(R.T @ R - np.eye(3)) <= 4 * EPS) and abs(np.linalg.det(R) - 1.0) <= 8 * EPS
            assert np.array_equal(R[:, 2], a) and np.array_equal(sec.origins[k], a * offs[k])
            e = np.zeros(3)
            e[int(np.argmin(np.abs(a)))] = 1.0
            assert R[:, 0] @ e > 0 and abs(R[:, 0] @ a) <= 4 * EPS
            assert np.allclose(R[:, 1], np.cross(a, R[:, 0]), rtol=0, atol=4 * EPS)
        assert np.array_equal(JointSections.on_axes(robot, [2]).origins, np.zeros((1, 3)))
    # a coordinate axis: ties go to the lowest index
    sc = chain_ref.serial_chain(dict(cc.case(1)[0], axis=np.array([[0.0, 0.0, 1.0]])))
    assert np.array_equal(JointSections.on_axes(sc, [0]).rotations[0], np.eye(3))
    with pytest.raises(ValueError, match="joints 0..0"):
        JointSections.on_axes(sc, [1])
    with pytest.raises(ValueError, match="offsets"):
        JointSections.on_axes(sc, [0], [0.1, 0.2])


# ---- JointSections, the constraint, the entries --------------------------------------------------------------------------------

def test_the_new_symbols_are_exported():
    import toppra_amd as ta
    from toppra_amd import _capi, batch, chain, constraint
    lib = _capi.load()
    for name in ("tpr_joint_sections_bytes", "tpr_tree_joint_wrench_batch", "tpr_tree_joint_wrench_terms_batch"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert lib.tpr_joint_sections_bytes() == 40 + 8 * 12 * 8 == ctypes.sizeof(_capi.tpr_joint_sections)
    assert _capi.JOINT_MAX_SECTIONS == 8
    for cls in (chain.SerialChain, chain.KinematicTree):
        assert hasattr(cls, "joint_wrenches") and hasattr(cls, "joint_wrench_terms")
    assert hasattr(batch, "joint_wrench_batch") and hasattr(batch, "joint_wrench_terms_batch")
    assert issubclass(constraint.BatchJointLoadConstraint, constraint._BatchChainRows)
    assert ta.JointSections is chain.JointSections and ta.BatchJointLoadConstraint is constraint.BatchJointLoadConstraint
    assert "JointSections" in ta.__all__ and "BatchJointLoadConstraint" in ta.__all__


def test_joint_sections_validation_and_defaults():
    from toppra_amd.chain import JointSections
    sc = chain_ref.serial_chain(chain_ref.random_chain(5, 5))
    s = JointSections([0, -1, 2])
    assert len(s) == 3 and np.array_equal(s.rotations, np.tile(np.eye(3), (3, 1, 1))) and not s.origins.any()
    assert s.on(sc).tolist() == [0, 4, 2]
    c = s.c_struct(sc)
    assert c.count == 3 and list(c.link)[:3] == [0, 4, 2] and list(c.rot[1]) == np.eye(3).ravel().tolist() and list(c.origin[2]) == [0.0] * 3
    with pytest.raises(ValueError):
        s.origins[0, 0] = 1.0  # (immutable)
    with pytest.raises(ValueError):
        s.joints[0] = 1
    sec = jc.sections("nested")
    c = jr.joint_sections_of(sec).c_struct(tree_ref.kinematic_tree(tc.case("nested")[0]))
    for k in range(len(sec["link"])):
        assert c.link[k] == sec["link"][k] and list(c.rot[k]) == sec["rot"][k].ravel().tolist() and list(c.origin[k]) == sec["origin"][k].tolist()
    with pytest.raises(ValueError, match="1..8 sections"):
        JointSections([])
    with pytest.raises(ValueError, match="1..8 sections"):
        JointSections(list(range(9)))
    with pytest.raises(ValueError, match="1..8 sections"):
        JointSections([[0, 1]])
    with pytest.raises(ValueError, match="integers"):
        JointSections([0.5])
    with pytest.raises(ValueError, match="-1 .. 31"):
        JointSections([-2])
    with pytest.raises(ValueError, match="-1 .. 31"):
        JointSections([32])
    with pytest.raises(ValueError, match=r"origins must have shape \[2, 3\]"):
        JointSections([0, 1], origins=np.zeros(3))
    with pytest.raises(ValueError, match=r"rotations must have shape \[1, 3, 3\]"):
        JointSections([0], rotations=np.eye(3))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="not finite"):
            JointSections([0], origins=[[0.0, bad, 0.0]])
        with pytest.raises(ValueError, match="not finite"):
            JointSections([0], rotations=[np.diag([1.0, bad, 1.0])])
    with pytest.raises(ValueError, match="orthonormal"):
        JointSections([0], rotations=[np.eye(3) * 1.001])
    with pytest.raises(ValueError, match="orthonormal"):
        JointSections([0], rotations=[np.diag([1.0, 1.0, -1.0])])
    with pytest.raises(ValueError, match="not an array of numbers"):
        JointSections([0], origins="flange")
    with pytest.raises(ValueError, match="joints 0..4"):
        JointSections([5]).on(sc)
    with pytest.raises(ValueError, match="joints 0..4"):
        JointSections([5]).c_struct(sc)


def _robots():
    return chain_ref.serial_chain(chain_ref.random_chain(3, 5)), tree_ref.kinematic_tree(tree_ref.random_tree([-1, 0, 0], 5))


def _problem(B=3, d=3, N=10):
    from toppra_amd import batch
    data = batch.make_synthetic_batch(B, d, N, seed=3)
    return data, (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])


def test_rows_per_stage_and_the_rows_of_each_spelling():
    from toppra_amd import constraint
    from toppra_amd.chain import JointSections
    C, DT = constraint.BatchJointLoadConstraint, constraint.DiscretizationType
    two = JointSections([0, -1])
    I3 = np.eye(3)
    for robot in _robots():
        assert C(robot, two, force=0.5).get_discretization_type() == DT.Interpolation
        assert C(robot, two, force=0.5).rows_per_stage(3) == 24 and C(robot, two, force=0.5, moment=2.0).rows_per_stage(3) == 48
        assert C(robot, two, moment=2.0, discretization_scheme=DT.Collocation).rows_per_stage(3) == 12
        assert C(robot, two, F=np.ones((5, 12)), g=np.ones(5)).rows_per_stage(3) == 10
        assert C(robot, two, F=np.ones((4, 11, 5, 12)), g=np.ones((4, 5)), discretization_scheme=DT.Collocation).rows_per_stage(3) == 5
        con = C(robot, two, force=[1.0, 2.0], moment=0.5)
        want = np.zeros((24, 12))
        for k in range(2):
            for j, at in enumerate((0, 3)):
                want[12 * k + 6 * j:12 * k + 6 * j + 3, 6 * k + at:6 * k + at + 3] = I3
                want[12 * k + 6 * j + 3:12 * k + 6 * j + 6, 6 * k + at:6 * k + at + 3] = -I3
        assert np.array_equal(con.F, want) and np.array_equal(con.g, [1.0] * 6 + [0.5] * 6 + [2.0] * 6 + [0.5] * 6)
        lim = np.stack([-np.arange(1.0, 25.0).reshape(4, 2, 3), np.arange(2.0, 26.0).reshape(4, 2, 3)], -1)  # [B = 4, S, 3, 2]
        con = C(robot, two, force=0.5, moment=lim)
        assert con.g.shape == (4, 24) and np.array_equal(con.g[1], [0.5] * 6 + [8.0, 9.0, 10.0, 7.0, 8.0, 9.0] + [0.5] * 6 + [11.0, 12.0, 13.0, 10.0, 11.0, 12.0])
        con.check(4, 10, 3)
        only = C(robot, two, moment=lim[0])
        assert only.F.shape == (12, 12) and not only.F[:, [0, 1, 2, 6, 7, 8]].any()
        con = C.bearing(robot, two, tilting=[1.0, 2.0], axial=3.0, sides=4)
        F, g = C.bearing_rows(2, [1.0, 2.0], 3.0, None, 4)
        assert np.array_equal(con.F, F) and np.array_equal(con.g, g) and con.rows_per_stage(3) == 24 and con.sections is two
    assert "F w(q, 0, 0) <= g" in C.__doc__ and "from_path_samples" in C.__doc__ and "out of\n    scope" in C.__doc__


def test_the_constraint_refuses_before_any_launch():
    from toppra_amd import algorithm, constraint
    from toppra_amd.chain import JointSections
    C = constraint.BatchJointLoadConstraint
    sc3, tree3 = _robots()
    sc4 = chain_ref.serial_chain(chain_ref.random_chain(4, 5))
    two = JointSections([0, -1])
    data, args = _problem()
    with pytest.raises(ValueError, match="SerialChain or KinematicTree"):
        C(lambda q, qd, qdd: q, two, force=0.5)
    with pytest.raises(ValueError, match="JointSections"):
        C(sc3, [0, 2], force=0.5)
    with pytest.raises(ValueError, match="JointSections"):
        C.bearing(sc3, [0, 2], axial=0.5)
    with pytest.raises(ValueError, match="joints 0..2"):
        C(sc3, JointSections([3]), force=0.5)
    with pytest.raises(ValueError, match="no limit given"):
        C(tree3, two)
    with pytest.raises(ValueError, match="not both"):
        C(sc3, two, force=0.5, F=np.ones((2, 12)), g=np.ones(2))
    with pytest.raises(ValueError, match="not both"):
        C.bearing(tree3, two, axial=1.0, force=10.0)
    with pytest.raises(ValueError, match="together"):
        C(sc3, two, F=np.ones((2, 12)))
    with pytest.raises(ValueError, match=r"force must be a scalar or have shape \[S\], \[S, 3, 2\]"):
        C(sc3, two, force=np.ones(3))
    with pytest.raises(ValueError, match=r"moment must be a scalar or have shape"):
        C(sc3, two, moment=np.ones((3, 2)))
    with pytest.raises(ValueError, match="above its upper"):
        C(tree3, two, moment=-0.5)
    with pytest.raises(ValueError, match="not finite"):
        C(tree3, two, force=np.inf)
    with pytest.raises(ValueError, match=r"\[m, 6 S\]"):
        C(sc3, two, F=np.ones((2, 6)), g=np.ones(2))
    with pytest.raises(ValueError, match="not finite"):
        C(sc3, two, F=np.ones((2, 12)), g=np.array([1.0, np.nan]))
    with pytest.raises(ValueError, match="per trajectory for 4 and 5"):
        C(sc3, two, force=np.tile([-1.0, 1.0], (4, 2, 3, 1)), moment=np.tile([-1.0, 1.0], (5, 2, 3, 1)))
    with pytest.raises(ValueError, match="has 4 joints"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc4, two, force=0.5)])
    with pytest.raises(ValueError, match="per trajectory for 5"):
        algorithm.BatchTOPPRA(*args, constraints=[C(tree3, two, force=np.tile([-1.0, 1.0], (5, 2, 3, 1)))])
    with pytest.raises(ValueError, match="leading shape"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, two, F=np.ones((5, 2, 12)), g=np.ones(2))])
    qs = np.random.default_rng(0).standard_normal((3, 11, 3))
    with pytest.raises(ValueError, match="path positions"):
        algorithm.BatchTOPPRA.from_path_samples(data["grid"], None, qs, qs, data["vlim"], data["alim"], constraints=[C(tree3, two, force=0.5)])
    with pytest.raises(NotImplementedError, match="BatchTOPPRA"):
        C(sc3, two, force=0.5).compute_constraint_params(None, None)
    # the existing cap on the rows of a stage, with its existing refusal: 8 sections x 12 rows x 2 (Interpolation) = 192 > 122
    eight = JointSections([0, 1, 2, 0, 1, 2, 0, 1])
    with pytest.raises(NotImplementedError, match="constraint rows per stage"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, eight, force=0.5, moment=0.5)])
    # a valid list passes the constructor, beside a torque limit on the same robot (its launches come later, on first use)
    taulim = np.stack([-np.ones(3), np.ones(3)], -1)
    inst = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchJointTorqueConstraint(tree3, taulim, np.zeros(3)),
                                                     C.bearing(tree3, two, tilting=1.0, axial=2.0, radial=3.0)])
    assert len(inst.constraints) == 2


def test_array_entries_refuse_wrong_shapes_before_any_launch():
    from toppra_amd import batch
    from toppra_amd.chain import JointSections
    q = np.zeros((2, 5, 3))
    two = JointSections([0, -1])
    for robot in _robots():
        with pytest.raises(ValueError, match="dof"):
            batch.joint_wrench_batch(robot, np.zeros((2, 5, 4)), np.zeros((2, 5, 4)), np.zeros((2, 5, 4)), two)
        with pytest.raises(ValueError, match="shape of q"):
            batch.joint_wrench_batch(robot, q, q, np.zeros((2, 4, 3)), two)
        with pytest.raises(ValueError, match="shape of q"):
            batch.joint_wrench_terms_batch(robot, q, np.zeros((2, 4, 3)), q, two)
        with pytest.raises(ValueError, match="JointSections"):
            batch.joint_wrench_batch(robot, q, q, q, [0, 2])
        with pytest.raises(ValueError, match="joints 0..2"):
            robot.joint_wrenches(q, q, q, JointSections([7]))


def test_entries_refuse_in_their_order_without_a_device():
    """What an entry decides before it looks for a device: the terms entry refuses B < 0 or N < 0 first, as its siblings do; valid
    early arguments reach the device check, which refuses with "tpr_init" -- nothing computes without a GPU."""
    from toppra_amd import _capi
    from toppra_amd.chain import JointSections
    sc = chain_ref.serial_chain(chain_ref.random_chain(3, 5))
    model, keep = sc.c_struct(np.zeros(1))
    parent = np.array([-1, 0, 1], dtype=np.int32)
    sec = JointSections([0, 2]).c_struct(sc)
    lib = _capi.load()
    buf = np.zeros(64)
    p = buf.ctypes.data
    for B, N in ((-1, 1), (1, -1)):
        assert lib.tpr_tree_joint_wrench_terms_batch(None, None, None, B, N, None, p, p, p, p, p, 0, None) == BADARG
        msg = lib.tpr_last_error()
        assert b"B >= 0, N >= 0" in msg and b"tpr_tree_joint_wrench_terms_batch" in msg, msg
    if _capi.device_count() == 0:  # (with a device the calls would be valid and run)
        m, t, f = ctypes.byref(model), parent.ctypes.data, ctypes.byref(sec)
        results = [(lib.tpr_tree_joint_wrench_batch(m, t, f, 4, p, p, p, p, 0, None), lib.tpr_last_error()),
                   (lib.tpr_tree_joint_wrench_terms_batch(m, t, f, 2, 1, p, p, p, p, p, p, 0, None), lib.tpr_last_error())]
        for rc, msg in results:
            assert rc < 0 and b"tpr_init" in msg, msg
        q = np.zeros((2, 5, 3))
        for robot in _robots():
            with pytest.raises(_capi.ToppraHipError):
                robot.joint_wrenches(q, q, q, JointSections([0]))
            with pytest.raises(_capi.ToppraHipError):
                robot.joint_wrench_terms(q, q, q, JointSections([0, -1]))

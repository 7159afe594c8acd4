"""The joint-wrench kernels on the MI355X: the single and the fused entry against the numpy reference (tests/joint_load_ref.py)
within the accuracy bound of tests/joint_load_cases.py on every chain dof and every tree shape, the fused outputs against the
single entry bit for bit, the exact zeros, a section alone against the same section in its set, subtree independence, a chain
against the tree of its links, the joint identity against the tree kernels' inverse dynamics, the joint-0 identity against the
base reaction, the calling conventions, ``BatchJointLoadConstraint`` (boxes and ``bearing``) against the same limit fed through the
batched callback route, the constraint beside a torque limit on the same robot, the reference's fixtures, and the C entries'
refusals.

Accuracy (the bound is 16 x the float64 reference's own error against np.longdouble, per case and quantity;
profiles/joint_load_accuracy.json holds the yardsticks, the bounds, the CPU restatement's fractions and the measured ones):
measured on the MI355X the kernels use at most 0.55 of a bound over the 16 cases (wb of the 32-dof chain; 0.42 and 0.37 at 17
and 9 dof, every other quantity at most 0.35 -- the CPU restatement's figures to two digits), and at most 0.31 of the stored
bound on the reference's fixtures, whose sd they reproduce to 3.5e-15 / 1.9e-16 (tolerances 1.0e-9 / 6.7e-11)."""
import ctypes

import numpy as np
import pytest

from tests import base_wrench_ref as bwr, chain_cases as cc, chain_ref, joint_load_cases as jc, joint_load_ref as jr
from tests import rigid_support as rs, second_order_ref as sor, tree_cases as tc, tree_ref
from tests.helpers import golden

pytestmark = pytest.mark.gpu
FIXTURES = ("joint_load_torso_d15_N30", "joint_load_d4_N30_colloc")
NAMES = ("w0", "wa", "wb")
GRAVITY = np.array([0.0, 0.0, -9.81])
BADARG, UNSUPPORTED = -1, -3


def _terms(model, key, q, qs, qss):
    return jc.by_sets(key, lambda sec: tuple(model.joint_wrench_terms(q, qs, qss, jr.joint_sections_of(sec))))


def _single(model, key, q, qd, qdd):
    return jc.by_sets(key, lambda sec: model.joint_wrenches(q, qd, qdd, jr.joint_sections_of(sec)))


@pytest.mark.parametrize("key", jc.CASES)
def test_kernels_against_the_numpy_reference(gpu, key):
    """(1) Both entries, from numpy arrays; each fused output equals the single evaluation on the same arguments in every bit; no
    negative zero; without gravity w0 is +0; the trajectory that stands still has wa == w0."""
    robot, q, qs, qss = jc.case(key)
    model = bwr.robot_of(robot)
    S = len(jc.sections(key)["link"])
    w0, wa, wb = _terms(model, key, q, qs, qss)
    single = _single(model, key, q, qs, qss)
    assert w0.shape == wa.shape == wb.shape == single.shape == q.shape[:2] + (S, 6)
    rs.check(jc, key, {"w0": w0, "wa": wa, "wb": wb, "wrench": single}, label="%s")
    zero = np.zeros_like(q)
    assert np.array_equal(w0, _single(model, key, q, zero, zero)) and np.array_equal(wa, _single(model, key, q, zero, qs))
    assert np.array_equal(wb, single)
    for v in (w0, wa, wb):  # a zero leaves as +0, so equal values are equal bits
        assert not np.signbit(v[v == 0]).any()
    assert np.array_equal(wa[jc.still(key)], w0[jc.still(key)])
    if not robot["gravity"].any():
        assert not w0.any() and not np.signbit(w0).any()


@pytest.mark.parametrize("key", (3, 17, "nested", "torso", "y18", "comb32"))
def test_a_section_alone_and_a_permuted_set(gpu, key):
    """(2) A section's output from a set of one equals its output from the full set, bit for bit; a permuted set gives permuted
    outputs."""
    robot, q, qs, qss = jc.case(key)
    model, sec = bwr.robot_of(robot), jc.sections(key)
    idx = np.array(jc.section_sets(key)[0])
    full = model.joint_wrench_terms(q, qs, qss, jr.joint_sections_of(jr.subset(sec, idx)))
    single = model.joint_wrenches(q, qs, qss, jr.joint_sections_of(jr.subset(sec, idx)))
    for k in range(len(idx)):
        one = jr.joint_sections_of(jr.subset(sec, idx[k:k + 1]))
        for a, b in zip(model.joint_wrench_terms(q, qs, qss, one), full):
            assert np.array_equal(a[..., 0, :], b[..., k, :]), (key, k)
        assert np.array_equal(model.joint_wrenches(q, qs, qss, one)[..., 0, :], single[..., k, :])
    perm = np.random.default_rng(11).permutation(len(idx))
    for a, b in zip(model.joint_wrench_terms(q, qs, qss, jr.joint_sections_of(jr.subset(sec, idx[perm]))), full):
        assert np.array_equal(a, b[..., perm, :])


def _subtree(parents, link):
    return [i for i in range(len(parents)) if link in tc.path_to(parents, i)]


@pytest.mark.parametrize("key", ("vee", "nested", "comb32"))
def test_links_outside_a_section_s_subtree_do_not_reach_it(gpu, key):
    """(3) Changing the masses, centres of mass and inertias of every link outside a section's subtree leaves that section's bits
    unchanged: no sibling's wrench leaks through a bank."""
    robot, q, qs, qss = jc.case(key)
    parents, sec = bwr.parents_of(robot), jc.sections(key)
    rng = np.random.default_rng(21)
    for idx in jc.section_sets(key):
        part = jr.subset(sec, idx)
        base = bwr.robot_of(robot).joint_wrench_terms(q, qs, qss, jr.joint_sections_of(part))
        for k, link in enumerate(part["link"].tolist()):
            inside = _subtree(parents, link)
            outside = [i for i in range(len(parents)) if i not in inside]
            if not outside:
                continue
            other = {n: np.array(v) for n, v in robot.items()}
            other["mass"][outside] = rng.uniform(0.5, 3.0, len(outside))
            other["com"][outside] = rng.uniform(-0.2, 0.2, (len(outside), 3))
            other["inertia"][outside, :3] *= rng.uniform(1.5, 2.0, (len(outside), 3))
            got = bwr.robot_of(other).joint_wrench_terms(q, qs, qss, jr.joint_sections_of(part))
            for a, b in zip(got, base):
                assert np.array_equal(a[..., k, :], b[..., k, :]), (key, link)
            if link != 0 and parents[link] >= 0:  # (... and the change is seen where it should be: at a section below it)
                below = [j for j, l in enumerate(part["link"].tolist()) if l not in inside and set(_subtree(parents, l)) & set(outside)]
                for j in below[:1]:
                    assert not np.array_equal(got[2][..., j, :], base[2][..., j, :])


@pytest.mark.parametrize("d", jc.DOFS)
def test_a_chain_and_the_tree_of_its_links_are_bit_equal(gpu, d):
    """(4) SerialChain and KinematicTree.from_chain(chain): one kernel, one parent table."""
    from toppra_amd.chain import KinematicTree
    chain, q, qs, qss = jc.case(d)
    sc, sec = chain_ref.serial_chain(chain), jr.joint_sections_of(jc.sections(d))
    tree = KinematicTree.from_chain(sc)
    for a, b in zip(sc.joint_wrench_terms(q, qs, qss, sec), tree.joint_wrench_terms(q, qs, qss, sec)):
        assert np.array_equal(a, b)
    assert np.array_equal(sc.joint_wrenches(q, qs, qss, sec), tree.joint_wrenches(q, qs, qss, sec))


def _default_wrenches(robot, model, q, qs, qss, dtype=None, absolute=False):
    """Default sections on every joint, [..., d, 6]: from the GPU (two or more sets above 8 joints), or from the reference."""
    d = q.shape[-1]
    if dtype is None:
        from toppra_amd.chain import JointSections
        return np.concatenate([model.joint_wrenches(q, qs, qss, JointSections(list(range(at, min(at + 8, d)))))
                               for at in range(0, d, 8)], -2)
    return jr.joint_wrenches(robot, q, qs, qss, jr.default_sections(range(d)), dtype=dtype, absolute=absolute)


@pytest.mark.parametrize("key", (7, 9, 32, "vee", "nested", "torso", "y18", "comb32"))
def test_the_joint_identity_against_the_tree_kernels(gpu, key):
    """(5) With default sections on every joint, axis . n (revolute) / axis . f (prismatic) computed on the host matches the tree
    kernel's inverse dynamics.  The allowance is the sum of the two quantities' bounds, each on its own all-absolute magnitude."""
    from toppra_amd.chain import KinematicTree
    robot, q, qs, qss = jc.case(key)
    model = bwr.robot_of(robot)
    tree = model if "parent" in robot else KinematicTree.from_chain(model)
    w = _default_wrenches(robot, model, q, qs, qss)
    ref = _default_wrenches(robot, model, q, qs, qss, dtype=np.float64)
    mag = _default_wrenches(robot, model, q, qs, qss, dtype=np.float64, absolute=True)
    b_w = jc.BOUND_FACTOR * cc._own_error(ref, _default_wrenches(robot, model, q, qs, qss, dtype=np.longdouble), mag)
    prismatic = np.asarray(robot["joint_type"]) == 1
    axis = np.abs(np.asarray(robot["axis"]))
    part = lambda x: np.where(prismatic[:, None], x[..., :3], x[..., 3:])  # noqa: E731
    proj = np.einsum("...dk,dk->...d", part(w), np.asarray(robot["axis"]))
    tau = tree.inverse_dynamics(q, qs, qss)
    tref = (tc if isinstance(key, str) else cc)
    allow = b_w * np.einsum("...dk,dk->...d", part(mag), axis) + tref.bound(key, "wb") * tref.reference(key)["wb_mag"]
    off = np.abs(proj - tau)
    live = allow > 0
    assert np.array_equal(proj[~live], tau[~live])
    print("%s: |axis . w - tau| at most %.3g of its allowance" % (key, float(np.max(off[live] / allow[live])) if live.any() else 0.0))
    assert np.all(off[live] <= allow[live])


@pytest.mark.parametrize("key", (7, 32, "vee", "nested", "torso", "y18", "comb32"))
def test_joint_0_identity_against_the_base_reaction(gpu, key):
    """(6) On single-root cases the section at joint 0, carried to the base on the host (f_b = E_0 f, n_b = E_0 n + r_0 x f_b),
    matches base_wrench with the default mount, within the sum of bounds."""
    from tests import base_wrench_ref
    from toppra_amd.chain import JointSections
    robot, q, qs, qss = jc.case(key)
    assert bwr.parents_of(robot).count(-1) == 1
    model = bwr.robot_of(robot)
    sec0 = jr.default_sections([0])
    w = model.joint_wrenches(q, qs, qss, JointSections([0]))[..., 0, :]
    ref = jr.joint_wrenches(robot, q, qs, qss, sec0)[..., 0, :]
    mag = jr.joint_wrenches(robot, q, qs, qss, sec0, absolute=True)[..., 0, :]
    b_w = jc.BOUND_FACTOR * cc._own_error(ref, jr.joint_wrenches(robot, q, qs, qss, sec0, dtype=np.longdouble)[..., 0, :], mag)
    rot, k, trans = np.asarray(robot["rot"][0]), np.asarray(robot["axis"][0]), np.asarray(robot["trans"][0])
    if int(robot["joint_type"][0]) == 1:
        E = np.broadcast_to(rot, q.shape[:-1] + (3, 3))
        r = trans + q[..., :1] * (rot @ k)
    else:
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        s, c = np.sin(q[..., 0])[..., None, None], np.cos(q[..., 0])[..., None, None]
        E = rot @ (c * np.eye(3) + s * K + (1 - c) * np.outer(k, k))
        r = np.broadcast_to(trans, q.shape[:-1] + (3,))
    fb = np.einsum("...rc,...c->...r", E, w[..., :3])
    nb = np.einsum("...rc,...c->...r", E, w[..., 3:]) + np.cross(r, fb)
    aE = np.abs(E)
    fb_mag = np.einsum("...rc,...c->...r", aE, mag[..., :3])
    nb_mag = np.einsum("...rc,...c->...r", aE, mag[..., 3:]) + np.stack(
        [np.abs(r[..., 1]) * fb_mag[..., 2] + np.abs(r[..., 2]) * fb_mag[..., 1], np.abs(r[..., 2]) * fb_mag[..., 0] + np.abs(r[..., 0]) * fb_mag[..., 2],
         np.abs(r[..., 0]) * fb_mag[..., 1] + np.abs(r[..., 1]) * fb_mag[..., 0]], -1)
    base = model.base_wrench(q, qs, qss)
    bmag = base_wrench_ref.base_wrench(robot, q, qs, qss, absolute=True)
    bref = base_wrench_ref.base_wrench(robot, q, qs, qss)
    b_b = jc.BOUND_FACTOR * cc._own_error(bref, base_wrench_ref.base_wrench(robot, q, qs, qss, dtype=np.longdouble), bmag)
    # (the host's own carry adds a few roundings of the carried magnitudes: 8 eps covers the 3-term dot products and the cross)
    allow = (b_w + 8 * np.finfo(float).eps) * np.concatenate((fb_mag, nb_mag), -1) + b_b * bmag
    off = np.abs(np.concatenate((fb, nb), -1) - base)
    live = allow > 0
    assert np.array_equal(off[~live], np.zeros_like(off[~live]))
    print("%s: |carried section 0 - base reaction| at most %.3g of its allowance" % (key, float(np.max(off[live] / allow[live])) if live.any() else 0.0))
    assert np.all(off[live] <= allow[live])


@pytest.mark.parametrize("key", (1, 7, 32, "nested", "comb32"))
def test_device_tensors_and_views_give_the_host_call_s_bits(gpu, key):
    """(7) torch tensors on the device, contiguous and as a non-contiguous view, a flattened shape, a single point."""
    torch, dev = rs.torch_device()
    robot, q, qs, qss = jc.case(key)
    d = q.shape[-1]
    model = bwr.robot_of(robot)
    sec = jr.joint_sections_of(jr.subset(jc.sections(key), jc.section_sets(key)[0]))
    S = sec.count
    host = model.joint_wrench_terms(q, qs, qss, sec)
    tq, tqs, tqss = (torch.from_numpy(np.array(v)).to(dev) for v in (q, qs, qss))
    for got, want in zip(model.joint_wrench_terms(tq, tqs, tqss, sec), host):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    wide = [torch.repeat_interleave(t, 2, dim=1) for t in (tq, tqs, tqss)]
    views = [w[:, ::2] for w in wide]
    assert not views[0].is_contiguous()
    assert np.array_equal(model.joint_wrenches(*views, sec).cpu().numpy(), host[2])
    for got, want in zip(model.joint_wrench_terms(*views, sec), host):
        assert np.array_equal(got.cpu().numpy(), want)
    flat = model.joint_wrenches(tq.reshape(-1, d), tqs.reshape(-1, d), tqss.reshape(-1, d), sec)
    assert tuple(flat.shape) == (q.shape[0] * q.shape[1], S, 6) and np.array_equal(flat.cpu().numpy(), host[2].reshape(-1, S, 6))
    assert np.array_equal(model.joint_wrenches(q[1, 3], qs[1, 3], qss[1, 3], sec), host[2][1, 3])
    one = model.joint_wrench_terms(q[1, 3], qs[1, 3], qss[1, 3], sec)
    assert all(np.array_equal(one[k], host[k][1, 3]) for k in range(3))


# ---- the constraint ---------------------------------------------------------------------------------------------------------

def _robot(kind):
    """A robot dict under gravity along -z with its sections: the 7-dof chain (joint 1 and the last link), or the torso with two
    7-dof arms (the first joint of each arm)."""
    from toppra_amd.chain import JointSections
    base = dict(cc.case(7)[0] if kind == "chain" else tc.case("torso")[0], gravity=GRAVITY)
    model = bwr.robot_of(base)
    sections = JointSections.on_axes(model, [1, -1] if kind == "chain" else [1, 8], [0.05, -0.03])
    sec = {"link": sections.on(model), "rot": sections.rotations, "origin": sections.origins}
    return base, model, sections, sec


def _peak(robot, sec, args):
    """Per section and component [S, 6], the largest of |w0|, |wa|, |wb| over the problem's gridpoints, from the CPU reference:
    limits above it hold at rest (F w0 < g) with room, so every trajectory is feasible."""
    q, qs, qss = sor.path_samples(*args[:3])
    return np.max([np.abs(jr.joint_wrenches(robot, *a, sections=sec)).max((0, 1)) for a in list(jc.evaluations(q, qs, qss).values())[:3]], 0)


def _compare(source, data, args, ours, F, g, DT):
    """The constraint against BatchSecondOrderConstraint(robot.joint_wrenches flattened, F, g): rows and all five passes."""
    robot, sections = ours.robot, ours.sections

    def inv_dyn(q, qd, qdd):
        w = robot.joint_wrenches(q, qd, qdd, sections)
        return w.reshape(tuple(w.shape[:-2]) + (6 * sections.count,))

    return rs.compare(source, data, args, ours, inv_dyn, F, g, DT)


def _box_rows(S):
    I3 = np.eye(3)
    F = np.zeros((12 * S, 6 * S))
    for k in range(S):
        for j, at in enumerate((0, 3)):
            r, c = 12 * k + 6 * j, 6 * k + at
            F[r:r + 3, c:c + 3], F[r + 3:r + 6, c:c + 3] = I3, -I3
    return F


@pytest.mark.parametrize("scheme", ["Collocation", "Interpolation"])
@pytest.mark.parametrize("source", ["spline", "samples"])
@pytest.mark.parametrize("kind,per_traj", [("chain", False), ("tree", True)])
def test_the_constraint_equals_the_callback_route(gpu, scheme, source, kind, per_traj):
    """(8) Force and moment boxes with g from the CPU reference's peaks, shared or per trajectory."""
    from toppra_amd import constraint
    robot, model, sections, sec = _robot(kind)
    d, S = len(robot["mass"]), sections.count
    data, args = rs.problem(d)
    peak = _peak(robot, sec, args)
    hi = 1.5 * peak[:, :3] * (1.0 + np.random.default_rng(9).random((cc.B, S, 3) if per_traj else (S, 3)))
    force, moment = np.stack([-1.25 * hi, hi], -1), 2.0 * peak[:, 3:].max(-1)
    g = np.concatenate((force[..., 1], -force[..., 0], np.broadcast_to(moment[:, None], force.shape[:-2] + (6,))), -1)
    g = g.reshape(g.shape[:-2] + (12 * S,))
    DT = getattr(constraint.DiscretizationType, scheme)
    ours = constraint.BatchJointLoadConstraint(model, sections, force=force, moment=moment, discretization_scheme=DT)
    F = _box_rows(S)
    assert np.array_equal(ours.F, F) and np.array_equal(ours.g, g)
    out = _compare(source, data, args, ours, F, g, DT)
    assert out["rows"][0].shape[-1] == 2 + 4 * d + (2 if scheme == "Interpolation" else 1) * 12 * S


@pytest.mark.parametrize("kind,source,scheme", [("chain", "samples", "Interpolation"), ("tree", "spline", "Collocation")])
def test_the_bearing_rows_equal_the_callback_route(gpu, kind, source, scheme):
    """(8) bearing(): tilting, axial and radial limits per section from the CPU reference's peaks (a circle of the radius of the
    largest component pair times sqrt 2 holds every point; the inscribed polygon needs 1 / cos(pi / sides) more)."""
    from toppra_amd import constraint
    robot, model, sections, sec = _robot(kind)
    d, S = len(robot["mass"]), sections.count
    data, args = rs.problem(d, seed=6)
    peak = _peak(robot, sec, args)
    sides = 6
    room = 1.5 * np.sqrt(2.0) / np.cos(np.pi / sides)
    tilting, radial, axial = room * peak[:, 3:5].max(-1), room * peak[:, 0:2].max(-1), 1.5 * peak[:, 2]
    DT = getattr(constraint.DiscretizationType, scheme)
    F, g = constraint.BatchJointLoadConstraint.bearing_rows(S, tilting, axial, radial, sides)
    assert F.shape == (S * (2 * sides + 2), 6 * S)
    ours = constraint.BatchJointLoadConstraint.bearing(model, sections, tilting=tilting, axial=axial, radial=radial, sides=sides,
                                                       discretization_scheme=DT)
    assert np.array_equal(ours.F, F) and np.array_equal(ours.g, g)
    _compare(source, data, args, ours, F, g, DT)


def test_beside_a_torque_constraint_on_the_same_robot(gpu):
    """(9) [torque on the torso's 15 joints, a moment box on two sections] under Interpolation: 2 + 60 + 30 + 24 = 116 rows per
    stage, within the 122; every pass runs, the rows are finite, every trajectory is feasible; the load block is the last one."""
    from toppra_amd import algorithm, batch, constraint
    robot, model, sections, sec = _robot("tree")
    d = len(robot["mass"])
    data, args = rs.problem(d, seed=8)
    pe = batch.path_eval_batch(*args[:3])
    taumax = np.abs(model.torque_terms(pe["q"], pe["qs"], pe["qss"])[0]).max() + 20.0
    peak = _peak(robot, sec, args)
    cons = [constraint.BatchJointTorqueConstraint(model, np.tile([-taumax, taumax], (d, 1)), np.zeros(d)),
            constraint.BatchJointLoadConstraint(model, sections, moment=1.5 * peak[:, 3:].max(-1))]
    inst = algorithm.BatchTOPPRA(*args, constraints=cons)
    out = rs.run_passes(inst)
    assert out["rows"][0].shape[-1] == 2 + 4 * d + 2 * d + 24 == 116 <= 122
    rs.passes_ran(out)
    alone = algorithm.BatchTOPPRA(*args, constraints=[cons[1]]).dense_rows()
    for k in range(3):
        assert np.array_equal(out["rows"][k][..., -24:], alone[k][..., -24:])


@pytest.mark.parametrize("name", FIXTURES)
def test_against_the_reference_s_fixtures(gpu, name):
    """(10) w0 / wa / wb within the stored accuracy bound, return codes equal, sd within the stored end-to-end tolerance
    (tools/make_joint_load_golden.py)."""
    from toppra_amd import constraint
    fx = golden(name)
    robot = rs.fixture_tree(fx)
    sec = {"link": fx["section_link"], "rot": fx["section_rot"], "origin": fx["section_origin"]}
    model, sections = tree_ref.kinematic_tree(robot), jr.joint_sections_of(sec)
    S = sections.count
    q, qs, qss = sor.path_samples(fx["coef"], fx["breaks"], fx["grid"])
    ev = jc.evaluations(q, qs, qss)
    got = dict(zip(NAMES, model.joint_wrench_terms(q, qs, qss, sections)))
    rs.fixture_accuracy(name, fx, got, {k: jr.joint_wrenches(robot, *ev[k], sections=sec, absolute=True) for k in NAMES})
    interp, DT = rs.fixture_scheme(fx)
    if "sides" in fx:
        con = constraint.BatchJointLoadConstraint.bearing(model, sections, tilting=fx["tilting"], axial=fx["axial"], radial=fx["radial"],
                                                          sides=int(fx["sides"]), discretization_scheme=DT)
        assert np.array_equal(con.F, fx["F"]) and np.array_equal(np.broadcast_to(con.g, fx["g"].shape), fx["g"])
    else:
        con = constraint.BatchJointLoadConstraint(model, sections, force=fx["force"], moment=fx["moment"], discretization_scheme=DT)
        assert np.array_equal(con.F, fx["F"]) and np.array_equal(con.g, fx["g"])
    rs.fixture_solve(name, fx, con, interp)


# ---- the entries' refusals --------------------------------------------------------------------------------------------------

def test_entries_refuse_bad_arguments_before_any_launch(gpu):
    """(11) In their order -- the links as a chain, the parent table, the fork count, the sections, the pointers; the terms entry
    B / N first -- each before anything is launched: the buffers handed over with the refused calls are a few doubles long."""
    from toppra_amd import _capi
    from toppra_amd.chain import JointSections
    lib = _capi.load()
    sc = chain_ref.serial_chain(cc.case(3)[0])
    buf = np.zeros(64)
    p = buf.ctypes.data
    model, keep = sc.c_struct(buf)
    m = ctypes.byref(model)
    table = np.array([-1, 0, 1], dtype=np.int32)

    def make(**change):
        sec = JointSections([0, 2], origins=[[0.1, 0, 0], [0, 0.2, 0]]).c_struct(sc)
        for field, v in change.items():
            if field == "count":
                sec.count = v
            elif field == "link":
                sec.link[v[0]] = v[1]
            else:
                getattr(sec, field)[v[0]][v[1]] = v[2]
        return sec

    good = make()

    def calls(chain=m, parent=table, sections=good, B=2, N=1, q=p, out=p):
        t = None if parent is None else parent.ctypes.data
        f = None if sections is None else ctypes.byref(sections)
        single = lib.tpr_tree_joint_wrench_batch(chain, t, f, B * (N + 1), q, p, p, out, 0, None), lib.tpr_last_error()
        terms = lib.tpr_tree_joint_wrench_terms_batch(chain, t, f, B, N, q, p, p, out, out, out, 0, None), lib.tpr_last_error()
        return single, terms

    def refused(result, code, text):
        for rc, msg in result:
            assert rc == code and text in msg, (rc, msg)

    nan_sec = make(origin=(1, 1, np.nan))
    # the order: each call is bad in the named way AND in every way that is checked later
    refused(calls(chain=None, parent=None, sections=nan_sec, q=None), BADARG, b"null chain")
    wrong = np.array([-1, 0, 2], dtype=np.int32)
    refused(calls(parent=wrong, sections=nan_sec, q=None), BADARG, b"the parent of link 2 is 2, outside -1 .. 1")
    refused(calls(parent=None, sections=nan_sec, q=None), BADARG, b"null parent")
    sc11 = chain_ref.serial_chain(chain_ref.random_chain(11, 5))
    model11, keep11 = sc11.c_struct(buf)
    five = np.array([-1, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4], dtype=np.int32)
    refused(calls(chain=ctypes.byref(model11), parent=five, sections=nan_sec, q=None), UNSUPPORTED, b"the tree has 5 forks")
    refused(calls(sections=None, q=None), BADARG, b"null sections")
    refused(calls(sections=nan_sec, q=None), BADARG, b"every entry of the sections must be finite")
    refused(calls(q=None), BADARG, b"are required")
    refused(calls(out=None), BADARG, b"are required")
    # the sections' own refusals, in their order: the count, the links, finiteness, the frames
    refused(calls(sections=make(count=0, link=(0, 5))), BADARG, b"the section count must be in")
    refused(calls(sections=make(count=9)), BADARG, b"the section count must be in")
    refused(calls(sections=make(link=(1, 3), rot=(0, 0, np.nan))), BADARG, b"a section's link is outside the robot")
    refused(calls(sections=make(link=(0, -1))), BADARG, b"a section's link is outside the robot")
    for field, size in (("rot", 9), ("origin", 3)):
        for k in (0, 1):
            for j in (0, size - 1):
                for bad in (np.nan, np.inf):
                    refused(calls(sections=make(**{field: (k, j, bad)})), BADARG, b"finite")
    refused(calls(sections=make(rot=(0, 0, 1.001))), BADARG, b"orthonormal")
    refused(calls(sections=make(rot=(1, 8, -1.0))), BADARG, b"orthonormal")  # (a reflection)
    refused(calls(sections=make(rot=(1, 1, 1e-9))), BADARG, b"orthonormal")
    # (entries past count are not read)
    past = make(count=1, link=(1, 77), rot=(1, 0, np.nan))
    assert all(rc == 0 for rc, _ in calls(sections=past))
    # sizes
    assert lib.tpr_tree_joint_wrench_terms_batch(None, None, None, -1, 1, p, p, p, p, p, p, 0, None) == BADARG and b"B >= 0" in lib.tpr_last_error()
    assert lib.tpr_tree_joint_wrench_terms_batch(m, table.ctypes.data, ctypes.byref(good), 1, -1, p, p, p, p, p, p, 0, None) == BADARG
    assert lib.tpr_tree_joint_wrench_batch(m, table.ctypes.data, ctypes.byref(good), -1, p, p, p, p, 0, None) == BADARG
    refused(calls(B=1 << 20, N=(1 << 11) - 1), UNSUPPORTED, b"2^31 - 1")
    bad_model, keep2 = sc.c_struct(buf)
    bad_model.d = 33
    refused(calls(chain=ctypes.byref(bad_model)), BADARG, b"dof must be in")
    assert lib.tpr_joint_sections_bytes() == ctypes.sizeof(_capi.tpr_joint_sections) == 40 + 96 * 8
    # ... and the valid call on the same model still runs
    z = np.zeros(3)
    w = np.zeros(12)
    zp = z.ctypes.data  # (the earlier valid calls wrote their outputs into buf)
    assert lib.tpr_tree_joint_wrench_batch(m, table.ctypes.data, ctypes.byref(good), 1, zp, zp, zp, w.ctypes.data, 0, None) == 0
    assert np.array_equal(w.reshape(2, 6), sc.joint_wrenches(z, z, z, JointSections([0, 2], origins=[[0.1, 0, 0], [0, 0.2, 0]])))
    assert np.isfinite(w).all()


def test_python_refuses_shape_errors_before_any_launch(gpu):
    from toppra_amd.chain import JointSections
    robot, q, qs, qss = jc.case("vee")
    model = bwr.robot_of(robot)
    sec = JointSections([0, -1])
    with pytest.raises(ValueError, match="dof"):
        model.joint_wrenches(q[..., :2], qs[..., :2], qss[..., :2], sec)
    with pytest.raises(ValueError, match="shape of q"):
        model.joint_wrench_terms(q, qs[:, :5], qss, sec)
    with pytest.raises(ValueError, match="JointSections"):
        model.joint_wrenches(q, qs, qss, jc.sections("vee"))
    with pytest.raises(ValueError, match="joints 0..2"):
        model.joint_wrenches(q, qs, qss, JointSections([5]))


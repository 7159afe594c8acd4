"""Effective mass and contact energy without a GPU: the numpy restatement of the kernel's walk (tests/effective_mass_ref.py)
against the dense route (mass matrix and solve) within cond2(M) 2^-52, closed forms on one-link robots, the Cauchy-Schwarz bound
s2^2 <= g q'' M q' that makes the total kinetic energy this quantity's upper envelope, the point sets of
tests/effective_mass_cases.py, and the surface of ``toppra_amd.contact`` / ``BatchContactEnergyConstraint``: the header's entry
bound with its declared argument count, signatures, shapes, units and every refusal before anything is launched (this machine has
no GPU: a launch would raise ToppraHipError instead of the expected error)."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import chain_ref, effective_mass_cases as ec, effective_mass_ref as er, tree_cases as tc, tree_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


# ---- the restatement against the dense route -----------------------------------------------------------------------------------

FLOOR = 64  # ulp: see test_the_walk_is_the_dense_route


@pytest.mark.parametrize("key", ec.CASES)
def test_the_walk_is_the_dense_route(key):
    """Per gridpoint and point, |walk - dense| / dense <= (cond2(M) + FLOOR) 2^-52 for the mobility, in both modes; the squared
    speeds, which no solve touches, agree to FLOOR ulp of their all-absolute magnitude.

    cond2(M) 2^-52 is what the solve costs.  Alone it cannot hold on the smallest robots: at 1 dof cond2(M) = 1, one ulp, while
    each route rounds some tens of times before any solve (tau = J' f cancels like any cross product) -- against the longdouble
    walk the float64 walk is off by up to 18 ulp and the dense route by up to 90 ulp on these cases, whatever cond2(M) is.  FLOOR
    covers that rounding; from 3 dof on (cond2(M) >= 500) it is noise beside the conditioning term, which is asserted alone
    there; the test prints the fractions (they depend on the host's libm and BLAS)."""
    robot, q, qs = ec.case(key)
    links, offsets = ec.point_set(key, "set")
    cond = np.linalg.cond(er.mass_matrix(robot, q))
    rng = np.random.default_rng(3)
    u = rng.standard_normal((len(links), 3))
    u /= np.sqrt((u * u).sum(-1, keepdims=True))
    worst = alone = 0.0
    # the squared speeds' scale: |J| |q'| squared, nothing cancelling
    mag = ((np.abs(er.jacobians(robot, links, offsets, q)[0]) @ np.abs(qs)[..., None, :, None])[..., 0] ** 2).sum(-1)
    for directions in (None, u):
        s2, g = er.walk(robot, links, offsets, q, qs, directions)
        ds2, dg = er.dense(robot, links, offsets, q, qs, directions)
        live = dg != 0
        c = np.broadcast_to(cond[..., None], g.shape)[live]
        rel = np.abs(g - dg)[live] / np.abs(dg)[live]
        worst, alone = max(worst, float((rel / (c + FLOOR)).max()) / EPS), max(alone, float((rel / c).max()) / EPS)
        assert np.all(rel <= (c + FLOOR) * EPS), (key, float((rel / (c + FLOOR)).max()) / EPS)
        assert np.array_equal(g[~live], np.zeros((~live).sum()))
        assert np.all(np.abs(s2 - ds2) <= FLOOR * EPS * mag)
        assert np.all(g >= 0) and np.all(s2 >= 0)
    print("%s: |walk - dense| / dense at most %.3g of (cond2(M) + %d) 2^-52, %.3g of cond2(M) 2^-52 alone (cond up to %.3g)"
          % (key, worst, FLOOR, alone, float(cond.max())))
    if len(robot["mass"]) >= 3:
        assert alone <= 1.0, (key, alone)  # the conditioning term alone, where it is more than the routes' own rounding


def test_the_longdouble_walk_is_closer_than_the_bound():
    for key in (7, "torso"):
        ref = ec.reference(key)
        for name, yard in ref["yardstick"].items():
            assert 0 < yard < 1e-10 and ec.bound(key, name) == ec.BOUND_FACTOR * yard


def test_a_chain_is_the_tree_of_its_links():
    robot, q, qs = ec.case(7)
    links, offsets = ec.point_set(7, "set")
    as_tree = dict(robot, parent=np.arange(7) - 1)
    for a, b in zip(er.walk(robot, links, offsets, q, qs), er.walk(as_tree, links, offsets, q, qs)):
        assert np.array_equal(a, b)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------

def _one_link(joint, axis=(0.0, 0.0, 1.0)):
    chain = chain_ref.random_chain(1, 11, massless=None, prismatic_every=0)
    chain["joint_type"] = np.array([1 if joint == "prismatic" else 0], dtype=np.int32)
    chain["axis"] = np.array([axis], dtype=np.float64)
    return chain


def test_one_revolute_link():
    """m_R = I_axis / r_perp^2: I_axis the link's inertia about the joint axis, r_perp the point's distance from it."""
    chain = _one_link("revolute")
    z, c, m = chain["axis"][0], chain["com"][0], chain["mass"][0]
    I = chain["inertia"][0]
    Ic = np.array([[I[0], I[3], I[4]], [I[3], I[1], I[5]], [I[4], I[5], I[2]]])
    I_axis = z @ Ic @ z + m * (c @ c - (c @ z) ** 2)
    q, qs = np.array([[0.3], [-1.2]]), np.array([[0.7], [2.0]])
    offsets = np.array([[0.2, -0.1, 0.4], [0.0, 0.3, 0.0]])
    s2, g = er.walk(chain, [0, 0], offsets, q, qs)
    r2 = (offsets ** 2).sum(-1) - (offsets @ z) ** 2
    assert np.allclose(s2 / g, I_axis / r2, rtol=1e-13, atol=0)
    assert np.allclose(s2, qs ** 2 * r2, rtol=1e-13, atol=0)


def test_one_prismatic_link():
    """m_R = m along the axis; a direction perpendicular to the axis meets no mobility at all: g = 0."""
    chain = _one_link("prismatic")
    q, qs = np.array([[0.3], [-1.2]]), np.array([[0.7], [2.0]])
    offsets = np.array([[0.2, -0.1, 0.4]])
    s2, g = er.walk(chain, [0], offsets, q, qs)
    assert np.allclose(s2 / g, chain["mass"][0], rtol=1e-14, atol=0) and np.allclose(s2[..., 0], qs[..., 0] ** 2, rtol=1e-15)
    s2p, gp = er.walk(chain, [0], offsets, q, qs, directions=np.array([[1.0, 0.0, 0.0]]))
    assert np.array_equal(gp, np.zeros_like(gp)) and np.array_equal(s2p, np.zeros_like(s2p))
    _, ga = er.walk(chain, [0], offsets, q, None, directions=np.array([[0.0, 0.0, 1.0]]))
    assert np.allclose(1.0 / ga, chain["mass"][0], rtol=1e-14, atol=0)
    _, dgp = er.dense(chain, [0], offsets, q, qs, directions=np.array([[1.0, 0.0, 0.0]]))
    assert np.all(np.abs(dgp) <= 1e-30)


@pytest.mark.parametrize("key", (1, 2, 7, "vee", "torso"))
def test_the_total_energy_is_the_upper_envelope(key):
    """Cauchy-Schwarz: s2^2 <= g * q'' M q', with equality to rounding at 1 dof."""
    robot, q, qs = ec.case(key)
    links, offsets = ec.point_set(key, "set")
    s2, g = er.walk(robot, links, offsets, q, qs)
    e2 = er.energy2(robot, q, qs)[..., None]
    live = s2 > 0
    ratio = (s2 * s2)[live] / np.broadcast_to(g * e2, s2.shape)[live]
    print("%s: s2^2 / (g q'Mq') in [%.6f, %.6f]" % (key, ratio.min(), ratio.max()))
    assert np.all(ratio <= 1.0 + 1e-12)
    if key == 1:
        assert np.all(np.abs(ratio - 1.0) <= 1e-13)
    else:
        assert ratio.min() < 0.999


def test_the_host_bound():
    s2 = np.array([[[4.0, 1.0], [0.0, 0.0], [0.0, 2.0]]])
    g = np.array([[[2.0, 0.5], [0.0, 0.0], [0.0, 1.0]]])
    lim = np.array([[[8.0, 0.5], [1.0, 0.0]]])
    got = er.xbound(s2, g, lim)
    assert np.array_equal(got, [[[0.0, 0.5], [0.0, np.inf], [0.0, 0.25]]])
    assert np.array_equal(er.xbound(s2, g, lim, directed=True)[0, :, 1], [0.5, np.inf, 0.5])


# ---- the point sets ----------------------------------------------------------------------------------------------------------------

def test_the_point_sets_are_what_the_cases_say():
    for key in ec.CASES:
        robot = ec.case(key)[0]
        d = len(robot["mass"])
        assert np.all(robot["mass"] > 0), key  # no weightless link
        links, offsets = ec.point_set(key, "set")
        assert 4 <= len(links) <= 16 and offsets.shape == (len(links), 3)
        assert links[0] == d - 1 and 0 in links and links.count((d - 1) // 2) >= 2
        if isinstance(key, str):
            parents = tc.SHAPES[key]
            assert set(tc.leaves_of(parents)) <= set(links), key  # one point per branch
            if tc.forks_of(parents):
                assert tc.forks_of(parents)[0] in links, key  # one below a fork
        if key in ec.FULL:
            full = ec.point_set(key, "full")[0]
            assert len(full) == 16 and list(full) != sorted(full) or d == 1
    assert ec.sets_of(32) == ("set", "full") and ec.sets_of(2) == ("set",)
    assert len(set(ec.point_set("comb32", "full")[0])) >= 12


# ---- the surface ---------------------------------------------------------------------------------------------------------------------

def _robots():
    return (chain_ref.serial_chain(chain_ref.random_chain(3, 5, massless=None)),
            tree_ref.kinematic_tree(tree_ref.random_tree([-1, 0, 0], 5, massless=None)))


def _points():
    from toppra_amd.chain import ControlPoints
    return ControlPoints([1, -1], [[0.1, 0.0, 0.2], [0.0, 0.1, 0.1]])


def test_the_header_s_entry_is_exported_and_bound():
    """Every tpr_*( name of include/toppra_hip_contact.h is in contact.EXPORTS, exported by the library, and bound with the number
    of arguments the header declares; none of them is in the main header's table."""
    from toppra_amd import _capi, contact
    header = open(os.path.join(ROOT, "include", "toppra_hip_contact.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(tpr_\w+)\s*\(([^;]*)\)\s*;", code))
    assert tuple(declared) == contact.EXPORTS == ("tpr_tree_effective_mass_batch",)
    lib = contact.load()
    for name, args in declared.items():
        entry = getattr(lib, name)
        assert len(entry.argtypes) == len(args.split(",")) == 14 and entry.restype is not None
        assert name not in _capi.EXPORTS
    assert '#include "toppra_hip.h"' in header


def test_the_new_symbols_are_exported():
    import toppra_amd as ta
    from toppra_amd import batch, chain, constraint, contact
    for cls in (chain.SerialChain, chain.KinematicTree):
        assert hasattr(cls, "effective_mass") and hasattr(cls, "contact_energy")
    assert "effective_mass_batch" not in batch.__all__  # (the module of its own: batch's table is pinned)
    assert issubclass(constraint.BatchContactEnergyConstraint, constraint._BatchChainBound)
    assert ta.BatchContactEnergyConstraint is constraint.BatchContactEnergyConstraint and "BatchContactEnergyConstraint" in ta.__all__
    assert ta.contact is contact
    con = constraint.BatchContactEnergyConstraint(_robots()[0], _points(), 1.0)
    assert con.needs_q and con.first_order and con.source_count() == 1
    assert "give the path positions" in con.no_q


def test_signatures():
    from toppra_amd import chain, constraint, contact
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(contact.effective_mass_batch) == ["robot", "q", "qs", "points", "limit", "directions"]
    assert sig(contact.effective_mass_bound_batch) == ["robot", "q", "qs", "points", "limit"]
    assert sig(chain._Robot.effective_mass) == ["self", "q", "qd", "points", "directions"]
    assert sig(chain._Robot.contact_energy) == ["self", "q", "qd", "points", "body_mass"]
    assert sig(constraint.BatchContactEnergyConstraint.__init__) == ["self", "robot", "points", "energy", "body_mass"]
    assert sig(constraint.BatchContactEnergyConstraint.from_force) == ["robot", "points", "force", "stiffness", "body_mass"]
    defaults = inspect.signature(contact.effective_mass_batch).parameters
    assert defaults["limit"].default is None and defaults["directions"].default is None


def test_the_constraint_forms_what_the_kernel_reads():
    from toppra_amd import constraint
    sc, tree = _robots()
    pts = _points()
    for robot in (sc, tree):
        con = constraint.BatchContactEnergyConstraint(robot, pts, 0.5)
        assert np.array_equal(con.limit, [[1.0, 0.0], [1.0, 0.0]]) and con._limit_batch is None
        con = constraint.BatchContactEnergyConstraint(robot, pts, [0.5, 2.0], body_mass=[4.0, np.inf])
        assert np.array_equal(con.limit, [[1.0, 0.25], [4.0, 0.0]])
        con = constraint.BatchContactEnergyConstraint(robot, pts, np.array([[0.5, 2.0], [1.0, 3.0], [0.25, 0.125]]), body_mass=8.0)
        assert con.limit.shape == (3, 2, 2) and con._limit_batch == 3
        assert np.array_equal(con.limit[..., 0], [[1.0, 4.0], [2.0, 6.0], [0.5, 0.25]]) and np.all(con.limit[..., 1] == 0.125)
        con.check(3, 10, 3)
        with pytest.raises(ValueError, match="per trajectory for 3 trajectories, the problem has 4"):
            con.check(4, 10, 3)
        with pytest.raises(ValueError, match="Wrong dimension"):
            con.check(3, 10, 4)
        with pytest.raises(ValueError, match="give the path positions"):
            con.bound_sources(None, 3, 10, 3, np.zeros(1), q=None)


def test_the_constraint_s_refusals():
    from toppra_amd import constraint
    sc, _ = _robots()
    pts = _points()
    C = constraint.BatchContactEnergyConstraint
    for bad in (0.0, -1.0, np.nan, [1.0, 0.0], [[1.0, np.nan]]):
        with pytest.raises(ValueError, match="energy must be > 0"):
            C(sc, pts, bad)
    for bad in ([1.0, 2.0, 3.0], np.ones((2, 3)), np.ones((2, 2, 2))):
        with pytest.raises(ValueError, match=r"energy must be a scalar or have shape \[P\] or \[B, P\] with P = 2"):
            C(sc, pts, bad)
    for bad in (0.0, -2.0, np.nan, [1.0, 0.0]):
        with pytest.raises(ValueError, match="body_mass must be > 0"):
            C(sc, pts, 1.0, body_mass=bad)
    for bad in ([1.0, 2.0, 3.0], np.ones((2, 2))):
        with pytest.raises(ValueError, match=r"body_mass must be a scalar or have shape \[P\] = \[2\]"):
            C(sc, pts, 1.0, body_mass=bad)
    with pytest.raises(ValueError, match="robot must be a toppra_amd.chain.SerialChain or KinematicTree"):
        C("arm", pts, 1.0)
    with pytest.raises(ValueError, match="points must be a toppra_amd.chain.ControlPoints"):
        C(sc, [0, 1], 1.0)
    from toppra_amd.chain import ControlPoints
    with pytest.raises(ValueError, match="a control point sits on link 5"):
        C(sc, ControlPoints([5], [[0.0, 0.0, 0.0]]), 1.0)


def test_from_force():
    """E = F^2 / (2 k): 140 N on 75 N / mm is 0.1307 J."""
    from toppra_amd import constraint
    sc, _ = _robots()
    pts = _points()
    con = constraint.BatchContactEnergyConstraint.from_force(sc, pts, 140.0, 75e3, body_mass=[40.0, 0.6])
    assert np.allclose(con.energy, 140.0 ** 2 / (2 * 75e3), rtol=1e-15) and abs(float(con.energy) - 0.130667) < 1e-6
    assert np.array_equal(con.limit[:, 0], np.full(2, 2.0 * (140.0 * 140.0 / (2.0 * 75e3)))) and np.array_equal(con.limit[:, 1], [1 / 40.0, 1 / 0.6])
    con = constraint.BatchContactEnergyConstraint.from_force(sc, pts, [140.0, 65.0], [75e3, 10e3])
    assert np.allclose(con.limit[:, 0], [140.0 ** 2 / 75e3, 65.0 ** 2 / 10e3], rtol=1e-15)
    for F, k in ((0.0, 1.0), (1.0, 0.0), (np.nan, 1.0), (1.0, -3.0)):
        with pytest.raises(ValueError, match="force and stiffness must be > 0"):
            constraint.BatchContactEnergyConstraint.from_force(sc, pts, F, k)


def test_the_batch_functions_refusals():
    """Everything is refused before the device is looked for."""
    from toppra_amd import contact
    sc, tree = _robots()
    pts = _points()
    q = np.zeros((2, 5, 3))
    for robot in (sc, tree):
        with pytest.raises(ValueError, match="points must be a toppra_amd.chain.ControlPoints"):
            contact.effective_mass_batch(robot, q, q, None)
        with pytest.raises(ValueError, match=r"directions must have shape \[P, 3\] = \[2, 3\]"):
            contact.effective_mass_batch(robot, q, q, pts, directions=np.zeros((3, 3)))
        with pytest.raises(ValueError, match="directions holds a value that is not finite"):
            contact.effective_mass_batch(robot, q, q, pts, directions=[[1.0, 0.0, np.inf], [0.0, 1.0, 0.0]])
        with pytest.raises(ValueError, match="qs is required"):
            contact.effective_mass_batch(robot, q, None, pts)
        with pytest.raises(ValueError, match="qs is required"):
            contact.effective_mass_batch(robot, q, None, pts, limit=np.ones((2, 2)), directions=np.eye(3)[:2])
        with pytest.raises(ValueError, match=r"q must have shape \[\.\.\., d\] with d = 3"):
            contact.effective_mass_batch(robot, np.zeros((2, 5, 4)), np.zeros((2, 5, 4)), pts)
        with pytest.raises(ValueError, match="qs must have the shape of q"):
            contact.effective_mass_batch(robot, q, np.zeros((2, 4, 3)), pts)
        with pytest.raises(ValueError, match=r"with a limit, q must have shape \[B, N\+1, d\]"):
            contact.effective_mass_batch(robot, q[0], q[0], pts, limit=np.ones((2, 2)))
        with pytest.raises(ValueError, match=r"limit must have shape \[P, 2\] = \[2, 2\] or \[B, P, 2\] = \[2, 2, 2\]"):
            contact.effective_mass_batch(robot, q, q, pts, limit=np.ones((3, 2, 2)))
        for bad in ([[0.0, 1.0], [1.0, 1.0]], [[1.0, -1.0], [1.0, 1.0]], [[np.nan, 1.0], [1.0, 1.0]]):
            with pytest.raises(ValueError, match="limit must hold 2 E_max > 0 and 1 / m_body >= 0"):
                contact.effective_mass_bound_batch(robot, q, q, pts, bad)
        with pytest.raises(ValueError, match="the bound needs limit"):
            contact.effective_mass_bound_batch(robot, q, q, pts, None)
    with pytest.raises(ValueError, match="robot must be a toppra_amd.chain.SerialChain or KinematicTree"):
        contact.effective_mass_batch("arm", q, q, pts)
    assert np.array_equal(contact.inverse_body_mass(None, 3), np.zeros(3)) and np.array_equal(contact.inverse_body_mass([2.0, np.inf], 2), [0.5, 0.0])


def test_the_package_files_speak_of_the_project_alone():
    text = open(os.path.join(ROOT, "toppra_amd", "contact.py")).read()
    assert "ora" + "cle" not in text

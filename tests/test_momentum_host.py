"""Momentum and kinetic energy without a GPU: the numpy reference (tests/momentum_ref.py) against routes of its own -- the mass
matrix of tests/chain_ref.py, a moved mount origin, the link sets adding up --, the link sets of tests/momentum_cases.py, and the
surface of ``momentum_batch`` / ``BatchMomentumConstraint``: shapes, units, link-set parsing, and every refusal before anything
is launched (this machine has no GPU: a launch would raise ToppraHipError instead of the expected error)."""
import numpy as np
import pytest

from tests import base_wrench_ref as bwr, chain_cases as cc, chain_ref, momentum_cases as mc, momentum_ref as mr, tree_cases as tc, tree_ref


# ---- the reference against routes of its own ---------------------------------------------------------------------------------

@pytest.mark.parametrize("key", (3, "vee"))
def test_reference_energy_is_the_mass_matrix_s(key):
    """energy2 = qs' M(q) qs with M from columns of the inverse dynamics: each side within 16 x its own error against
    np.longdouble (the composed float64 tolerance)."""
    robot, q, qs, _ = mc.case(key)
    ref = mc.reference(key)
    route = lambda dtype: np.einsum("...i,...ij,...j->...", qs.astype(dtype), chain_ref.mass_matrix(robot, q, dtype), qs.astype(dtype))  # noqa: E731
    got, exact = route(np.float64), route(np.longdouble)
    allow = mc.bound(key, "energy2") * ref["energy2_mag"] + mc.BOUND_FACTOR * np.abs(got - exact)
    assert mc.bound(key, "energy2") > 0 and np.any(np.abs(got - exact) > 0)
    err = np.abs(ref["energy2"] - got)
    print("%s: |energy2 - qs' M qs| at most %.3g of its allowance" % (key, float(np.max(err[allow > 0] / allow[allow > 0]))))
    assert np.all(err <= allow), key
    assert np.all(ref["energy2"][mc.still(key)] == 0.0) and np.all(ref["energy2"][0] > 0.0)


@pytest.mark.parametrize("key", (7, "skip", "roots"))
def test_reference_moving_the_mount_origin(key):
    """The angular momentum about a point moved by delta changes by -delta x P; the linear momentum and the energy do not."""
    robot, q, qs, _ = mc.case(key)
    delta = np.array([0.25, -0.4, 0.15])
    here, there = dict(mr.NO_MOUNT), dict(mr.NO_MOUNT, origin=delta)
    a, b = mr.momentum(robot, q, qs, here), mr.momentum(robot, q, qs, there)
    mag_a, mag_b = mr.momentum(robot, q, qs, here, absolute=True), mr.momentum(robot, q, qs, there, absolute=True)
    assert np.array_equal(a[..., :3], b[..., :3])
    assert np.array_equal(mr.energy2(robot, q, qs, here), mr.energy2(robot, q, qs, there))
    allow = 8 * np.finfo(float).eps * (mag_a[..., 3:] + mag_b[..., 3:])
    assert np.all(np.abs(b[..., 3:] - (a[..., 3:] - np.cross(delta, a[..., :3]))) <= allow)


@pytest.mark.parametrize("key", (8, "torso", "nested"))
def test_reference_link_sets_add_up(key):
    """A link set and its complement sum to the whole robot, to rounding on the all-absolute magnitude."""
    robot, q, qs, _ = mc.case(key)
    part = mc.link_set(key, "set")
    rest = [i for i in range(len(robot["mass"])) if i not in part]
    for fn in (mr.momentum, mr.energy2):
        whole, mag = fn(robot, q, qs, mc.MOUNT), fn(robot, q, qs, mc.MOUNT, absolute=True)
        two = fn(robot, q, qs, mc.MOUNT, links=part) + fn(robot, q, qs, mc.MOUNT, links=rest)
        assert np.all(np.abs(whole - two) <= 8 * len(robot["mass"]) * np.finfo(float).eps * mag)


def test_a_chain_is_the_tree_of_its_links():
    chain, q, qs, _ = mc.case(7)
    as_tree = dict(chain, parent=np.arange(7) - 1)
    assert np.array_equal(mr.momentum(chain, q, qs, mc.MOUNT), mr.momentum(as_tree, q, qs, mc.MOUNT))
    assert np.array_equal(mr.energy2(chain, q, qs), mr.energy2(as_tree, q, qs))


def test_the_link_sets_are_what_the_cases_say():
    for d in mc.DOFS:
        assert mc.link_set(d, "all") is None and mc.link_set(d, "set") == tuple(range(d // 2, d)) and len(mc.link_set(d, "set")) >= 1
    for name in mc.NAMES:
        links, parents = mc.link_set(name, "set"), tc.SHAPES[name]
        assert links == mc.BRANCH_LINKS[name]
        # a branch: closed under "child of", and nothing of it is an ancestor of its first link
        assert all((parents[i] in links) == (i != links[0]) for i in links)
        assert all(parents[i] not in links for i in range(len(parents)) if i not in links)
    assert max(mc.link_set("nested", "set")) < len(tc.SHAPES["nested"]) - 1  # (the walk ends early there)


def test_the_bounds_are_positive_where_anything_is_summed():
    """... and zero where nothing is: the upper half of the 2-dof chain is its massless link, whose every term is an exact zero."""
    for key in mc.CASES:
        robot = mc.case(key)[0]
        for which in mc.SETS:
            links = mr.link_set(robot, mc.link_set(key, which))
            heavy = bool(robot["mass"][links].any() or robot["inertia"][links].any())
            assert heavy == ((key, which) != (2, "set"))
            for name in mc.QUANTITIES:
                assert (mc.bound(key, mc.name_of(name, which)) > 0) == heavy, (key, which, name)


def test_the_host_bound_is_the_minimum_of_three_divisions():
    h = np.array([[[3.0, 4.0, 0.0, 0.0, 0.0, 2.0], [0.0] * 6]])
    e2 = np.array([[8.0, 0.0]])
    got = mr.xbound(h, e2, [[50.0, 2.0, np.inf]])
    assert np.array_equal(got, [[[0.0, 0.5], [0.0, np.inf]]])
    assert np.array_equal(mr.xbound(h, e2, [[np.inf, np.inf, 4.0]])[0, :, 1], [0.5, np.inf])


# ---- momentum_batch, the robots' methods, the constraint ---------------------------------------------------------------------------

def _robots():
    return chain_ref.serial_chain(chain_ref.random_chain(3, 5)), tree_ref.kinematic_tree(tree_ref.random_tree([-1, 0, 0], 5))


def _problem(B=3, d=3, N=10):
    from toppra_amd import batch
    data = batch.make_synthetic_batch(B, d, N, seed=3)
    return data, (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])


def test_the_new_symbols_are_exported():
    import toppra_amd as ta
    from toppra_amd import _capi, batch, chain, constraint
    lib = _capi.load()
    assert "tpr_tree_momentum_batch" in _capi.EXPORTS and hasattr(lib, "tpr_tree_momentum_batch")
    for cls in (chain.SerialChain, chain.KinematicTree):
        assert hasattr(cls, "momentum") and hasattr(cls, "kinetic_energy")
    assert hasattr(batch, "momentum_batch") and "momentum_batch" in batch.__all__
    assert issubclass(constraint.BatchMomentumConstraint, constraint._BatchChainBound)
    assert ta.BatchMomentumConstraint is constraint.BatchMomentumConstraint and "BatchMomentumConstraint" in ta.__all__
    con = constraint.BatchMomentumConstraint(_robots()[0], linear=1.0)
    assert con.needs_q and con.first_order and con.source_count() == 1


def test_link_set_parsing():
    from toppra_amd import batch
    sc, tree = _robots()
    for robot in (sc, tree):
        assert batch.link_mask(robot) == batch.link_mask(robot, None) == 0b111
        assert batch.link_mask(robot, [0]) == 0b001 and batch.link_mask(robot, (2, 1)) == 0b110
        assert batch.link_mask(robot, [-1]) == 0b100 and batch.link_mask(robot, [-3, -1]) == 0b101
        assert batch.link_mask(robot, np.array([1, 1, 2])) == 0b110 and batch.link_mask(robot, iter(range(3))) == 0b111
        assert batch.link_mask(robot, {np.int32(1)}) == 0b010
        with pytest.raises(ValueError, match="empty"):
            batch.link_mask(robot, [])
        for bad in ([3], [-4], [0, 7]):
            with pytest.raises(ValueError, match="outside the robot's links 0..2"):
                batch.link_mask(robot, bad)
        for bad in ([0.0], [True], ["1"], [None]):
            with pytest.raises(ValueError, match="integers"):
                batch.link_mask(robot, bad)
        for bad in (1, "01", 0.5):
            with pytest.raises(ValueError, match="iterable"):
                batch.link_mask(robot, bad)
    wide = chain_ref.serial_chain(chain_ref.random_chain(32, 5))
    assert batch.link_mask(wide) == 0xFFFFFFFF and batch.link_mask(wide, [-1]) == 1 << 31


def test_units_are_physical_and_squared_on_the_host():
    from toppra_amd import constraint
    C = constraint.BatchMomentumConstraint
    sc, tree = _robots()
    con = C(sc, linear=5)
    assert con.limit.shape == (3,) and con.limit[0] == 25.0 and np.all(np.isinf(con.limit[1:])) and con._limit_batch is None
    con = C(tree, linear=5.0, angular=3.0, energy=4.0, links=[-1])
    assert np.array_equal(con.limit, [25.0, 9.0, 8.0]) and con.links == (-1,)
    con = C(sc, energy=np.array([1.0, 2.5, 4.0, 0.125]), angular=0.5)
    assert con._limit_batch == 4 and np.array_equal(con.limit, [[np.inf, 0.25, 2.0], [np.inf, 0.25, 5.0], [np.inf, 0.25, 8.0], [np.inf, 0.25, 0.25]])
    con.check(4, 10, 3)
    lin = np.array([0.1, 0.7, 3.0])
    assert np.array_equal(C(sc, linear=lin).limit[:, 0], lin * lin)  # (the very product: p * p, not p ** 2.0 or a rounded root)
    assert C(sc, linear=1.0).mount.mass == 0.0 and not C(sc, linear=1.0).mount.origin.any()
    assert "PHYSICAL" in C.__doc__ and "SQUARE" in C.__doc__  # (the contrast with the speed constraints' limits is documented)


def test_the_constraint_refuses_before_any_launch():
    from toppra_amd import algorithm, constraint
    C = constraint.BatchMomentumConstraint
    sc3, tree3 = _robots()
    sc4 = chain_ref.serial_chain(chain_ref.random_chain(4, 5))
    data, args = _problem()
    with pytest.raises(ValueError, match="SerialChain or KinematicTree"):
        C(lambda q, qd: q, linear=0.5)
    with pytest.raises(ValueError, match="Mount"):
        C(sc3, linear=0.5, mount=mc.MOUNT)
    with pytest.raises(ValueError, match="no limit given"):
        C(tree3)
    for name in ("linear", "angular", "energy"):
        for bad in (0.0, -1.0, np.nan, np.array([1.0, 0.0])):
            with pytest.raises(ValueError, match=name + " must be > 0"):
                C(sc3, **{name: bad})
        with pytest.raises(ValueError, match=name + r" must be a scalar or have shape \[B\]"):
            C(sc3, **{name: np.ones((2, 2))})
    with pytest.raises(ValueError, match="per trajectory for 3 and 5"):
        C(sc3, linear=np.ones(3), energy=np.ones(5))
    with pytest.raises(ValueError, match="outside the robot's links"):
        C(tree3, linear=1.0, links=[3])
    with pytest.raises(ValueError, match="empty"):
        C(tree3, linear=1.0, links=())
    with pytest.raises(ValueError, match="iterable"):
        C(tree3, linear=1.0, links=2)
    with pytest.raises(ValueError, match="has 4 joints"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc4, linear=0.5)])
    with pytest.raises(ValueError, match="per trajectory for 5"):
        algorithm.BatchTOPPRA(*args, constraints=[C(tree3, energy=np.ones(5))])
    qs = np.random.default_rng(0).standard_normal((3, 11, 3))
    with pytest.raises(ValueError, match="path positions"):
        algorithm.BatchTOPPRA.from_path_samples(data["grid"], None, qs, qs, data["vlim"], data["alim"], constraints=[C(tree3, linear=0.5)])
    with pytest.raises(ValueError, match="give the path positions"):
        C(sc3, linear=0.5).bound_sources(data["grid"], 3, 10, 3, qs, q=None)
    # a single path: the class serves batches alone
    with pytest.raises(NotImplementedError, match="BatchTOPPRA"):
        C(sc3, linear=0.5).compute_constraint_params(None, None)
    # a valid list passes the constructor, beside a torque limit on the same robot (its launches come later, on first use)
    taulim = np.stack([-np.ones(3), np.ones(3)], -1)
    inst = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchJointTorqueConstraint(tree3, taulim, np.zeros(3)),
                                                     C(tree3, linear=2.0, energy=np.ones(3), mount=bwr.mount_of(mc.MOUNT), links=[2])])
    assert len(inst.constraints) + len(inst.first_order) == 2


def test_array_entry_refuses_before_any_launch():
    from toppra_amd import _capi, batch
    q = np.zeros((2, 5, 3))
    for robot in _robots():
        with pytest.raises(ValueError, match="dof"):
            batch.momentum_batch(robot, np.zeros((2, 5, 4)), np.zeros((2, 5, 4)))
        with pytest.raises(ValueError, match="shape of q"):
            batch.momentum_batch(robot, q, np.zeros((2, 4, 3)))
        with pytest.raises(ValueError, match="Mount"):
            batch.momentum_batch(robot, q, q, mc.MOUNT)
        with pytest.raises(ValueError, match="outside the robot's links"):
            batch.momentum_batch(robot, q, q, links=[5])
        with pytest.raises(ValueError, match=r"\[B, N\+1, d\]"):
            batch.momentum_batch(robot, q[0], q[0], limit=np.ones(3))
        for bad in (1.0, np.ones(2), np.ones((3, 3)), np.ones((2, 2))):
            with pytest.raises(ValueError, match=r"limit must have shape \[3\] or \[B, 3\]"):
                batch.momentum_batch(robot, q, q, limit=bad)
        with pytest.raises(ValueError, match="limit must be > 0"):
            batch.momentum_batch(robot, q, q, limit=[1.0, 0.0, np.inf])
        with pytest.raises(ValueError, match="limit must be > 0"):
            batch.momentum_batch(robot, q, q, limit=[1.0, np.nan, 1.0])
        if _capi.device_count() == 0:  # (nothing computes without a GPU)
            with pytest.raises(_capi.ToppraHipError):
                robot.momentum(q, q)
            with pytest.raises(_capi.ToppraHipError):
                robot.kinetic_energy(q, q, links=[-1])
            with pytest.raises(_capi.ToppraHipError):
                batch.momentum_batch(robot, q, q, bwr.mount_of(mc.MOUNT), [0, 1], np.array([1.0, np.inf, 2.0]))

"""Control points on any link, without a GPU: the exports and the ABI guard, ``ControlPoints``, the surfaces of
``BatchPointSpeedConstraint`` / ``BatchPointAccelerationConstraint`` and the array entries -- every refusal happens before anything
is launched (without a GPU a launch would raise ToppraHipError instead of the expected error), and the C entries refuse a bad
point set before they look for a device."""
import ctypes

import numpy as np
import pytest

from tests import chain_ref

BADARG = -1


def _problem(B=3, d=3, N=10):
    from toppra_amd import batch
    data = batch.make_synthetic_batch(B, d, N, seed=3)
    return data, (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])


def _chain(d=3):
    return chain_ref.serial_chain(chain_ref.random_chain(d, 5))


def test_the_new_symbols_are_exported():
    import toppra_amd
    from toppra_amd import _capi, batch, chain, constraint
    lib = _capi.load()
    for name in ("tpr_chain_points_bytes", "tpr_chain_points_speed_batch", "tpr_chain_points_acceleration_batch",
                 "tpr_chain_points_acceleration_terms_batch"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert _capi.CHAIN_MAX_POINTS == 16
    assert lib.tpr_chain_points_bytes() == ctypes.sizeof(_capi.tpr_chain_points) == 8 + 16 * 4 + 16 * 3 * 8
    assert _capi.tpr_chain_points.link.offset == 4 and _capi.tpr_chain_points.offset.offset == 72
    assert toppra_amd.ControlPoints is chain.ControlPoints and "ControlPoints" in toppra_amd.__all__
    for name in ("point_speeds", "point_accelerations", "point_acceleration_terms"):
        assert hasattr(chain.SerialChain, name)
    for name in ("chain_points_speed_batch", "chain_points_acceleration_batch", "chain_points_acceleration_terms_batch"):
        assert name in batch.__all__
    assert issubclass(constraint.BatchPointAccelerationConstraint, constraint._BatchSecondOrder)
    assert issubclass(constraint.BatchPointSpeedConstraint, constraint._BatchFirstOrder)
    assert constraint.BatchPointSpeedConstraint.needs_q is True


def test_control_points_construction():
    from toppra_amd.chain import ControlPoints
    pts = ControlPoints([2, -1, 2, 0], np.arange(12.0).reshape(4, 3))
    assert pts.count == len(pts) == 4 and pts.links.dtype == np.int32 and pts.offsets.shape == (4, 3)
    assert pts.on(_chain(3)).tolist() == [2, 2, 2, 0] and pts.on(_chain(5)).tolist() == [2, 4, 2, 0]
    body = pts.c_struct(_chain(5))
    assert body.count == 4 and list(body.link)[:5] == [2, 4, 2, 0, 0] and list(body.offset[2]) == [6.0, 7.0, 8.0]
    assert ControlPoints(np.zeros(16, dtype=np.int64), np.zeros((16, 3))).count == 16
    for links, offsets in (([], np.zeros((0, 3))), ([0] * 17, np.zeros((17, 3))), (3, np.zeros(3)), ([[0]], np.zeros((1, 3)))):
        with pytest.raises(ValueError, match="1..16 points"):
            ControlPoints(links, offsets)
    for links in ([0.0, 1.0], [0.5], [True], ["a"], [None]):
        with pytest.raises(ValueError, match="integers"):
            ControlPoints(links, np.zeros((len(links), 3)))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="not finite"):
            ControlPoints([0, 1], [[0.0, 0.0, 0.0], [0.0, bad, 0.0]])
    with pytest.raises(ValueError, match=r"\[P, 3\]"):
        ControlPoints([0, 1], np.zeros((3, 3)))
    with pytest.raises(ValueError, match=r"\[P, 3\]"):
        ControlPoints([0, 1], np.zeros(3))
    with pytest.raises(ValueError, match="links must lie"):
        ControlPoints([-2], np.zeros((1, 3)))
    # bound to a chain: a link outside it
    with pytest.raises(ValueError, match="link 3, the chain has links 0..2"):
        ControlPoints([0, 3], np.zeros((2, 3))).on(_chain(3))
    with pytest.raises(ValueError, match="outside|the chain has"):
        ControlPoints([4], np.zeros((1, 3))).c_struct(_chain(3))


def test_array_entries_refuse_before_any_launch():
    from toppra_amd import batch
    from toppra_amd.chain import ControlPoints
    sc = _chain(3)
    pts = ControlPoints([0, 2], np.zeros((2, 3)))
    q = np.zeros((2, 5, 3))
    calls = (lambda p, a=q, b=q, c=q: batch.chain_points_speed_batch(sc, a, b, p),
             lambda p, a=q, b=q, c=q: batch.chain_points_acceleration_batch(sc, a, b, c, p),
             lambda p, a=q, b=q, c=q: batch.chain_points_acceleration_terms_batch(sc, a, b, c, p),
             lambda p, a=q, b=q, c=q: sc.point_speeds(a, b, p),
             lambda p, a=q, b=q, c=q: sc.point_accelerations(a, b, c, p),
             lambda p, a=q, b=q, c=q: sc.point_acceleration_terms(a, b, c, p))
    for call in calls:
        with pytest.raises(ValueError, match="ControlPoints"):
            call(([0], [[0.0, 0.0, 0.0]]))
        with pytest.raises(ValueError, match="the chain has links 0..2"):
            call(ControlPoints([3], np.zeros((1, 3))))
        with pytest.raises(ValueError, match="chain's dof"):
            call(pts, np.zeros((2, 5, 4)), np.zeros((2, 5, 4)), np.zeros((2, 5, 4)))
        with pytest.raises(ValueError, match="shape of q"):
            call(pts, q, np.zeros((2, 4, 3)), q)
    with pytest.raises(ValueError, match=r"\[B, N\+1, d\]"):
        batch.chain_points_speed_batch(sc, np.zeros((5, 3)), np.zeros((5, 3)), pts, limit=0.5)
    for bad in (np.ones(3), np.ones((3, 2)), np.ones((2, 3)), np.ones((2, 5, 2))):
        with pytest.raises(ValueError, match=r"\[B, P\]"):
            batch.chain_points_speed_batch(sc, q, q, pts, limit=bad)
    for bad in (0.0, -1.0, np.nan, np.array([0.5, 0.0]), np.array([[0.5, 0.5], [0.5, -0.5]])):
        with pytest.raises(ValueError, match="limit must be > 0"):
            batch.chain_points_speed_batch(sc, q, q, pts, limit=bad)


def test_c_entries_refuse_a_bad_point_set_first():
    """TPR_E_BADARG for a NULL struct, a count outside 1..16, a link outside 0..d-1, a non-finite offset, speed2 and xbound both
    NULL, xbound without limit -- each before the entry looks for a device, so also on a machine without one; the buffers
    handed over with the refused calls are a few doubles long."""
    from toppra_amd import _capi
    from toppra_amd.chain import ControlPoints
    lib = _capi.load()
    sc = _chain(3)
    one = np.zeros(6)
    p = one.ctypes.data
    model, keep = sc.c_struct(one)
    m = ctypes.byref(model)

    def calls(points, chain=m):
        x = None if points is None else ctypes.byref(points)
        return (lib.tpr_chain_points_speed_batch(chain, x, 1, 1, p, p, p, p, p, 0, None),
                lib.tpr_chain_points_acceleration_batch(chain, x, 2, p, p, p, p, 0, None),
                lib.tpr_chain_points_acceleration_terms_batch(chain, x, 1, 1, p, p, p, p, p, 0, None))

    def points(**kw):
        body = ControlPoints([0, 2], np.ones((2, 3))).c_struct(sc)
        for k, v in kw.items():
            setattr(body, k, v)
        return body

    assert calls(None) == (BADARG,) * 3 and b"null control points" in lib.tpr_last_error()
    assert calls(points(), chain=None) == (BADARG,) * 3
    for count in (0, -1, 17, 1 << 20):
        assert calls(points(count=count)) == (BADARG,) * 3, count
        assert b"point count" in lib.tpr_last_error()
    for link in (3, -1, 32, -(1 << 31)):
        body = points()
        body.link[1] = link
        assert calls(body) == (BADARG,) * 3, link
        assert b"outside the chain" in lib.tpr_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        body = points()
        body.offset[1][2] = bad
        assert calls(body) == (BADARG,) * 3
        assert b"finite" in lib.tpr_last_error()
    body = points()
    body.link[2], body.offset[2][0] = 99, np.nan  # (past count: not read)
    x = ctypes.byref(body)
    assert lib.tpr_chain_points_speed_batch(m, x, 1, 1, p, p, p, None, None, 0, None) == BADARG
    assert b"one of speed2, xbound" in lib.tpr_last_error()
    assert lib.tpr_chain_points_speed_batch(m, x, 1, 1, p, p, None, p, p, 0, None) == BADARG
    assert b"xbound needs limit" in lib.tpr_last_error()
    assert lib.tpr_chain_points_speed_batch(m, x, -1, 1, p, p, p, p, p, 0, None) == BADARG
    assert lib.tpr_chain_points_acceleration_terms_batch(m, x, 1, -1, p, p, p, p, p, 0, None) == BADARG
    for k in range(2):  # q, qs
        a = [p] * 2
        a[k] = None
        assert lib.tpr_chain_points_speed_batch(m, x, 1, 1, *a, p, p, p, 0, None) == BADARG, k
    for k in range(4):  # q, qd, qdd, acc
        a = [p] * 4
        a[k] = None
        assert lib.tpr_chain_points_acceleration_batch(m, x, 2, *a, 0, None) == BADARG, k
    for k in range(5):  # q, qs, qss, wa, wb
        a = [p] * 5
        a[k] = None
        assert lib.tpr_chain_points_acceleration_terms_batch(m, x, 1, 1, *a, 0, None) == BADARG, k
    if _capi.device_count() == 0:  # ... and nothing is computed without a GPU
        assert all(rc < 0 for rc in calls(points())) and b"tpr_init" in lib.tpr_last_error()
        pts = ControlPoints([0, 2], np.zeros((2, 3)))
        q = np.zeros((2, 5, 3))
        for call in (lambda: sc.point_speeds(q, q, pts), lambda: sc.point_accelerations(q, q, q, pts),
                     lambda: sc.point_acceleration_terms(q, q, q, pts)):
            with pytest.raises(_capi.ToppraHipError):
                call()


def test_rows_per_stage_and_the_rows_of_each_spelling():
    from toppra_amd import constraint
    from toppra_amd.chain import ControlPoints
    C, DT = constraint.BatchPointAccelerationConstraint, constraint.DiscretizationType
    sc = _chain(3)
    two, three = ControlPoints([0, -1], np.ones((2, 3))), ControlPoints([1, 1, 0], np.ones((3, 3)))
    assert C(sc, two, linear=0.5).get_discretization_type() == DT.Interpolation  # the reference's default for SecondOrderConstraint
    assert C(sc, two, linear=0.5).rows_per_stage(3) == 24
    assert C(sc, two, linear=0.5, discretization_scheme=DT.Collocation).rows_per_stage(3) == 12
    assert C(sc, three, linear=[0.5, 1.0, 2.0]).rows_per_stage(3) == 36
    assert C(sc, three, F=np.ones((5, 9)), g=np.ones(5)).rows_per_stage(3) == 10
    assert C(sc, three, F=np.ones((4, 11, 5, 9)), g=np.ones((4, 5)), discretization_scheme=DT.Collocation).rows_per_stage(3) == 5
    # six rows per point, the signed identity on that point's three components, g = [upper; -lower], the points in order
    I, Z = np.eye(3), np.zeros((3, 3))
    want_F = np.block([[I, Z], [-I, Z], [Z, I], [Z, -I]])
    con = C(sc, two, linear=0.5)
    assert np.array_equal(con.F, want_F) and np.array_equal(con.g, [0.5] * 12)
    con = C(sc, two, linear=[0.5, 2.0])
    assert np.array_equal(con.F, want_F) and np.array_equal(con.g, [0.5] * 6 + [2.0] * 6)
    lim = np.array([[[-1.0, 2.0], [-3.0, 4.0], [-5.0, 6.0]], [[-7.0, 8.0], [-9.0, 10.0], [-11.0, 12.0]]])  # [P = 2, 3, 2]
    con = C(sc, two, linear=lim)
    assert np.array_equal(con.F, want_F) and np.array_equal(con.g, [2.0, 4.0, 6.0, 1.0, 3.0, 5.0, 8.0, 10.0, 12.0, 7.0, 9.0, 11.0])
    per_traj = np.stack([lim, 2.0 * lim, 3.0 * lim, 4.0 * lim])  # [B = 4, P, 3, 2]
    con = C(sc, two, linear=per_traj)
    assert con.g.shape == (4, 12) and np.array_equal(con.g[2], 3.0 * np.array([2.0, 4.0, 6.0, 1.0, 3.0, 5.0, 8.0, 10.0, 12.0, 7.0, 9.0, 11.0]))
    con.check(4, 10, 3)
    con = C(sc, three, linear=1.0)
    assert con.F.shape == (18, 9) and np.array_equal(con.F[12:15, 6:9], I) and np.array_equal(con.F[15:18, 6:9], -I)
    assert np.count_nonzero(con.F) == 18
    F, g = np.arange(45.0).reshape(5, 9), np.arange(5.0)
    con = C(sc, three, F=F, g=g)
    assert con.F is F and con.g is g


def test_the_acceleration_constraint_refuses_before_any_launch():
    from toppra_amd import algorithm, constraint
    from toppra_amd.chain import ControlPoints
    C = constraint.BatchPointAccelerationConstraint
    sc3, sc4 = _chain(3), _chain(4)
    two = ControlPoints([0, -1], np.ones((2, 3)))
    data, args = _problem()
    with pytest.raises(ValueError, match="SerialChain"):
        C(lambda q, qd, qdd: q, two, linear=0.5)
    with pytest.raises(ValueError, match="ControlPoints"):
        C(sc3, [0, 1], linear=0.5)
    with pytest.raises(ValueError, match="the chain has links 0..2"):
        C(sc3, ControlPoints([3], np.zeros((1, 3))), linear=0.5)
    with pytest.raises(ValueError, match="no limit given"):
        C(sc3, two)
    with pytest.raises(ValueError, match="not both"):
        C(sc3, two, linear=0.5, F=np.ones((2, 6)), g=np.ones(2))
    with pytest.raises(ValueError, match="together"):
        C(sc3, two, F=np.ones((2, 6)))
    with pytest.raises(ValueError, match="together"):
        C(sc3, two, g=np.ones(2))
    for bad in (np.ones(3), np.ones((3, 2)), np.ones((2, 2)), np.ones((3, 3, 2)), np.ones((5, 4, 2, 3, 2))):
        with pytest.raises(ValueError, match=r"\[P, 3, 2\]"):
            C(sc3, two, linear=bad)
    for bad in (np.nan, np.inf, [1.0, np.inf]):
        with pytest.raises(ValueError, match="not finite"):
            C(sc3, two, linear=bad)
    with pytest.raises(ValueError, match="above its upper"):
        C(sc3, two, linear=-0.5)
    with pytest.raises(ValueError, match="above its upper"):
        C(sc3, two, linear=[0.5, -0.5])
    with pytest.raises(ValueError, match=r"\[m, 3 P\]"):
        C(sc3, two, F=np.ones((2, 9)), g=np.ones(2))
    with pytest.raises(ValueError, match="g must have shape"):
        C(sc3, two, F=np.ones((2, 6)), g=np.ones((1, 1, 1, 2)))
    with pytest.raises(ValueError, match="F has 2 rows"):
        C(sc3, two, F=np.ones((2, 6)), g=np.ones(3))
    with pytest.raises(ValueError, match="not finite"):
        C(sc3, two, F=np.ones((2, 6)), g=np.array([1.0, np.nan]))
    # against the problem's sizes: in BatchTOPPRA's constructor
    with pytest.raises(ValueError, match="chain has 4 joints"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc4, two, linear=0.5)])
    with pytest.raises(ValueError, match="per trajectory for 5"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, two, linear=np.tile([-1.0, 1.0], (5, 2, 3, 1)))])
    with pytest.raises(ValueError, match="leading shape"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, two, F=np.ones((5, 2, 6)), g=np.ones(2))])
    qs = np.random.default_rng(0).standard_normal((3, 11, 3))
    with pytest.raises(ValueError, match="path positions"):
        algorithm.BatchTOPPRA.from_path_samples(data["grid"], None, qs, qs, data["vlim"], data["alim"], constraints=[C(sc3, two, linear=0.5)])
    with pytest.raises(NotImplementedError, match="BatchTOPPRA"):
        C(sc3, two, linear=0.5).compute_constraint_params(None, None)
    with pytest.raises(NotImplementedError, match="BatchPointAccelerationConstraint"):
        algorithm.BatchTOPPRA(*args, constraints=[object()])


def test_the_speed_constraint_s_surface():
    from toppra_amd import algorithm, constraint
    from toppra_amd.chain import ControlPoints
    C = constraint.BatchPointSpeedConstraint
    sc3, sc4 = _chain(3), _chain(4)
    two = ControlPoints([0, -1], np.ones((2, 3)))
    sixteen = ControlPoints([0, 1, 2, 1] * 4, np.ones((16, 3)))
    data, args = _problem()
    for limit in (0.25, [0.25, 0.5], np.full((3, 2), 0.25)):
        con = C(sc3, two, limit)
        assert con.source_count() == 1 and con.first_order and con.needs_q
    assert C(sc3, sixteen, 0.25).source_count() == 1  # one xbound source however many points
    with pytest.raises(ValueError, match="SerialChain"):
        C(None, two, 0.25)
    with pytest.raises(ValueError, match="ControlPoints"):
        C(sc3, ([0], [[0.0] * 3]), 0.25)
    with pytest.raises(ValueError, match="the chain has links 0..2"):
        C(sc3, ControlPoints([5], np.zeros((1, 3))), 0.25)
    for bad in (np.ones(3), np.ones((3, 3)), np.ones((2, 2, 2))):
        with pytest.raises(ValueError, match=r"\[B, P\]"):
            C(sc3, two, bad)
    for bad in (0.0, -1.0, np.nan, [0.25, 0.0], np.array([[0.25, 0.25], [0.25, np.nan]])):
        with pytest.raises(ValueError, match="limit must be > 0"):
            C(sc3, two, bad)
    with pytest.raises(ValueError, match="chain has 4 joints"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc4, two, 0.25)])
    with pytest.raises(ValueError, match="per trajectory for 5"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, two, np.full((5, 2), 0.25))])
    qs = np.random.default_rng(0).standard_normal((3, 11, 3))
    with pytest.raises(ValueError, match="path positions"):
        algorithm.BatchTOPPRA.from_path_samples(data["grid"], None, qs, qs, data["vlim"], data["alim"], constraints=[C(sc3, two, 0.25)])
    with pytest.raises(NotImplementedError, match="BatchTOPPRA"):
        C(sc3, two, 0.25).compute_constraint_params(None, None)
    # eight sets are eight sources: with vlim one too many for the box kernel
    with pytest.raises(NotImplementedError, match="9 bound sources"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, two, 0.25) for _ in range(8)])
    # a valid list passes both constructors, beside every other chain constraint (its launches come later, on first use)
    taulim = np.stack([-np.ones(3), np.ones(3)], -1)
    A = constraint.BatchPointAccelerationConstraint
    cons = [constraint.BatchJointTorqueConstraint(sc3, taulim, np.zeros(3)), A(sc3, two, linear=0.5), C(sc3, two, 0.25),
            constraint.BatchCartesianVelocityNormConstraint(sc3, 0.25), constraint.BatchCartesianAccelerationConstraint(sc3, linear=0.5)]
    inst = algorithm.BatchTOPPRA(*args, constraints=cons)
    assert len(inst.constraints) == 3 and len(inst.first_order) == 2
    inst = algorithm.BatchTOPPRA.from_path_samples(data["grid"], qs, qs, qs, data["vlim"], data["alim"], constraints=cons)
    assert len(inst.constraints) == 3 and len(inst.first_order) == 2


def test_the_122_row_limit_is_refused_before_any_launch():
    """27 dof, acceleration limits and 4 control points under Interpolation: 2 + 108 + 48 = 158 rows per stage; one point: 122."""
    from toppra_amd import algorithm, constraint
    from toppra_amd.chain import ControlPoints
    d = 27
    sc = _chain(d)
    data, args = _problem(B=2, d=d, N=6)
    C = constraint.BatchPointAccelerationConstraint
    con = C(sc, ControlPoints([3, 9, 20, -1], np.zeros((4, 3))), linear=0.5)
    with pytest.raises(NotImplementedError, match="158 constraint rows"):
        algorithm.BatchTOPPRA(*args, constraints=[con])
    q = np.zeros((2, 7, d))
    with pytest.raises(NotImplementedError, match="158 constraint rows"):
        algorithm.BatchTOPPRA.from_path_samples(data["grid"], q, q, q, data["vlim"], data["alim"], constraints=[con])
    # ... and one point fits exactly: 2 + 108 + 12; two do not: 134
    algorithm.BatchTOPPRA(*args, constraints=[C(sc, ControlPoints([9], np.zeros((1, 3))), linear=0.5)])
    with pytest.raises(NotImplementedError, match="134 constraint rows"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc, ControlPoints([9, 26], np.zeros((2, 3))), linear=0.5)])

"""The wrench at the tool without a GPU: the numpy reference (tests/tool_wrench_ref.py) against an independent route, the
merged chain of ``SerialChain.with_payload``, the closed-form contact wrench cone against the corner-force LP, and the surface of
``Payload`` / ``BatchToolWrenchConstraint`` -- every refusal happens before anything is launched (this machine has no GPU: a
launch would raise ToppraHipError instead of the expected error)."""
import os

import numpy as np
import pytest

from tests import chain_cases as cc, chain_ref, tool_wrench_cases as tw, tool_wrench_ref as twr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = np.eye(3)


def _extended(chain, q, qs, qss, axis, prismatic, dtype=np.float64, absolute=False):
    """Inverse dynamics of the chain extended by the payload as a (d+1)-th link, the extra joint held at 0."""
    ext = twr.extended_chain(chain, tw.PAYLOAD, axis, prismatic)
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (1,))], -1)  # noqa: E731
    return chain_ref.rnea(ext, pad(q), pad(qs), pad(qss), dtype=dtype, absolute=absolute)


@pytest.mark.parametrize("d", tw.DOFS)
def test_reference_against_the_extended_chain(d):
    """(1) The payload as the link of an extra joint at the contact frame, held still: the joint's torque about axis k is the
    k-th moment component, a prismatic joint's force along axis k the k-th force component.  The allowance is the case's bound
    (16 x the float64 reference's own error against np.longdouble), on the reference's magnitude."""
    chain, q, qs, qss = cc.case(d)
    ref = tw.reference(d)
    for name in ("w0", "wb"):
        args = tw.evaluations(q, qs, qss)[name]
        got = np.stack([_extended(chain, *args, AXES[k], True)[..., -1] for k in range(3)]
                       + [_extended(chain, *args, AXES[k], False)[..., -1] for k in range(3)], -1)
        err, bound = cc.metric(got, ref[name], ref[name + "_mag"]), tw.bound(d, name)
        print("d %d %s: extended chain vs reference %.3g, bound %.3g" % (d, name, err, bound))
        assert err <= bound, (d, name, err, bound)
        assert bound > 0 or not chain["gravity"].any()


def test_the_reference_at_rest_is_the_weight():
    chain, q, _, _ = cc.case(8)
    assert chain["gravity"].any()
    centred = dict(tw.PAYLOAD, origin=tw.PAYLOAD["com"])
    w0 = twr.tool_wrench(chain, centred, q, np.zeros_like(q), np.zeros_like(q))
    weight = tw.PAYLOAD["mass"] * np.linalg.norm(chain["gravity"])
    assert np.allclose(np.linalg.norm(w0[..., :3], axis=-1), weight, rtol=1e-13, atol=0)
    assert np.abs(w0[..., 3:]).max() <= 1e-13 * weight


def _dict_of(sc):
    return {"joint_type": np.array([1 if t == "prismatic" else 0 for t in sc.joint_types], dtype=np.int32), "axis": sc.axes,
            "rot": sc.rotations, "trans": sc.translations, "mass": sc.masses, "com": sc.coms, "inertia": sc.inertias,
            "gravity": sc.gravity, "tool": sc.tool}


@pytest.mark.parametrize("d", tw.DOFS)
def test_with_payload_loads_the_joints_as_the_extended_chain_does(d):
    """(2) Inverse dynamics of the merged chain = the first d entries of the extended chain's, within 16 x the error the float64
    extended chain shows against np.longdouble, in the metric of tests/chain_cases.py."""
    chain, q, qs, qss = cc.case(d)
    merged = _dict_of(chain_ref.serial_chain(chain).with_payload(twr.payload_of(tw.PAYLOAD, chain)))
    assert merged["mass"][-1] == chain["mass"][-1] + tw.PAYLOAD["mass"] and np.array_equal(merged["mass"][:-1], chain["mass"][:-1])
    got = chain_ref.rnea(merged, q, qs, qss)
    want, mag = (_extended(chain, q, qs, qss, AXES[2], False, absolute=ab)[..., :d] for ab in (False, True))
    yardstick = cc._own_error(want, _extended(chain, q, qs, qss, AXES[2], False, dtype=np.longdouble)[..., :d], mag)
    err = cc.metric(got, want, mag)
    print("d %d: merged vs extended chain %.3g, bound %.3g" % (d, err, tw.BOUND_FACTOR * yardstick))
    assert 0 < yardstick and err <= tw.BOUND_FACTOR * yardstick, (d, err, yardstick)


def test_with_payload_of_nothing_changes_nothing():
    from toppra_amd.chain import Payload
    sc = chain_ref.serial_chain(cc.case(7)[0])
    same = sc.with_payload(Payload(0.0, com=(0.1, 0.2, 0.3)))
    assert same is not sc
    for name in ("axes", "rotations", "translations", "masses", "coms", "inertias", "gravity", "tool"):
        assert np.array_equal(getattr(same, name), getattr(sc, name)), name
    assert same.joint_types == sc.joint_types


def _corner_lp_feasible(w, mu, X, Y):
    """The authority: four corner forces, each in its 4-sided friction pyramid, that sum to the wrench w about the patch centre."""
    from scipy.optimize import linprog
    corners = [(sx * X, sy * Y) for sx in (1, -1) for sy in (1, -1)]
    A_eq, A_ub = np.zeros((6, 12)), np.zeros((16, 12))
    for i, (x, y) in enumerate(corners):
        A_eq[0, 3 * i], A_eq[1, 3 * i + 1], A_eq[2, 3 * i + 2] = 1, 1, 1
        A_eq[3, 3 * i + 2] = y                           # tx = y fz - z fy, z = 0
        A_eq[4, 3 * i + 2] = -x                          # ty = z fx - x fz
        A_eq[5, 3 * i + 1], A_eq[5, 3 * i] = x, -y       # tz = x fy - y fx
        for k, (col, sign) in enumerate(((0, 1), (0, -1), (1, 1), (1, -1))):
            A_ub[4 * i + k, 3 * i + col], A_ub[4 * i + k, 3 * i + 2] = sign, -mu
    res = linprog(np.zeros(12), A_ub=A_ub, b_ub=np.zeros(16), A_eq=A_eq, b_eq=w, bounds=[(None, None)] * 12, method="highs")
    return res.status == 0


def test_surface_contact_rows_against_the_corner_force_lp():
    """(3) 2 400 seeded random wrenches; those within 1e-6 of the cone's boundary are skipped (the LP's own tolerance)."""
    from toppra_amd.constraint import BatchToolWrenchConstraint as C
    mu, X, Y = 0.6, 0.08, 0.05
    F, g = C.surface_contact_rows(mu, (X, Y))
    assert F.shape == (16, 6) and not g.any()
    rng = np.random.default_rng(31)
    n, inside, skipped = 2400, 0, 0
    for _ in range(n):
        fz = rng.uniform(-0.2, 2.0)
        w = np.array([rng.normal(0, 0.45 * mu), rng.normal(0, 0.45 * mu), fz, rng.normal(0, 0.45 * Y), rng.normal(0, 0.45 * X),
                      rng.normal(0, 0.3 * mu * (X + Y))])
        worst = np.max(F @ w)
        if abs(worst) < 1e-6:
            skipped += 1
            continue
        ok = _corner_lp_feasible(w, mu, X, Y)
        assert ok == (worst <= 0), (w, worst, ok)
        inside += ok
    print("%d wrenches, %d inside, %d skipped" % (n, inside, skipped))
    assert 0.1 * n <= inside <= 0.9 * n and skipped < 0.01 * n


def test_surface_contact_rows_and_the_normal_force_row():
    from toppra_amd.constraint import BatchToolWrenchConstraint as C
    mu, X, Y = 0.5, 0.2, 0.1
    F, g = C.surface_contact_rows(mu, (X, Y))
    assert np.array_equal(F[0], [1, 0, -mu, 0, 0, 0]) and np.array_equal(F[3], [0, -1, -mu, 0, 0, 0])
    assert np.array_equal(F[4], [0, 0, -Y, 1, 0, 0]) and np.array_equal(F[7], [0, 0, -X, 0, -1, 0])
    assert np.array_equal(F[8], [Y, X, -mu * (X + Y), mu, mu, 1]) and np.array_equal(F[9], [Y, X, -mu * (X + Y), -mu, -mu, -1])
    assert np.array_equal(F[14], [-Y, -X, -mu * (X + Y), -mu, -mu, 1])
    F2, g2 = C.surface_contact_rows(mu, (X, Y), normal_force_min=3.0)
    assert F2.shape == (17, 6) and np.array_equal(F2[:16], F) and np.array_equal(F2[16], [0, 0, -1, 0, 0, 0])
    assert np.array_equal(g2, [0.0] * 16 + [-3.0])
    sc = chain_ref.serial_chain(chain_ref.random_chain(3, 5))
    con = C.surface_contact(sc, twr.payload_of(tw.PAYLOAD, None), mu, (X, Y), normal_force_min=3.0)
    assert np.array_equal(con.F, F2) and np.array_equal(con.g, g2) and con.rows_per_stage(3) == 34
    for bad in dict(mu=0.0), dict(mu=np.nan), dict(half_extents=(0.1, 0.0)), dict(half_extents=(0.1,)), dict(normal_force_min=-1.0):
        kw = dict(dict(mu=mu, half_extents=(X, Y)), **bad)
        with pytest.raises(ValueError):
            C.surface_contact(sc, twr.payload_of(tw.PAYLOAD, None), **kw)


def _problem(B=3, d=3, N=10):
    from toppra_amd import batch
    data = batch.make_synthetic_batch(B, d, N, seed=3)
    return data, (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])


def test_the_new_symbols_are_exported():
    import toppra_amd as ta
    from toppra_amd import _capi, batch, chain, constraint
    lib = _capi.load()
    for name in ("tpr_payload_bytes", "tpr_chain_tool_wrench_batch", "tpr_chain_tool_wrench_terms_batch"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert lib.tpr_payload_bytes() == 22 * 8
    for name in ("tool_wrench", "tool_wrench_terms", "with_payload"):
        assert hasattr(chain.SerialChain, name)
    assert "chain_tool_wrench_batch" in batch.__all__ and "chain_tool_wrench_terms_batch" in batch.__all__
    assert issubclass(constraint.BatchToolWrenchConstraint, constraint._BatchSecondOrder)
    assert ta.Payload is chain.Payload and ta.BatchToolWrenchConstraint is constraint.BatchToolWrenchConstraint
    assert "Payload" in ta.__all__


def test_payload_validation_and_defaults():
    from toppra_amd.chain import Payload
    sc = chain_ref.serial_chain(chain_ref.random_chain(3, 5))
    p = Payload(2.0)
    assert p.mass == 2.0 and not p.com.any() and not p.inertia.any() and np.array_equal(p.frame_rotation, np.eye(3))
    assert p.frame_origin is None and np.array_equal(p.origin(sc), sc.tool)
    body = p.c_struct(sc)
    assert list(body.origin) == list(sc.tool) and list(body.rot) == list(np.eye(3).ravel()) and body.mass == 2.0
    full = np.array([[3.0, 0.1, 0.2], [0.1, 4.0, 0.3], [0.2, 0.3, 5.0]])
    assert np.array_equal(Payload(1.0, inertia=full).inertia, [3.0, 4.0, 5.0, 0.1, 0.2, 0.3])
    assert list(Payload(1.0, frame_origin=(1, 2, 3)).c_struct(sc).origin) == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="mass must be >= 0"):
        Payload(-1.0)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="not finite"):
            Payload(bad)
        with pytest.raises(ValueError, match="not finite"):
            Payload(1.0, com=(0.0, bad, 0.0))
        with pytest.raises(ValueError, match="not finite"):
            Payload(1.0, inertia=[1, 1, 1, 0, 0, bad])
        with pytest.raises(ValueError, match="not finite"):
            Payload(1.0, frame_origin=(bad, 0, 0))
    with pytest.raises(ValueError, match="symmetric"):
        Payload(1.0, inertia=full + np.triu(np.ones((3, 3)), 1))
    with pytest.raises(ValueError, match=r"com must have shape \[3\]"):
        Payload(1.0, com=(0.0, 1.0))
    with pytest.raises(ValueError, match=r"inertia must have shape \[6\]"):
        Payload(1.0, inertia=np.ones(5))
    with pytest.raises(ValueError, match=r"frame_rotation must have shape \[3, 3\]"):
        Payload(1.0, frame_rotation=np.ones(3))
    with pytest.raises(ValueError, match="orthonormal"):
        Payload(1.0, frame_rotation=np.eye(3) * 1.001)
    with pytest.raises(ValueError, match="orthonormal"):
        Payload(1.0, frame_rotation=np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError, match="not an array of numbers"):
        Payload("heavy")


def test_rows_per_stage_and_the_rows_of_each_spelling():
    """(5)"""
    from toppra_amd import constraint
    C, DT = constraint.BatchToolWrenchConstraint, constraint.DiscretizationType
    sc, obj = chain_ref.serial_chain(chain_ref.random_chain(3, 5)), twr.payload_of(tw.PAYLOAD, None)
    assert C(sc, obj, force=0.5).get_discretization_type() == DT.Interpolation  # the reference's default for SecondOrderConstraint
    assert C(sc, obj, force=0.5).rows_per_stage(3) == 12
    assert C(sc, obj, force=0.5, discretization_scheme=DT.Collocation).rows_per_stage(3) == 6
    assert C(sc, obj, moment=np.tile([-1.0, 2.0], (3, 1))).rows_per_stage(3) == 12
    assert C(sc, obj, force=0.5, moment=2.0).rows_per_stage(3) == 24
    assert C(sc, obj, force=0.5, moment=2.0, discretization_scheme=DT.Collocation).rows_per_stage(3) == 12
    assert C(sc, obj, F=np.ones((5, 6)), g=np.ones(5)).rows_per_stage(3) == 10
    assert C(sc, obj, F=np.ones((4, 11, 5, 6)), g=np.ones((4, 5)), discretization_scheme=DT.Collocation).rows_per_stage(3) == 5
    assert C.surface_contact(sc, obj, 0.5, (0.1, 0.1)).rows_per_stage(3) == 32
    assert C.surface_contact(sc, obj, 0.5, (0.1, 0.1), discretization_scheme=DT.Collocation).rows_per_stage(3) == 16
    # the signed identity on each part, g = [upper; -lower]; the force first
    con = C(sc, obj, force=np.array([[-1.0, 2.0], [-3.0, 4.0], [-5.0, 6.0]]), moment=0.25)
    I, Z = np.eye(3), np.zeros((3, 3))
    assert np.array_equal(con.F, np.block([[I, Z], [-I, Z], [Z, I], [Z, -I]]))
    assert np.array_equal(con.g, [2.0, 4.0, 6.0, 1.0, 3.0, 5.0] + [0.25] * 6)
    lim = np.stack([-np.arange(1.0, 13.0).reshape(4, 3), np.arange(2.0, 14.0).reshape(4, 3)], -1)  # [B = 4, 3, 2]
    con = C(sc, obj, force=0.5, moment=lim)
    assert con.g.shape == (4, 12) and np.array_equal(con.g[1], [0.5] * 6 + [5.0, 6.0, 7.0, 4.0, 5.0, 6.0])
    con.check(4, 10, 3)


def test_the_constraint_refuses_before_any_launch():
    """(4)"""
    from toppra_amd import algorithm, constraint
    C = constraint.BatchToolWrenchConstraint
    sc3, sc4 = chain_ref.serial_chain(chain_ref.random_chain(3, 5)), chain_ref.serial_chain(chain_ref.random_chain(4, 5))
    obj = twr.payload_of(tw.PAYLOAD, None)
    data, args = _problem()
    with pytest.raises(ValueError, match="SerialChain"):
        C(lambda q, qd, qdd: q, obj, force=0.5)
    with pytest.raises(ValueError, match="Payload"):
        C(sc3, tw.PAYLOAD, force=0.5)
    with pytest.raises(ValueError, match="no limit given"):
        C(sc3, obj)
    with pytest.raises(ValueError, match="not both"):
        C(sc3, obj, force=0.5, F=np.ones((2, 6)), g=np.ones(2))
    with pytest.raises(ValueError, match="not both"):
        C(sc3, obj, moment=0.5, g=np.ones(2))
    with pytest.raises(ValueError, match="not both"):
        C.surface_contact(sc3, obj, 0.5, (0.1, 0.1), force=10.0)
    with pytest.raises(ValueError, match="together"):
        C(sc3, obj, F=np.ones((2, 6)))
    with pytest.raises(ValueError, match="together"):
        C(sc3, obj, g=np.ones(2))
    for bad in (np.ones(3), np.ones((3, 3)), np.ones((2, 2)), np.ones((5, 4, 3, 2))):
        with pytest.raises(ValueError, match=r"force must be a scalar or have shape \[3, 2\]"):
            C(sc3, obj, force=bad)
        with pytest.raises(ValueError, match=r"moment must be a scalar or have shape \[3, 2\]"):
            C(sc3, obj, moment=bad)
    for bad in (np.nan, np.inf, np.array([[-1.0, 1.0], [-1.0, np.inf], [-1.0, 1.0]])):
        with pytest.raises(ValueError, match="not finite"):
            C(sc3, obj, force=bad)
    with pytest.raises(ValueError, match="above its upper"):
        C(sc3, obj, force=-0.5)
    with pytest.raises(ValueError, match="above its upper"):
        C(sc3, obj, moment=np.array([[-1.0, 1.0], [2.0, 1.0], [-1.0, 1.0]]))
    with pytest.raises(ValueError, match="force and moment are given per trajectory for 3 and 4"):
        C(sc3, obj, force=np.tile([-1.0, 1.0], (3, 3, 1)), moment=np.tile([-1.0, 1.0], (4, 3, 1)))
    with pytest.raises(ValueError, match=r"\[m, 6\]"):
        C(sc3, obj, F=np.ones((2, 3)), g=np.ones(2))
    with pytest.raises(ValueError, match=r"\[m, 6\]"):
        C(sc3, obj, F=np.ones(6), g=np.ones(1))
    with pytest.raises(ValueError, match="g must have shape"):
        C(sc3, obj, F=np.ones((2, 6)), g=np.ones((1, 1, 1, 2)))
    with pytest.raises(ValueError, match="F has 2 rows"):
        C(sc3, obj, F=np.ones((2, 6)), g=np.ones(3))
    with pytest.raises(ValueError, match="not finite"):
        C(sc3, obj, F=np.ones((2, 6)), g=np.array([1.0, np.nan]))
    with pytest.raises(ValueError, match="not finite"):
        C(sc3, obj, F=np.full((2, 6), np.inf), g=np.ones(2))
    # against the problem's sizes: in BatchTOPPRA's constructor
    with pytest.raises(ValueError, match="chain has 4 joints"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc4, obj, force=0.5)])
    with pytest.raises(ValueError, match="per trajectory for 5"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, obj, force=np.tile([-1.0, 1.0], (5, 3, 1)))])
    with pytest.raises(ValueError, match="leading shape"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, obj, F=np.ones((5, 2, 6)), g=np.ones(2))])
    with pytest.raises(ValueError, match="leading shape"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, obj, F=np.ones((2, 6)), g=np.ones((3, 12, 2)))])
    qs = np.random.default_rng(0).standard_normal((3, 11, 3))
    with pytest.raises(ValueError, match="path positions"):
        algorithm.BatchTOPPRA.from_path_samples(data["grid"], None, qs, qs, data["vlim"], data["alim"], constraints=[C(sc3, obj, force=0.5)])
    with pytest.raises(NotImplementedError, match="BatchTOPPRA"):
        C(sc3, obj, force=0.5).compute_constraint_params(None, None)
    with pytest.raises(NotImplementedError, match="BatchToolWrenchConstraint are supported"):
        algorithm.BatchTOPPRA(*args, constraints=[constraint.JointAccelerationConstraint(data["alim"][0])])
    # a valid list passes the constructor, beside the other chain constraints (its launches come later, on first use)
    taulim = np.stack([-np.ones(3), np.ones(3)], -1)
    inst = algorithm.BatchTOPPRA(*args, constraints=[
        constraint.BatchJointTorqueConstraint(sc3.with_payload(obj), taulim, np.zeros(3)), C(sc3, obj, force=50.0),
        constraint.BatchCartesianAccelerationConstraint(sc3, linear=0.5), constraint.BatchCartesianVelocityNormConstraint(sc3, 0.25)])
    assert len(inst.constraints) == 3 and len(inst.first_order) == 1
    algorithm.BatchTOPPRA.from_path_samples(data["grid"], qs, qs, qs, data["vlim"], data["alim"],
                                            constraints=[C.surface_contact(sc3, obj, 0.5, (0.1, 0.1))])


def test_the_122_row_limit_is_refused_before_any_launch():
    """25 dof, acceleration limits and the 16 contact rows under Interpolation: 2 + 100 + 32 = 134 rows per stage."""
    from toppra_amd import algorithm, constraint
    d = 25
    sc, obj = chain_ref.serial_chain(chain_ref.random_chain(d, 5)), twr.payload_of(tw.PAYLOAD, None)
    data, args = _problem(B=2, d=d, N=6)
    con = constraint.BatchToolWrenchConstraint.surface_contact(sc, obj, 0.5, (0.1, 0.1))
    with pytest.raises(NotImplementedError, match="134 constraint rows"):
        algorithm.BatchTOPPRA(*args, constraints=[con])
    algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchToolWrenchConstraint.surface_contact(
        sc, obj, 0.5, (0.1, 0.1), discretization_scheme=constraint.DiscretizationType.Collocation)])  # 2 + 100 + 16


def test_array_entries_refuse_wrong_shapes_before_any_launch():
    from toppra_amd import batch
    sc, obj = chain_ref.serial_chain(chain_ref.random_chain(3, 5)), twr.payload_of(tw.PAYLOAD, None)
    q = np.zeros((2, 5, 3))
    with pytest.raises(ValueError, match="chain's dof"):
        batch.chain_tool_wrench_batch(sc, np.zeros((2, 5, 4)), np.zeros((2, 5, 4)), np.zeros((2, 5, 4)), obj)
    with pytest.raises(ValueError, match="shape of q"):
        batch.chain_tool_wrench_batch(sc, q, q, np.zeros((2, 4, 3)), obj)
    with pytest.raises(ValueError, match="shape of q"):
        batch.chain_tool_wrench_terms_batch(sc, q, np.zeros((2, 4, 3)), q, obj)


def test_entries_refuse_without_a_gpu():
    from toppra_amd import _capi
    if _capi.device_count() > 0:
        pytest.skip("a GPU is present")
    sc, obj = chain_ref.serial_chain(chain_ref.random_chain(3, 5)), twr.payload_of(tw.PAYLOAD, None)
    q = np.zeros((2, 5, 3))
    with pytest.raises(_capi.ToppraHipError):
        sc.tool_wrench(q, q, q, obj)
    with pytest.raises(_capi.ToppraHipError):
        sc.tool_wrench_terms(q, q, q, obj)


def test_the_staging_area_needs_no_permission():
    """(6) 3 arrays x 64 rows x (d | 1) doubles, or the three outputs at pitch 7 where that is more (csrc/tpr_chain.hip.inc:
    chain_accel_lds_bytes(d, 3) for the fused kernel): 50 688 bytes at 32 dof, under the 64 KB of dynamic LDS a launch gets
    without an attribute."""
    text = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_chain.hip.inc")).read()
    assert "in = 3 * (size_t)kChainBlock * (size_t)(d | 1), out = (size_t)outputs * kChainBlock * 7" in text
    unit = open(os.path.join(ROOT, "toppra_amd", "csrc", "tpr_chain_tu.hip")).read()
    assert "tpr::chain_tool_wrench_terms_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), tpr::chain_accel_lds_bytes(A->M.d, 3)" in unit
    assert "tpr::chain_tool_wrench_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), tpr::chain_accel_lds_bytes(A->M.d, 1)" in unit
    size = lambda d, outputs: max(3 * 64 * (d | 1), outputs * 64 * 7) * 8  # noqa: E731
    assert max(size(d, o) for d in range(1, 33) for o in (1, 3)) == size(32, 3) == 50688 <= 64 * 1024
    assert size(1, 3) == size(5, 3) == 3 * 64 * 7 * 8  # (up to 5 dof the fused kernel's outputs are the larger part)
    assert size(7, 3) == 3 * 64 * 7 * 8 and size(8, 3) == 3 * 64 * 9 * 8

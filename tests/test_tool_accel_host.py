"""The tool-acceleration limit without a GPU: the numpy reference checked against itself (tests/tool_accel_ref.py), and the
surface of ``BatchCartesianAccelerationConstraint`` -- every refusal happens before anything is launched (this machine has no
GPU: a launch would raise ToppraHipError instead of the expected error)."""
import numpy as np
import pytest

from tests import chain_cases as cc, chain_ref, tool_accel_cases as tc, tool_accel_ref as tar

# Steps of the central difference in (ii), chosen on the CPU: in np.longdouble the truncation error c h^2 of these steps
# stands ten orders above the rounding error 1e-19 / h, and the next term c4 h^4 moves the ratio by about h^2 |q'|^2 < 1e-3.
STEPS = (1e-3, 5e-4)


@pytest.mark.parametrize("d", tc.DOFS)
def test_reference_at_rest_is_the_jacobian(d):
    """(i) acc(q, 0, e_j) = J e_j = the tool velocity for qd = e_j, linear and angular part.  Both sides are evaluated in
    np.longdouble, where they agree to its rounding; the allowance is the case's float64-vs-longdouble yardstick, three orders
    above that and fifteen below a wrong term."""
    chain, q, _, _ = cc.case(d)
    zero = np.zeros_like(q)
    for j in range(d):
        e = np.zeros_like(q)
        e[..., j] = 1.0
        acc = tar.tool_acceleration(chain, q, zero, e, dtype=np.longdouble)
        mag = tar.tool_acceleration(chain, q, zero, e, absolute=True)
        v, w = chain_ref.tool_velocity(chain, q, e, dtype=np.longdouble)
        vel = np.stack(list(v) + list(w), -1)
        f64 = tar.tool_acceleration(chain, q, zero, e)
        yardstick = cc._own_error(f64, acc, mag)
        assert yardstick > 0 or not (mag > 0).any()
        assert cc.metric(acc, vel, mag) <= yardstick, (d, j)


@pytest.mark.parametrize("d", tc.DOFS)
def test_reference_converges_to_the_derivative_of_the_velocity(d):
    """(ii) acc(q, qd, 0) is d/dt of the tool velocity along q(t) = q + t qd: the central difference of
    tool_velocity(q +- h qd, qd) converges to it at second order -- the error at h over the error at h / 2 lies in [3.5, 4.5]."""
    chain, q, qs, _ = cc.case(d)
    ld = np.longdouble
    q, qs = np.asarray(q, dtype=ld), np.asarray(qs, dtype=ld)
    acc = tar.tool_acceleration(chain, q, qs, np.zeros_like(q), dtype=ld)

    def error(h):
        h = ld(h)
        up, dn = (chain_ref.tool_velocity(chain, q + s * h * qs, qs, dtype=ld) for s in (1, -1))
        diff = np.stack([(a - b) / (2 * h) for a, b in zip(list(up[0]) + list(up[1]), list(dn[0]) + list(dn[1]))], -1)
        return float(np.max(np.abs(diff - acc)))
    e1, e2 = error(STEPS[0]), error(STEPS[1])
    print("d %d: error %.3g at h = %g, %.3g at h / 2, ratio %.4f" % (d, e1, STEPS[0], e2, e1 / e2))
    assert e2 > 0 and 3.5 <= e1 / e2 <= 4.5, (d, e1, e2)
    assert np.all(acc[2] == 0)  # the trajectory that stands still


def test_gravity_does_not_enter():
    chain, q, qs, qss = cc.case(7)
    assert np.any(chain["gravity"] != 0) or np.any(cc.case(8)[0]["gravity"] != 0)
    other = dict(chain, gravity=np.array([1.0, 2.0, 3.0]))
    assert np.array_equal(tar.tool_acceleration(chain, q, qs, qss), tar.tool_acceleration(other, q, qs, qss))


def _problem(B=3, d=3, N=10):
    from toppra_amd import batch
    data = batch.make_synthetic_batch(B, d, N, seed=3)
    return data, (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])


def test_the_new_symbols_are_exported():
    from toppra_amd import _capi, batch, chain, constraint
    lib = _capi.load()
    for name in ("tpr_chain_tool_acceleration_batch", "tpr_chain_tool_acceleration_terms_batch"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    assert hasattr(chain.SerialChain, "tool_acceleration") and hasattr(chain.SerialChain, "tool_acceleration_terms")
    assert "chain_tool_acceleration_batch" in batch.__all__ and "chain_tool_acceleration_terms_batch" in batch.__all__
    assert issubclass(constraint.BatchCartesianAccelerationConstraint, constraint._BatchSecondOrder)


def test_rows_per_stage_and_the_rows_of_each_spelling():
    from toppra_amd import constraint
    C, DT = constraint.BatchCartesianAccelerationConstraint, constraint.DiscretizationType
    sc = chain_ref.serial_chain(chain_ref.random_chain(3, 5))
    assert C(sc, linear=0.5).get_discretization_type() == DT.Interpolation  # the reference's default for SecondOrderConstraint
    assert C(sc, linear=0.5).rows_per_stage(3) == 12
    assert C(sc, linear=0.5, discretization_scheme=DT.Collocation).rows_per_stage(3) == 6
    assert C(sc, angular=np.tile([-1.0, 2.0], (3, 1))).rows_per_stage(3) == 12
    assert C(sc, linear=0.5, angular=2.0).rows_per_stage(3) == 24
    assert C(sc, linear=0.5, angular=2.0, discretization_scheme=DT.Collocation).rows_per_stage(3) == 12
    assert C(sc, F=np.ones((5, 6)), g=np.ones(5)).rows_per_stage(3) == 10
    assert C(sc, F=np.ones((4, 11, 5, 6)), g=np.ones((4, 5)), discretization_scheme=DT.Collocation).rows_per_stage(3) == 5
    # the signed identity on each part, g = [upper; -lower]; the linear part first
    con = C(sc, linear=np.array([[-1.0, 2.0], [-3.0, 4.0], [-5.0, 6.0]]), angular=0.25)
    I, Z = np.eye(3), np.zeros((3, 3))
    assert np.array_equal(con.F, np.block([[I, Z], [-I, Z], [Z, I], [Z, -I]]))
    assert np.array_equal(con.g, [2.0, 4.0, 6.0, 1.0, 3.0, 5.0] + [0.25] * 6)
    lim = np.stack([-np.arange(1.0, 13.0).reshape(4, 3), np.arange(2.0, 14.0).reshape(4, 3)], -1)  # [B = 4, 3, 2]
    con = C(sc, linear=0.5, angular=lim)
    assert con.g.shape == (4, 12) and np.array_equal(con.g[1], [0.5] * 6 + [5.0, 6.0, 7.0, 4.0, 5.0, 6.0])
    con.check(4, 10, 3)


def test_the_constraint_refuses_before_any_launch():
    from toppra_amd import algorithm, constraint
    C = constraint.BatchCartesianAccelerationConstraint
    sc3, sc4 = chain_ref.serial_chain(chain_ref.random_chain(3, 5)), chain_ref.serial_chain(chain_ref.random_chain(4, 5))
    data, args = _problem()
    with pytest.raises(ValueError, match="SerialChain"):
        C(lambda q, qd, qdd: q, linear=0.5)
    with pytest.raises(ValueError, match="no limit given"):
        C(sc3)
    with pytest.raises(ValueError, match="not both"):
        C(sc3, linear=0.5, F=np.ones((2, 6)), g=np.ones(2))
    with pytest.raises(ValueError, match="not both"):
        C(sc3, angular=0.5, g=np.ones(2))
    with pytest.raises(ValueError, match="together"):
        C(sc3, F=np.ones((2, 6)))
    with pytest.raises(ValueError, match="together"):
        C(sc3, g=np.ones(2))
    for bad in (np.ones(3), np.ones((3, 3)), np.ones((2, 2)), np.ones((5, 4, 3, 2))):
        with pytest.raises(ValueError, match=r"\[3, 2\]"):
            C(sc3, linear=bad)
        with pytest.raises(ValueError, match=r"\[3, 2\]"):
            C(sc3, angular=bad)
    for bad in (np.nan, np.inf, np.array([[-1.0, 1.0], [-1.0, np.inf], [-1.0, 1.0]])):
        with pytest.raises(ValueError, match="not finite"):
            C(sc3, linear=bad)
    with pytest.raises(ValueError, match="above its upper"):
        C(sc3, linear=-0.5)
    with pytest.raises(ValueError, match="above its upper"):
        C(sc3, angular=np.array([[-1.0, 1.0], [2.0, 1.0], [-1.0, 1.0]]))
    with pytest.raises(ValueError, match="per trajectory for 3 and 4"):
        C(sc3, linear=np.tile([-1.0, 1.0], (3, 3, 1)), angular=np.tile([-1.0, 1.0], (4, 3, 1)))
    with pytest.raises(ValueError, match=r"\[m, 6\]"):
        C(sc3, F=np.ones((2, 3)), g=np.ones(2))
    with pytest.raises(ValueError, match=r"\[m, 6\]"):
        C(sc3, F=np.ones(6), g=np.ones(1))
    with pytest.raises(ValueError, match="g must have shape"):
        C(sc3, F=np.ones((2, 6)), g=np.ones((1, 1, 1, 2)))
    with pytest.raises(ValueError, match="F has 2 rows"):
        C(sc3, F=np.ones((2, 6)), g=np.ones(3))
    with pytest.raises(ValueError, match="not finite"):
        C(sc3, F=np.ones((2, 6)), g=np.array([1.0, np.nan]))
    # against the problem's sizes: in BatchTOPPRA's constructor
    with pytest.raises(ValueError, match="chain has 4 joints"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc4, linear=0.5)])
    with pytest.raises(ValueError, match="per trajectory for 5"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, linear=np.tile([-1.0, 1.0], (5, 3, 1)))])
    with pytest.raises(ValueError, match="leading shape"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, F=np.ones((5, 2, 6)), g=np.ones(2))])
    with pytest.raises(ValueError, match="leading shape"):
        algorithm.BatchTOPPRA(*args, constraints=[C(sc3, F=np.ones((2, 6)), g=np.ones((3, 12, 2)))])
    qs = np.random.default_rng(0).standard_normal((3, 11, 3))
    with pytest.raises(ValueError, match="path positions"):
        algorithm.BatchTOPPRA.from_path_samples(data["grid"], None, qs, qs, data["vlim"], data["alim"], constraints=[C(sc3, linear=0.5)])
    with pytest.raises(NotImplementedError, match="BatchTOPPRA"):
        C(sc3, linear=0.5).compute_constraint_params(None, None)
    # a valid list passes the constructor, beside the other chain constraints (its launches come later, on first use)
    taulim = np.stack([-np.ones(3), np.ones(3)], -1)
    inst = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchJointTorqueConstraint(sc3, taulim, np.zeros(3)), C(sc3, linear=0.5),
                                                     constraint.BatchCartesianVelocityNormConstraint(sc3, 0.25)])
    assert len(inst.constraints) == 2 and len(inst.first_order) == 1
    algorithm.BatchTOPPRA.from_path_samples(data["grid"], qs, qs, qs, data["vlim"], data["alim"], constraints=[C(sc3, linear=0.5, angular=1.0)])


def test_the_122_row_limit_is_refused_before_any_launch():
    """27 dof, acceleration limits and 12 tool-acceleration rows under Interpolation: 2 + 108 + 24 = 134 rows per stage."""
    from toppra_amd import algorithm, constraint
    d = 27
    sc = chain_ref.serial_chain(chain_ref.random_chain(d, 5))
    data, args = _problem(B=2, d=d, N=6)
    con = constraint.BatchCartesianAccelerationConstraint(sc, linear=0.5, angular=1.0)
    with pytest.raises(NotImplementedError, match="134 constraint rows"):
        algorithm.BatchTOPPRA(*args, constraints=[con])
    q = np.zeros((2, 7, d))
    with pytest.raises(NotImplementedError, match="134 constraint rows"):
        algorithm.BatchTOPPRA.from_path_samples(data["grid"], q, q, q, data["vlim"], data["alim"], constraints=[con])
    # ... and 6 rows under Collocation fit: 2 + 108 + 6
    algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchCartesianAccelerationConstraint(
        sc, linear=0.5, discretization_scheme=constraint.DiscretizationType.Collocation)])


def test_array_entries_refuse_wrong_shapes_before_any_launch():
    from toppra_amd import batch
    sc = chain_ref.serial_chain(chain_ref.random_chain(3, 5))
    q = np.zeros((2, 5, 3))
    with pytest.raises(ValueError, match="chain's dof"):
        batch.chain_tool_acceleration_batch(sc, np.zeros((2, 5, 4)), np.zeros((2, 5, 4)), np.zeros((2, 5, 4)))
    with pytest.raises(ValueError, match="shape of q"):
        batch.chain_tool_acceleration_batch(sc, q, q, np.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match="shape of q"):
        batch.chain_tool_acceleration_terms_batch(sc, q, np.zeros((2, 4, 3)), q)


def test_entries_refuse_without_a_gpu():
    from toppra_amd import _capi
    if _capi.device_count() > 0:
        pytest.skip("a GPU is present")
    sc = chain_ref.serial_chain(chain_ref.random_chain(3, 5))
    q = np.zeros((2, 5, 3))
    with pytest.raises(_capi.ToppraHipError):
        sc.tool_acceleration(q, q, q)
    with pytest.raises(_capi.ToppraHipError):
        sc.tool_acceleration_terms(q, q, q)

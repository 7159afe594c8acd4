"""The serial chain on the CPU: the numpy reference (tests/chain_ref.py) against closed forms and against itself, the
reference's JointTorqueConstraint on it against the stored fixtures, and everything SerialChain, the two constraints and the
C-ABI refuse before any launch."""
import ctypes

import numpy as np
import pytest

from tests import chain_cases, chain_ref
from tests.helpers import golden

EPS = np.finfo(np.float64).eps
FIXTURES = ("chain_torque_d6_N40", "chain_torque_d3_N30_interp")


def _close(got, terms):
    """Agreement to rounding level: 64 eps x the sum of the absolute values of the closed form's terms."""
    want = sum(terms)
    scale = sum(np.abs(t) for t in terms)
    assert np.all(np.abs(got - want) <= 64 * EPS * scale), float(np.max(np.abs(got - want) / scale))


def test_planar_two_link_arm():
    m1, m2, l1, l2, r1, r2, I1, I2, g = 1.3, 0.7, 0.8, 0.5, 0.35, 0.2, 0.11, 0.05, 9.81
    chain = {"joint_type": [0, 0], "axis": [[0, 0, 1], [0, 0, 1]], "rot": [np.eye(3)] * 2, "trans": [[0, 0, 0], [l1, 0, 0]],
             "mass": [m1, m2], "com": [[r1, 0, 0], [r2, 0, 0]], "inertia": [[0.01, 0.02, I1, 0, 0, 0], [0.03, 0.01, I2, 0, 0, 0]],
             "gravity": [0, -g, 0], "tool": [l2, 0, 0]}
    rng = np.random.default_rng(0)
    q, qd, qdd = rng.uniform(-3, 3, (3, 200, 2))
    tau = chain_ref.rnea(chain, q, qd, qdd)
    (q1, q2), (d1, d2), (a1, a2) = q.T, qd.T, qdd.T
    h = m2 * l1 * r2 * np.sin(q2)
    M11 = [m1 * r1 ** 2, I1, I2, m2 * l1 ** 2, m2 * r2 ** 2, 2 * m2 * l1 * r2 * np.cos(q2)]
    M12 = [I2, m2 * r2 ** 2, m2 * l1 * r2 * np.cos(q2)]
    M22 = [I2, m2 * r2 ** 2]
    grav2 = m2 * r2 * g * np.cos(q1 + q2)
    _close(tau[:, 0], [t * a1 for t in M11] + [t * a2 for t in M12]
           + [-h * 2 * d1 * d2, -h * d2 ** 2, m1 * r1 * g * np.cos(q1), m2 * l1 * g * np.cos(q1), grav2])
    _close(tau[:, 1], [t * a1 for t in M12] + [t * a2 for t in M22] + [h * d1 ** 2, grav2])
    _close(chain_ref.tool_vsv(chain, q, qd),
           [l1 ** 2 * d1 ** 2, l2 ** 2 * (d1 + d2) ** 2, 2 * l1 * l2 * d1 * (d1 + d2) * np.cos(q2)])
    # the same in extended precision, and the magnitude bounds the value
    ld = chain_ref.rnea(chain, q, qd, qdd, dtype=np.longdouble)
    assert ld.dtype == np.longdouble and np.max(np.abs(ld - tau)) < 1e-13
    assert np.all(chain_ref.rnea(chain, q, qd, qdd, absolute=True) >= np.abs(tau))


def test_cart_pole():
    """Prismatic along x, then revolute about z; the pole's centre of mass at distance l, gravity along -y."""
    mc, mp, l, Ip, g = 2.0, 0.4, 0.6, 0.03, 9.81
    chain = {"joint_type": [1, 0], "axis": [[1, 0, 0], [0, 0, 1]], "rot": [np.eye(3)] * 2, "trans": [[0, 0, 0], [0, 0, 0]],
             "mass": [mc, mp], "com": [[0, 0, 0], [l, 0, 0]], "inertia": [[0.1, 0.1, 0.1, 0, 0, 0], [0.01, 0.02, Ip, 0, 0, 0]],
             "gravity": [0, -g, 0], "tool": [0, 0, 0]}
    rng = np.random.default_rng(1)
    q, qd, qdd = rng.uniform(-3, 3, (3, 200, 2))
    tau = chain_ref.rnea(chain, q, qd, qdd)
    th, thd, (xdd, thdd) = q[:, 1], qd[:, 1], qdd.T
    _close(tau[:, 0], [mc * xdd, mp * xdd, -mp * l * np.sin(th) * thdd, -mp * l * np.cos(th) * thd ** 2])
    _close(tau[:, 1], [mp * l ** 2 * thdd, Ip * thdd, -mp * l * np.sin(th) * xdd, mp * g * l * np.cos(th)])


def test_pendulum_with_tilted_axis_and_rotated_joint_frame():
    rng = np.random.default_rng(2)
    Rj = chain_ref.random_rotation(rng)
    k = rng.standard_normal(3)
    k /= np.linalg.norm(k)
    k /= np.linalg.norm(k)
    c, m, grav = np.array([0.2, -0.1, 0.3]), 1.7, np.array([0.5, -1.0, -9.0])
    A = rng.uniform(-0.3, 0.3, (3, 3))
    I = A @ A.T + 0.02 * np.eye(3)
    chain = {"joint_type": [0], "axis": [k], "rot": [Rj], "trans": [[0.1, 0.2, 0.3]], "mass": [m], "com": [c],
             "inertia": [[I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]], "gravity": grav, "tool": [0, 0, 0]}
    q, qd, qdd = rng.uniform(-3, 3, (3, 200, 1))
    tau = chain_ref.rnea(chain, q, qd, qdd)[:, 0]
    # rotation about a fixed axis: the velocity terms vanish; tau = (k' I k + m |k x c|^2) qdd - m z . (c_w x g)
    kxc = np.cross(k, c)
    cw = (Rj @ (c[:, None] * np.cos(q[:, 0]) + kxc[:, None] * np.sin(q[:, 0]) + (k * (k @ c))[:, None] * (1 - np.cos(q[:, 0])))).T
    z = Rj @ k
    terms = [(k @ I @ k) * qdd[:, 0], m * (kxc @ kxc) * qdd[:, 0]]
    for (i, j, l), sign in (((0, 1, 2), 1), ((1, 2, 0), 1), ((2, 0, 1), 1), ((0, 2, 1), -1), ((1, 0, 2), -1), ((2, 1, 0), -1)):
        terms.append(-m * sign * z[i] * cw[:, j] * grav[l])
    # (c_w itself carries three rounded terms per component: their sizes belong to the sum)
    want, scale = sum(terms), sum(np.abs(t) for t in terms) + m * np.abs(z).sum() * np.abs(c).sum() * 3 * np.abs(grav).sum()
    assert np.all(np.abs(tau - want) <= 64 * EPS * scale)


@pytest.mark.parametrize("d", [2, 5, 9])
def test_mass_matrix_is_symmetric_and_positive_definite(d):
    chain = chain_ref.random_chain(d, seed=40 + d)
    q = np.random.default_rng(d).uniform(-3, 3, (6, d))
    M = chain_ref.mass_matrix(chain, q)
    assert np.max(np.abs(M - np.swapaxes(M, 1, 2))) <= 1e-12 * np.max(np.abs(M))
    assert np.linalg.eigvalsh(0.5 * (M + np.swapaxes(M, 1, 2))).min() > 0
    # ... and tau is affine in qdd with that matrix
    qd, qdd = np.random.default_rng(d + 1).standard_normal((2, 6, d))
    lin = chain_ref.rnea(chain, q, qd, np.zeros_like(q)) + np.einsum("pij,pj->pi", M, qdd)
    assert np.allclose(chain_ref.rnea(chain, q, qd, qdd), lin, rtol=0, atol=1e-11)


def _fixture_chain(fx):
    return {k: fx[k] for k in ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity", "tool")}


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_torque_constraint_on_chain_ref_reproduces_the_fixture(reference, name):
    """The reference's own JointTorqueConstraint and seidel TOPPRA, inv_dyn from chain_ref: the stored w0 / wa / wb, torque rows,
    sd, K and return codes, bit for bit."""
    from toppra_amd.solverwrapper import dense_rows
    ta = reference
    import toppra.algorithm as algo
    import toppra.constraint as constraint
    fx = golden(name)
    chain = _fixture_chain(fx)
    inv_dyn = lambda q, qd, qdd: chain_ref.rnea(chain, q, qd, qdd)  # noqa: E731
    B, d = fx["coef"].shape[0], fx["coef"].shape[3]
    scheme = int(fx["torque_scheme"])
    for b in range(B):
        path = ta.SplineInterpolator(fx["knots"], fx["way"][b])
        assert np.array_equal(path.cspl.c, fx["coef"][b])
        lim = fx["taulim"][b] if fx["taulim"].ndim == 3 else fx["taulim"]
        cons = [constraint.JointVelocityConstraint(fx["vlim"][b]),
                constraint.JointAccelerationConstraint(fx["alim"][b], discretization_scheme=constraint.DiscretizationType.Interpolation),
                constraint.JointTorqueConstraint(inv_dyn, lim, fx["fric"], discretization_scheme=constraint.DiscretizationType(scheme))]
        if scheme == 0:
            a, bb, c = cons[2].compute_constraint_params(path, fx["grid"])[:3]
            assert np.array_equal(a, fx["wa"][b] - fx["w0"][b]) and np.array_equal(bb, fx["wb"][b] - fx["w0"][b])
        rows = dense_rows(cons, path, fx["grid"])
        for k in "abc":
            assert np.array_equal(rows[k][:, 2 + 4 * d:], fx["rows_" + k][b]), (name, b, k)
        inst = algo.TOPPRA(cons, path, gridpoints=fx["grid"], solver_wrapper="seidel")
        sdd, sd, _, K = inst.compute_parameterization(0, 0, return_data=True)
        assert int(fx["status"][b]) == 0 and inst.problem_data.return_code == algo.algorithm.ParameterizationReturnCode.Ok
        assert np.array_equal(sd, fx["sd"][b]) and np.array_equal(sdd, fx["u"][b]) and np.array_equal(K, fx["K"][b])


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_self_consistent(name):
    """No reference needed: the stored w0 / wa / wb are chain_ref's values, every trajectory is feasible, and the stored
    accuracy bound is 16 x a yardstick of rounding size."""
    fx = golden(name)
    chain = _fixture_chain(fx)
    from tests import second_order_ref as sor
    q, qs, qss = sor.path_samples(fx["coef"], fx["breaks"], fx["grid"])
    for key, args in chain_cases.evaluations(q, qs, qss).items():
        assert np.array_equal(chain_ref.rnea(chain, *args), fx[key]), key
    assert np.all(fx["status"] == 0) and np.all(np.isfinite(fx["sd"]))
    assert np.array_equal(fx["acc_bound"], chain_cases.BOUND_FACTOR * fx["acc_yardstick"])
    assert np.all(fx["acc_yardstick"] < 4 * EPS) and float(fx["sd_tol"]) > 0  # (a few roundings relative to the magnitude)


def _chain_args(d=3):
    c = chain_ref.random_chain(d, seed=5)
    return [c["joint_type"], c["axis"], c["rot"], c["trans"], c["mass"], c["com"], c["inertia"]]


def test_serial_chain_accepts_a_valid_model():
    from toppra_amd.chain import SerialChain
    args = _chain_args()
    chain = SerialChain(*args)
    assert chain.dof == 3 and chain.joint_types == ["revolute", "prismatic", "revolute"]
    assert np.array_equal(chain.gravity, [0, 0, -9.81]) and np.array_equal(chain.tool, [0, 0, 0])
    full = np.zeros((3, 3, 3))
    for (r, c), k in {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 0): 3, (0, 2): 4, (2, 0): 4, (1, 2): 5, (2, 1): 5}.items():
        full[:, r, c] = args[6][:, k]
    assert np.array_equal(SerialChain(*(args[:6] + [full])).inertias, args[6])
    assert SerialChain(["r", "p", "revolute"], *args[1:]).joint_types == ["revolute", "prismatic", "revolute"]
    model, keep = chain.c_struct(np.zeros(1))
    assert model.d == 3 and model.axis == chain._host.ctypes.data


@pytest.mark.parametrize("what", ["type", "count", "axis_shape", "axis_unit", "rot_orth", "rot_det", "mass", "nan", "inertia_shape",
                                  "gravity_shape", "too_many"])
def test_serial_chain_validation(what):
    from toppra_amd.chain import SerialChain
    a = [np.array(v, dtype=object if i == 0 else np.float64) for i, v in enumerate(_chain_args())]
    a[0] = list(_chain_args()[0])
    kw = {}
    if what == "type":
        a[0][1] = "spherical"
    elif what == "count":
        a[0] = a[0][:2]
    elif what == "axis_shape":
        a[1] = a[1][:, :2]
    elif what == "axis_unit":
        a[1][0] *= 1.0 + 1e-9
    elif what == "rot_orth":
        a[2][1, 0, 1] += 1e-9
    elif what == "rot_det":
        a[2][2] = np.diag([1.0, 1.0, -1.0])
    elif what == "mass":
        a[4][0] = -1.0
    elif what == "nan":
        a[5][1, 2] = np.inf
    elif what == "inertia_shape":
        a[6] = a[6][:, :5]
    elif what == "gravity_shape":
        kw["gravity"] = [0.0, -9.81]
    elif what == "too_many":
        c = chain_ref.random_chain(33, seed=1)
        a = [c[k] for k in ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia")]
    with pytest.raises(ValueError):
        SerialChain(*a, **kw)


def _spline_problem(B=3, d=3, N=10):
    from toppra_amd import batch
    data = batch.make_synthetic_batch(B, d, N, seed=3)
    return data


def test_constraints_refuse_wrong_shapes_before_any_launch():
    """Nothing here may reach the library: this machine has no GPU, a launch would raise ToppraHipError instead."""
    from toppra_amd import algorithm, constraint
    chain3, chain4 = chain_ref.serial_chain(chain_ref.random_chain(3, 5)), chain_ref.serial_chain(chain_ref.random_chain(4, 5))
    data = _spline_problem()
    args = (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])
    taulim = np.stack([-np.ones(3), np.ones(3)], -1)
    # a chain of another dof than the path
    with pytest.raises(ValueError, match="chain has 4 joints"):
        algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchJointTorqueConstraint(chain4, taulim, np.zeros(3))])
    with pytest.raises(ValueError, match="chain has 4 joints"):
        algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchSecondOrderConstraint.joint_torque_constraint(chain4, taulim, np.zeros(3))])
    with pytest.raises(ValueError, match="chain has 4 joints"):
        algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchCartesianVelocityNormConstraint(chain4, 0.25)])
    # limits per trajectory for another batch size; a limit that is no scalar or vector; a bad S; a negative limit; no chain
    with pytest.raises(ValueError, match="per trajectory for 5"):
        algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchCartesianVelocityNormConstraint(chain3, np.ones(5))])
    with pytest.raises(ValueError):
        constraint.BatchCartesianVelocityNormConstraint(chain3, np.ones((3, 2)))
    with pytest.raises(ValueError):
        constraint.BatchCartesianVelocityNormConstraint(chain3, 0.25, S=np.eye(3))
    with pytest.raises(ValueError):
        constraint.BatchCartesianVelocityNormConstraint(chain3, -1.0)
    with pytest.raises(ValueError, match="> 0"):
        constraint.BatchCartesianVelocityNormConstraint(chain3, [0.1, 0.0, 0.2])  # 0 / 0 at a standstill would be NaN
    with pytest.raises(ValueError):
        constraint.BatchCartesianVelocityNormConstraint(chain3, np.nan)
    with pytest.raises(ValueError, match="symmetric"):
        constraint.BatchCartesianVelocityNormConstraint(chain3, 0.25, S=np.triu(np.ones((6, 6))))
    with pytest.raises(ValueError, match="semi-definite"):
        constraint.BatchCartesianVelocityNormConstraint(chain3, 0.25, S=np.diag([1.0, 1, 1, 1, 1, -1]))
    constraint.BatchCartesianVelocityNormConstraint(chain3, 0.25, S=np.diag([1.0, 1, 1, 0, 0, 0]))  # semi-definite is fine
    with pytest.raises(ValueError):
        constraint.BatchCartesianVelocityNormConstraint(lambda q, qd, qdd: q, 0.25)
    # a sampled batch without positions
    qs = np.random.default_rng(0).standard_normal((3, 11, 3))
    with pytest.raises(ValueError, match="path positions"):
        algorithm.BatchTOPPRA.from_path_samples(data["grid"], None, qs, qs, data["vlim"], data["alim"],
                                                constraints=[constraint.BatchCartesianVelocityNormConstraint(chain3, 0.25)])
    # a valid list passes the constructor (its launches come later, on first use)
    inst = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchJointTorqueConstraint(chain3, taulim, np.zeros(3)),
                                                     constraint.BatchCartesianVelocityNormConstraint(chain3, [0.1, 0.2, 0.3])])
    assert len(inst.constraints) == 1 and len(inst.first_order) == 1


def test_array_entries_refuse_wrong_shapes_before_any_launch():
    from toppra_amd import batch
    chain = chain_ref.serial_chain(chain_ref.random_chain(3, 5))
    q = np.zeros((2, 5, 3))
    with pytest.raises(ValueError, match="chain's dof"):
        batch.chain_inverse_dynamics_batch(chain, np.zeros((2, 5, 4)), np.zeros((2, 5, 4)), np.zeros((2, 5, 4)))
    with pytest.raises(ValueError, match="shape of q"):
        batch.chain_torque_terms_batch(chain, q, q, np.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match=r"\[6, 6\]"):
        batch.chain_tool_bound_batch(chain, q, q, None, np.eye(3))
    with pytest.raises(ValueError, match=r"\[B, N\+1, d\]"):
        batch.chain_tool_bound_batch(chain, q[0], q[0], 0.25)
    with pytest.raises(ValueError, match=r"limit must be a scalar or have shape \[B\]"):
        batch.chain_tool_bound_batch(chain, q, q, np.ones(3))
    with pytest.raises(ValueError, match="> 0"):
        batch.chain_tool_bound_batch(chain, q, q, 0.0)
    with pytest.raises(ValueError, match="semi-definite"):
        batch.chain_tool_bound_batch(chain, q, q, None, -np.eye(6))


def test_tpr_chain_bytes_matches_the_binding():
    from toppra_amd import _capi
    lib = _capi.load()
    assert lib.tpr_chain_bytes() == ctypes.sizeof(_capi.tpr_chain) == 2 * 4 + 9 * 8
    assert _capi.tpr_chain.joint_type.offset == 8 and _capi.tpr_chain.tool.offset == 8 + 8 * 8
    for name in ("tpr_chain_bytes", "tpr_chain_inverse_dynamics_batch", "tpr_chain_torque_terms_batch", "tpr_chain_tool_velocity_batch"):
        assert name in _capi.EXPORTS and hasattr(lib, name)


def test_entries_refuse_without_a_gpu():
    from toppra_amd import _capi
    if _capi.device_count() > 0:
        pytest.skip("a GPU is present")
    chain = chain_ref.serial_chain(chain_ref.random_chain(3, 5))
    q = np.zeros((2, 5, 3))
    with pytest.raises(_capi.ToppraHipError):
        chain.inverse_dynamics(q, q, q)
    with pytest.raises(_capi.ToppraHipError):
        chain.torque_terms(q, q, q)
    with pytest.raises(_capi.ToppraHipError):
        chain.tool_velocity_norm(q, q)
    # ... and the C entries themselves, before a successful tpr_init
    lib = _capi.load()
    model, keep = chain.c_struct(q)
    out = np.zeros_like(q)
    rc = lib.tpr_chain_inverse_dynamics_batch(ctypes.byref(model), 10, q.ctypes.data, q.ctypes.data, q.ctypes.data, out.ctypes.data, 0, None)
    assert rc < 0 and b"tpr_init" in lib.tpr_last_error()

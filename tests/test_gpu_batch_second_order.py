"""BatchTOPPRA(..., constraints=[...]): torque / second-order constraints with a batched inverse-dynamics callback, their dense
rows built on the GPU (tpr_path_eval_batch + tpr_second_order_rows_batch) and every pass served by the dense-row entries --
against the reference's own outputs (tests/golden/dense_*.npz), a numpy restatement of the row arithmetic
(tests/second_order_ref.py) and the single-path classes with their per-gridpoint host callbacks."""
import numpy as np
import pytest

import toppra_amd as ta
from tests import second_order_ref as ref
from tests.helpers import assert_same, dense_fixtures, golden
from toppra_amd import batch
from toppra_amd.algorithm import BatchTOPPRA
from toppra_amd.constraint import BatchJointTorqueConstraint, BatchSecondOrderConstraint, DiscretizationType
from toppra_amd.solverwrapper import dense_rows

pytestmark = pytest.mark.gpu

ROWS = ("a", "b", "c", "low", "high")


def _fixture_instance(fx):
    """The fixture's constraint list for the whole batch: vlim / alim arrays and the batched constraint objects."""
    kinds, DT = str(fx["kinds"]).split(","), DiscretizationType(int(fx["scheme"]))
    model = ref.batched_torque_model(fx["mass"], fx["grav"], fx["cori"])
    taulim = np.stack([-fx["taumax"], fx["taumax"]], axis=-1)
    vlim = np.stack([-fx["vmax"], fx["vmax"]], axis=-1) if "vel" in kinds else None
    alim = np.stack([-fx["amax"], fx["amax"]], axis=-1) if "acc" in kinds else None
    cons = []
    for kind in kinds:
        if kind == "torque":
            cons.append(BatchJointTorqueConstraint(model, taulim, fx["fric"], discretization_scheme=DT))
        elif kind == "second":
            cons.append(BatchSecondOrderConstraint.joint_torque_constraint(model, taulim, fx["fric"], discretization_scheme=DT))
    return BatchTOPPRA.from_waypoints(fx["knots"], fx["way"], fx["grid"], vlim, alim, constraints=cons,
                                      interpolation=bool(int(fx["scheme"])))


def _assert_rows(inst, want, what):
    got = dict(zip(ROWS + ("deltas",), inst.dense_rows()))
    for k in ROWS:
        assert_same(got[k], want[k], "%s: %s" % (what, k))
    return got


@pytest.mark.parametrize("name", dense_fixtures())
def test_fixture_rows_and_every_pass(gpu, name):
    """The four reference-generated fixtures (vel,torque / torque / vel,acc,second x 2; both discretisations; failing
    trajectories in two): rows, K, sd, u, status, feasible / controllable / reachable sets and the TOPPRAsd fields, bit
    for bit, from waypoints and a batched numpy callback."""
    fx = golden(name)
    inst = _fixture_instance(fx)
    got = _assert_rows(inst, fx, name)
    B, N = fx["a"].shape[0], fx["a"].shape[1] - 1
    assert_same(got["deltas"], np.broadcast_to(fx["deltas"], (B, N)), "deltas")
    res = inst.compute_parameterization(fx["sd_start"], fx["sd_end"])
    assert np.array_equal(res["status"], fx["status"])
    for k in ("K", "sd", "u"):
        assert_same(res[k], fx[k], k)
    assert_same(inst.compute_feasible_sets(), fx["X"], "X")
    assert_same(inst.compute_controllable_sets(np.full(B, float(fx["sdmin_c"])), np.full(B, float(fx["sdmax_c"]))), fx["Kc"],
                "controllable sets")
    assert_same(inst.compute_reachable_sets(np.zeros(B), np.full(B, 0.3)), fx["L"], "reachable sets")
    assert_same(inst.compute_reachable_sets(np.full(B, 0.1), np.full(B, 0.1)), fx["L_point"], "reachable sets from a point")
    sd = inst.compute_parameterization_sd(fx["sd_desired"], fx["sd_start"], fx["sd_end"])
    assert np.array_equal(sd["status"], fx["sd_status"])
    for k in ("K", "sd", "u"):
        assert_same(sd[k], fx["sd_" + k], "TOPPRAsd " + k)


def test_fixture_rows_with_three_constraint_kinds(gpu):
    """dense_reuse_d5_N60 (vel, acc, torque under Interpolation): rows only."""
    fx = golden("dense_reuse_d5_N60")
    _assert_rows(_fixture_instance(fx), fx, "dense_reuse_d5_N60")


def _poly_model(mass, grav, cori):
    """A multiply / add only dynamics model (no transcendental, no fused op): the same expression for numpy arrays, torch
    tensors and the scalars of one gridpoint."""
    return lambda q, qd, qdd: mass * qdd + cori * q * (1.0 + qd * qd) + grav * q


def test_device_tensors_at_chip_size(gpu):
    """4096 x 7 x 100 as torch tensors on the device, the callback in torch (separate multiply and add ops): rows against
    the numpy restatement, then 32 sampled trajectories -- rows and results -- against the single-path route
    (solverwrapper.dense_rows + TOPPRA with the scalar callback), bit for bit."""
    import torch
    dev = torch.device("cuda:0")
    B, d, N = 4096, 7, 100
    data = batch.make_synthetic_batch(B, d, N, seed=91)
    rng = np.random.default_rng(92)
    mass, grav, cori = 1.0 + rng.random((B, d)), 0.5 * rng.standard_normal((B, d)), 0.3 * rng.standard_normal((B, d))
    taumax, fric = 20.0 + 20.0 * rng.random((B, d)), 0.1 * rng.random((B, d))
    taulim = np.stack([-taumax, taumax], axis=-1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    calls = []

    def model_t(q, qd, qdd):
        calls.append((q.is_cuda, tuple(q.shape)))
        return _poly_model(t(mass)[:, None, :], t(grav)[:, None, :], t(cori)[:, None, :])(q, qd, qdd)

    con = BatchJointTorqueConstraint(model_t, t(taulim), t(fric), discretization_scheme=DiscretizationType.Interpolation)
    inst = BatchTOPPRA(t(data["coef"]), t(data["breaks"]), t(data["grid"]), t(data["vlim"]), None, constraints=[con])
    rows = inst.dense_rows()
    assert all(r.is_cuda for r in rows) and calls == [(True, (B, N + 1, d))] * 3
    assert inst.dense_rows() is rows and len(calls) == 3  # built once per object
    pe = batch.path_eval_batch(t(data["coef"]), t(data["breaks"]), t(data["grid"]))
    q, qs, qss = ref.path_samples(data["coef"], data["breaks"], data["grid"])
    for k, want in (("q", q), ("qs", qs), ("qss", qss)):
        assert_same(pe[k].cpu().numpy(), want, "path samples " + k)
    model_n = _poly_model(mass[:, None, :], grav[:, None, :], cori[:, None, :])
    z = np.zeros_like(q)
    blk = dict(w0=model_n(q, z, z), wa=model_n(q, z, qs), wb=model_n(q, qs, qss), F=None,
               g=np.concatenate((taumax, taumax), -1), friction=fric, interpolation=True)
    want = ref.dense_problem(data["coef"], data["breaks"], data["grid"], data["vlim"], None, True, [blk])
    got = {k: v.cpu().numpy() for k, v in zip(ROWS + ("deltas",), rows)}
    for k in ROWS + ("deltas",):
        assert_same(got[k], want[k], "restatement: " + k)
    res = {k: v.cpu().numpy() for k, v in inst.compute_parameterization().items()}
    X = inst.compute_feasible_sets().cpu().numpy()
    assert (res["status"] == 0).sum() > B // 2
    for b in rng.choice(B, 32, replace=False):
        path = ta.SplineInterpolator(data["knots"], data["waypoints"][b])
        cons = [ta.constraint.JointVelocityConstraint(data["vlim"][b]),
                ta.constraint.JointTorqueConstraint(_poly_model(mass[b], grav[b], cori[b]), taulim[b], fric[b],
                                                    discretization_scheme=DiscretizationType.Interpolation)]
        single = dense_rows(cons, path, data["grid"])
        for k in ROWS:
            assert_same(got[k][b], single[k], "single path %d: %s" % (b, k))
        sdd, sd, _, K = ta.algorithm.TOPPRA(cons, path, gridpoints=data["grid"]).compute_parameterization(0, 0, return_data=True)
        assert_same(res["K"][b], K, "K[%d]" % b)
        if res["status"][b] == 0:
            assert_same(res["sd"][b], sd, "sd[%d]" % b)
            assert_same(res["u"][b], sdd, "u[%d]" % b)
        else:
            assert sd is None
        assert_same(X[b], ta.algorithm.TOPPRA(cons, path, gridpoints=data["grid"]).compute_feasible_sets(), "X[%d]" % b)


def _dense_F_case(per_point, scheme, seed):
    """B paths, d = p = 4, F with m = 6 rows (two of them a single +-1 entry), dry friction.  Returns the batched pieces
    and a factory of the single-path constraint of trajectory b."""
    B, d, N, m = 12, 4, 30, 6
    data = batch.make_synthetic_batch(B, d, N, seed=seed)
    rng = np.random.default_rng(seed + 1)
    mass, grav, cori = 1.0 + rng.random((B, d)), 0.5 * rng.standard_normal((B, d)), 0.3 * rng.standard_normal((B, d))
    fric = 0.1 * rng.random((B, d))
    F0 = rng.standard_normal((B, m, d))
    F0[:, 0] = 0.0; F0[:, 0, 1] = 1.0
    F0[:, 3] = 0.0; F0[:, 3, 2] = -1.0
    unit = np.zeros((m, 1), dtype=bool); unit[[0, 3]] = True
    g0 = 15.0 + 10.0 * rng.random((B, m))
    model = ref.batched_torque_model(mass, grav, cori)
    if per_point:  # callables of q: [B, N+1, d] -> [B, N+1, m, d] / [B, N+1, m]
        F = lambda q: np.where(unit, F0[:, None], F0[:, None] * (1.0 + 0.1 * q[:, :, 0])[:, :, None, None])  # noqa: E731
        g = lambda q: g0[:, None] * (1.0 + 0.05 * q[:, :, 1])[:, :, None]  # noqa: E731
    else:
        F, g = F0, g0

    def single(b):
        inv = lambda q, qd, qdd: mass[b] * qdd + cori[b] * np.sin(q) * (1 + qd * qd) + grav[b] * np.cos(q)  # noqa: E731
        if per_point:
            cF = lambda q: np.where(unit, F0[b], F0[b] * (1.0 + 0.1 * q[0]))  # noqa: E731
            cg = lambda q: g0[b] * (1.0 + 0.05 * q[1])  # noqa: E731
        else:
            cF, cg = (lambda q: F0[b]), (lambda q: g0[b])
        return ta.constraint.SecondOrderConstraint(inv, cF, cg, d, custom_term=lambda path, s: np.sign(path(s, 1)) * fric[b],
                                                   discretization_scheme=scheme)
    con = BatchSecondOrderConstraint(model, F, g, friction=fric, discretization_scheme=scheme)
    return data, con, single, unit[:, 0]


@pytest.mark.parametrize("per_point,scheme", [(False, DiscretizationType.Collocation), (True, DiscretizationType.Interpolation)])
def test_dense_F_against_the_single_path_rows(gpu, per_point, scheme):
    """Dense F per trajectory ([B, m, p]) and per gridpoint (a callable of q), m != 2 p, against solverwrapper.dense_rows on
    SecondOrderConstraint: rows of F with a single +-1 entry bit for bit; general rows within the dot product's rounding
    bound 2 p 2^-53 sum_k |F_k x_k| + 2^-52 |want| (the host's BLAS fixes neither order nor fusion, the kernel sums in index
    order: both sides are only known to that bound).  The solve is compared on the GPU-built rows (the wiring)."""
    data, con, single, unit = _dense_F_case(per_point, scheme, seed=101 + int(per_point))
    inst = BatchTOPPRA(data["coef"], data["breaks"], data["grid"], data["vlim"], None, constraints=[con])
    got = dict(zip(ROWS + ("deltas",), inst.dense_rows()))
    B, d = data["coef"].shape[0], data["coef"].shape[3]
    halves = 2 if scheme == DiscretizationType.Interpolation else 1
    unit_cols = 2 + np.flatnonzero(np.tile(unit, halves))
    worst = 0.0
    for b in range(B):
        path = ta.SplineInterpolator(data["knots"], data["waypoints"][b])
        cons = [ta.constraint.JointVelocityConstraint(data["vlim"][b]), single(b)]
        want = dense_rows(cons, path, data["grid"])
        pa, pb, pc, pF, pg = want["params"][1][:5]
        for k in ("low", "high"):
            assert_same(got[k][b], want[k], "%s[%d]" % (k, b))
        for k, x in (("a", pa), ("b", pb), ("c", pc)):
            assert_same(got[k][b][:, unit_cols], want[k][:, unit_cols], "%s[%d], rows of F with one +-1 entry" % (k, b))
            mag = np.abs(pF * x[:, None, :]).sum(-1)  # sum_k |F_k x_k| per gridpoint and row
            bound = 2 * pF.shape[-1] * 2.0 ** -53 * mag + 2.0 ** -52 * np.abs(want[k][:, 2:])
            err = np.abs(got[k][b][:, 2:] - want[k][:, 2:])
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (k, b, float(np.max(err - bound)))
    print("dense F, per_point=%s: worst error / bound = %.3f" % (per_point, worst))
    res = inst.compute_parameterization()
    direct = batch.solve_dense_batch(*inst.dense_rows(), want_sd=True)
    for k in ("sd2", "sd", "u", "K", "status"):
        assert_same(res[k], direct[k], "wiring: " + k)
    assert (res["status"] == 0).any()


def test_per_trajectory_grids_two_constraints_and_trajectories(gpu):
    """Per-trajectory grids [B, N+1], a torque constraint (Collocation) and a second-order constraint (Interpolation) in
    one list: rows against the numpy restatement, compute_trajectory (both parametrizers) and compute_trajectory_samples
    bit for bit against param_spline_batch / const_accel_times_batch / param_spline_sample_batch on the sd of
    compute_parameterization."""
    B, d, N = 48, 5, 60
    data = batch.make_synthetic_batch(B, d, N, seed=111)
    rng = np.random.default_rng(112)
    cuts = np.sort(rng.random((B, N - 1)), axis=1) * 0.9 + 0.05
    grid = np.concatenate((np.zeros((B, 1)), 0.5 * cuts + 0.5 * np.linspace(0, 1, N + 1)[None, 1:-1], np.ones((B, 1))), axis=1)
    assert np.all(np.diff(grid, axis=1) > 0)
    mass, grav, cori = 1.0 + rng.random((B, d)), 0.5 * rng.standard_normal((B, d)), 0.3 * rng.standard_normal((B, d))
    taumax, fric = 12.0 + 6.0 * rng.random((B, d)), 0.1 * rng.random((B, d))
    taulim = np.stack([-taumax, taumax], axis=-1)
    model = ref.batched_torque_model(mass, grav, cori)
    model2 = ref.batched_torque_model(0.5 * mass, grav, 2.0 * cori)
    cons = [BatchJointTorqueConstraint(model, taulim, fric),
            BatchSecondOrderConstraint.joint_torque_constraint(model2, taulim[0], fric[0])]
    assert cons[0].get_discretization_type() == DiscretizationType.Collocation
    assert cons[1].get_discretization_type() == DiscretizationType.Interpolation
    inst = BatchTOPPRA(data["coef"], data["breaks"], grid, data["vlim"], data["alim"], constraints=cons)
    q, qs, qss = ref.path_samples(data["coef"], data["breaks"], grid)
    z = np.zeros_like(q)
    blocks = [dict(w0=model(q, z, z), wa=model(q, z, qs), wb=model(q, qs, qss), F=None, g=np.concatenate((taumax, taumax), -1),
                   friction=fric, interpolation=False),
              dict(w0=model2(q, z, z), wa=model2(q, z, qs), wb=model2(q, qs, qss), F=None,
                   g=np.concatenate((taumax[0], taumax[0])), friction=fric[0], interpolation=True)]
    want = ref.dense_problem(data["coef"], data["breaks"], grid, data["vlim"], data["alim"], True, blocks)
    got = _assert_rows(inst, want, "two constraints")
    assert got["a"].shape[2] == 2 + 4 * d + 2 * d + 4 * d
    assert_same(got["deltas"], want["deltas"], "deltas")
    res = inst.compute_parameterization()
    assert (res["status"] == 0).sum() > B // 2
    traj = inst.compute_trajectory()
    sp = batch.param_spline_batch(data["coef"], data["breaks"], grid, res["sd"])
    for k in ("knot_times", "counts", "coef"):
        assert_same(traj._sp[k], sp[k], "ParametrizeSpline " + k)
    assert np.array_equal(traj.status, res["status"])
    ca = inst.compute_trajectory(parametrizer="ParametrizeConstAccel")
    ts, us = batch.const_accel_times_batch(grid, res["sd"])
    assert_same(ca._ts, ts, "ParametrizeConstAccel ts")
    assert_same(ca._us, us, "ParametrizeConstAccel us")
    times = np.linspace(0, 1, 17)
    smp = inst.compute_trajectory_samples(times, orders=(0, 1, 2))
    direct = batch.param_spline_sample_batch(data["coef"], data["breaks"], grid, res["sd"], times, orders=(0, 1, 2))
    for k in ("q", "qd", "qdd", "duration"):
        assert_same(smp[k], direct[k], "samples " + k)
    assert np.array_equal(smp["status"], res["status"])


def _array_level_case(B, d, N, p, seed):
    data = batch.make_synthetic_batch(B, d, N, seed=seed)
    rng = np.random.default_rng(seed + 1)
    w = [rng.standard_normal((B, N + 1, p)) for _ in range(3)]
    return data, rng, dict(w0=w[0], wa=w[1], wb=w[2])


def _assert_array_level(data, vlim, alim, interp, blocks, what):
    got = batch.second_order_rows_batch(data["coef"], data["breaks"], data["grid"], vlim, alim, blocks, interp)
    want = ref.dense_problem(data["coef"], data["breaks"], data["grid"], vlim, alim, interp, blocks)
    for k in ROWS + ("deltas",):
        assert_same(got[k], want[k], "%s: %s" % (what, k))
    return got


@pytest.mark.parametrize("interp", [False, True])
def test_F_shared_by_the_batch(gpu, interp):
    """F [m, p], one for the whole batch (TPR_SO_F_SHARED), p != d, g [m]: batch.second_order_rows_batch against the numpy
    restatement, which sums a dense row in the kernel's index order: bit for bit."""
    data, rng, blk = _array_level_case(10, 3, 37, 5, seed=121)
    blk.update(F=rng.standard_normal((4, 5)), g=5.0 + rng.random(4), friction=None, interpolation=interp)
    got = _assert_array_level(data, data["vlim"], data["alim"], True, [blk], "shared F")
    assert got["a"].shape[2] == 2 + 4 * 3 + (2 if interp else 1) * 4


@pytest.mark.parametrize("interp", [False, True])
def test_signed_identity_with_g_per_gridpoint(gpu, interp):
    """The signed identity with g [B, N+1, 2 p] (TPR_SO_G_PER_POINT): under Interpolation the second half of a stage reads
    the next gridpoint's g, the last stage its own."""
    data, rng, blk = _array_level_case(9, 4, 33, 4, seed=123)
    blk.update(F=None, g=5.0 + rng.random((9, 34, 8)), friction=0.1 * rng.random((9, 4)), interpolation=interp)
    _assert_array_level(data, data["vlim"], None, True, [blk], "g per gridpoint")


@pytest.mark.parametrize("vel,acc,interp", [(True, True, True), (True, True, False), (True, False, True), (False, False, True)])
def test_no_second_order_block(gpu, vel, acc, interp):
    """An empty block list: the rows of tpr_constraint_params_batch, down to the two zero columns alone."""
    data = batch.make_synthetic_batch(7, 3, 41, seed=125)
    vlim, alim = (data["vlim"] if vel else None), (data["alim"] if acc else None)
    got = _assert_array_level(data, vlim, alim, interp, [], "no block")
    params = batch.constraint_params_batch(data["coef"], data["breaks"], data["grid"], vlim, alim, interp)
    for k in ROWS:
        assert_same(got[k], params[k], "constraint_params: " + k)


def test_wide_blocks_shrink_the_tile(gpu):
    """Blocks wide enough that a 32-gridpoint tile does not fit the kernel's LDS budget (p = 200 and p = 60: the tile
    shrinks to 4 gridpoints), N + 1 not a multiple of the tile, per-trajectory F and a shared one."""
    data, rng, blk = _array_level_case(5, 3, 45, 200, seed=127)
    blk.update(F=rng.standard_normal((5, 3, 200)), g=5.0 + rng.random((5, 3)), friction=None, interpolation=True)
    w = [rng.standard_normal((5, 46, 60)) for _ in range(3)]
    blk2 = dict(w0=w[0], wa=w[1], wb=w[2], F=rng.standard_normal((7, 60)), g=rng.random(7), friction=None, interpolation=False)
    got = _assert_array_level(data, data["vlim"], data["alim"], False, [blk, blk2], "wide blocks")
    assert got["a"].shape[2] == 2 + 2 * 3 + 6 + 7


def test_numpy_problem_keeps_its_rows_on_the_device(gpu):
    """numpy in: dense_rows() hands out host arrays, the passes read a device copy made once and return numpy arrays."""
    fx = golden("dense_torque_only_d3_N30")
    inst = _fixture_instance(fx)
    res = inst.compute_parameterization(fx["sd_start"], fx["sd_end"])
    assert all(isinstance(v, np.ndarray) for v in res.values()) and all(isinstance(r, np.ndarray) for r in inst.dense_rows())
    assert all(r.is_cuda for r in inst._rows_dev)
    dev = inst._rows_dev
    inst.compute_feasible_sets()
    assert inst._rows_dev is dev

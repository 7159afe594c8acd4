#!/usr/bin/env python
"""Generate the control-point fixtures tests/golden/control_points_*.npz by running the REAL reference (hungpham2511/toppra):
its SecondOrderConstraint with inv_dyn = the numpy accelerations of the control points stacked [3 P] (tests/control_points_cases.py:
the tool acceleration of tests/tool_accel_ref.py on the chain cut after each point's link; one gridpoint per call, as the
reference calls it), F = the signed identity on every point's three components and g the limits, in [JointVelocityConstraint,
JointAccelerationConstraint, that] through TOPPRA(solver_wrapper="seidel"), one trajectory at a time; and
profiles/control_points_accuracy.json.

    python tools/make_control_points_golden.py        # needs the reference; builds oracle/_ref on demand

It follows tools/make_tool_accel_golden.py: B = 4; data only -- the chain's parameters, the points, waypoints, coefficient tables,
grid and limits; the reference's wa, wb [B, N+1, 3 P], the dense rows of its constraint (the columns after the acceleration
block), low, high, sd, u, K and return codes; and the two tolerances of the GPU tests --
  acc_yardstick / acc_bound [2]: the error of the float64 reference against np.longdouble on the fixture's own wa, wb, in the
      metric of tests/chain_cases.py, and 16 x that;
  sd_tol: 4 x the largest change of sd over 20 seeds when wa, wb are disturbed by noise of the size of the accuracy bound
      (each uniform in +- its acc_bound x its magnitude; w0 is an exact zero and is not disturbed) and the problem is solved by
      the CPU restatement under oracle/.
The limits are chosen here, on the CPU: a fraction of each point's largest acceleration along the reference's own solution
WITHOUT the constraint -- so the constraint is active (the reference's sd differs from its sd without it) -- and positive on
both sides, so standing still satisfies it and every trajectory stays feasible.  Both are asserted.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

from oracle import oracle as orc, ref_loader  # noqa: E402
from tests import chain_cases, chain_ref, control_points_cases as cp, second_order_ref as sor  # noqa: E402

ta = ref_loader.load()
if ta is None:
    raise SystemExit("reference not available")
import toppra.algorithm as algo  # noqa: E402
import toppra.constraint as constraint  # noqa: E402
from toppra.algorithm.algorithm import ParameterizationReturnCode as RC  # noqa: E402

STATUS = {RC.Ok: 0, RC.FailUncontrollable: 1, RC.ErrUnknown: 2}
CHAIN_KEYS = ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity", "tool")


def signed_identity(P):
    """F [6 P, 3 P]: [I; -I] on each point's three components, the points in order."""
    F = np.zeros((6 * P, 3 * P))
    for p in range(P):
        F[6 * p:6 * p + 3, 3 * p:3 * p + 3], F[6 * p + 3:6 * p + 6, 3 * p:3 * p + 3] = np.eye(3), -np.eye(3)
    return F


def fixture(name, B, d, N, seed, scheme, links, per_traj):
    rng = np.random.default_rng(seed)
    chain = chain_ref.random_chain(d, seed=seed + 1, gravity=True, prismatic_every=4)
    links = np.array(links, dtype=np.int64)
    P = len(links)
    offsets = rng.uniform(-0.25, 0.25, (P, 3))
    inv_dyn = lambda q, qd, qdd: cp.point_accelerations(chain, links, offsets, q, qd, qdd).reshape(q.shape[:-1] + (3 * P,))  # noqa: E731
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    way = rng.uniform(-1.5, 1.5, (B, 5, d))
    vmax, amax = 2.0 + 2.0 * rng.random((B, d)), 6.0 + 4.0 * rng.random((B, d))
    vlim, alim = np.stack([-vmax, vmax], -1), np.stack([-amax, amax], -1)
    paths = [ta.SplineInterpolator(knots, way[b]) for b in range(B)]
    q, qs, qss = (np.stack([p(grid, k) for p in paths]) for k in (0, 1, 2))
    zero = np.zeros(d)
    w0 = np.array([[inv_dyn(q_, zero, zero) for q_ in q[b]] for b in range(B)])
    wa = np.array([[inv_dyn(q_, zero, s_) for q_, s_ in zip(q[b], qs[b])] for b in range(B)])
    wb = np.array([[inv_dyn(q_, s_, ss_) for q_, s_, ss_ in zip(q[b], qs[b], qss[b])] for b in range(B)])
    assert not w0.any(), "acc(q, 0, 0) is an exact zero"
    DT = constraint.DiscretizationType(scheme)
    acc_dt = constraint.DiscretizationType.Interpolation

    def base_constraints(b):
        return [constraint.JointVelocityConstraint(vlim[b]), constraint.JointAccelerationConstraint(alim[b], discretization_scheme=acc_dt)]

    # the reference without the constraint, and every point's acceleration along its solution
    free_sd, peak = [], []
    for b in range(B):
        inst = algo.TOPPRA(base_constraints(b), paths[b], gridpoints=grid, solver_wrapper="seidel")
        sdd, sd, _ = inst.compute_parameterization(0, 0)
        assert sd is not None
        free_sd.append(sd)
        along = wa[b, :-1] * sdd[:, None] + wb[b, :-1] * (sd[:-1] ** 2)[:, None]
        peak.append(np.abs(along).reshape(-1, P, 3).max((0, 2)))
    peak = np.array(peak)  # [B, P]
    # per trajectory [B, P, 3, 2], or one [P, 3, 2] for the batch; lower and upper limits of different size
    if per_traj:
        hi = 0.5 * peak[:, :, None] * (1.0 + 0.2 * rng.random((B, P, 3)))
    else:
        hi = 0.5 * peak.min(0)[:, None] * (1.0 + 0.2 * rng.random((P, 3)))
    linear = np.stack([-hi * (1.0 + 0.2 * rng.random(hi.shape)), hi], -1)
    F = signed_identity(P)
    g = np.concatenate((linear[..., 1], -linear[..., 0]), -1).reshape(hi.shape[:-2] + (6 * P,))  # [B, 6 P] or [6 P]
    g_of = (lambda b: g[b]) if per_traj else (lambda b: g)

    out = {k: [] for k in ("rows_a", "rows_b", "rows_c", "low", "high", "K", "sd", "u", "status")}
    from toppra_amd.solverwrapper import dense_rows
    for b in range(B):
        cons = base_constraints(b) + [constraint.SecondOrderConstraint(inv_dyn, lambda q_: F, lambda q_, b=b: g_of(b), dof=d,
                                                                       discretization_scheme=DT)]
        inst = algo.TOPPRA(cons, paths[b], gridpoints=grid, solver_wrapper="seidel")
        sdd, sd, _, K = inst.compute_parameterization(0, 0, return_data=True)
        st = STATUS[inst.problem_data.return_code]
        assert st == 0 and sd is not None, "%s: trajectory %d is not feasible in the reference (status %d)" % (name, b, st)
        assert not np.array_equal(sd, free_sd[b]), "%s: the constraint is not active in trajectory %d" % (name, b)
        print("%s trajectory %d: largest sd %.4f, without the constraint %.4f" % (name, b, sd.max(), free_sd[b].max()))
        rows = dense_rows(cons, paths[b], grid)
        first = 2 + 4 * d  # (the x_next pair, the acceleration block under Interpolation)
        for k in "abc":
            out["rows_" + k].append(rows[k][:, first:])
        out["low"].append(rows["low"]); out["high"].append(rows["high"])
        out["K"].append(K); out["sd"].append(sd); out["u"].append(sdd); out["status"].append(st)
    rec = {k: np.stack(v) for k, v in out.items()}
    rec["status"] = rec["status"].astype(np.int32)
    coef = np.stack([np.asarray(p.cspl.c) for p in paths])
    breaks = np.asarray(paths[0].cspl.x)

    # the accuracy yardstick on the fixture's own inputs
    ref = cp.reference_of(chain, links, offsets, q, qs, qss)
    flat = lambda v: v.reshape(v.shape[:-2] + (3 * P,))  # noqa: E731
    assert all(np.array_equal(flat(ref[k]), v) for k, v in (("wa", wa), ("wb", wb))), "batched reference differs from per-point calls"
    yard = np.array([ref["yardstick"][k] for k in ("wa", "wb")])
    bound = chain_cases.BOUND_FACTOR * yard

    # the end-to-end tolerance of sd: the CPU restatement on rows from disturbed wa, wb
    gB = g if per_traj else np.broadcast_to(g, (B, 6 * P))
    block = {"F": F, "g": gB, "friction": None, "interpolation": bool(scheme)}

    def solve(va, vb):
        rows = sor.dense_problem(coef, breaks, grid, vlim, alim, True, [dict(block, w0=w0, wa=va, wb=vb)])
        return orc.solve_dense_batch(*(rows[k] for k in ("a", "b", "c", "low", "high", "deltas")))
    base = solve(wa, wb)
    assert np.array_equal(base["status"], rec["status"]) and np.array_equal(base["sd"], rec["sd"]), "the restatement differs from the reference"
    worst = 0.0
    for s in range(20):
        nrng = np.random.default_rng(1000 + s)
        noisy = [v + bd * flat(ref[k + "_mag"]) * nrng.uniform(-1.0, 1.0, v.shape) for bd, (k, v) in zip(bound, (("wa", wa), ("wb", wb)))]
        got = solve(*noisy)
        assert np.array_equal(got["status"], rec["status"])
        worst = max(worst, float(np.max(np.abs(got["sd"] - base["sd"]))))
    rec.update({k: np.asarray(chain[k]) for k in CHAIN_KEYS})
    rec.update(links=links, offsets=offsets, knots=knots, way=way, coef=coef, breaks=breaks, grid=grid, vlim=vlim, alim=alim, linear=linear,
               F=F, g=g, wa=wa, wb=wb, scheme=np.array(scheme), acc_yardstick=yard, acc_bound=bound, sd_tol=np.array(4.0 * worst))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)
    print(name, "rows", rec["rows_a"].shape, "status", np.bincount(rec["status"], minlength=3), "acc_bound", bound,
          "sd_tol %.3g" % (4.0 * worst), "%.0f KB" % (os.path.getsize(os.path.join(OUT, name + ".npz")) / 1024))
    return {"yardstick": dict(zip(("wa", "wb"), yard.tolist())), "bound": dict(zip(("wa", "wb"), bound.tolist())), "sd_tol": 4.0 * worst}


if __name__ == "__main__":
    fixtures = {"control_points_d6_N40": fixture("control_points_d6_N40", 4, 6, 40, 511, 1, [2, -1, 2], True),
                "control_points_d4_N30_colloc": fixture("control_points_d4_N30_colloc", 4, 4, 30, 512, 0, [-1, 0, 1, 1], False)}
    path = os.path.join(ROOT, "profiles", "control_points_accuracy.json")
    measured = {}
    if os.path.exists(path):  # (what the kernels were measured to use is written by the GPU run, not here: keep it)
        with open(path) as fh:
            measured = json.load(fh).get("measured", {})
    with open(path, "w") as fh:
        json.dump({"metric": "|got - ref| / (|ref| with every product and sum in absolute value); yardstick = the float64 numpy "
                             "recursion on the chain cut after each point's link (tests/control_points_cases.py) against "
                             "np.longdouble on the same inputs; bound = %g x yardstick" % chain_cases.BOUND_FACTOR,
                   "cases": cp.accuracy_table(), "fixtures": fixtures, "measured": measured}, fh, indent=1, sort_keys=True)
        fh.write("\n")

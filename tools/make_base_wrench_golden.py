#!/usr/bin/env python
"""Generate the base-reaction fixtures tests/golden/base_wrench_*.npz by running the REAL reference (hungpham2511/toppra): its
SecondOrderConstraint with inv_dyn = the numpy base wrench of tests/base_wrench_ref.py (one gridpoint per call, as the reference
calls it) in [JointVelocityConstraint, JointAccelerationConstraint, that] through TOPPRA(solver_wrapper="seidel"), one trajectory
at a time; and profiles/base_wrench_accuracy.json.

    python tools/make_base_wrench_golden.py        # needs the reference; builds oracle/_ref on demand

It follows tools/make_tool_wrench_golden.py: B = 4; data only -- the robot's and the mount's parameters, waypoints, coefficient
tables, grid and limits; the reference's w0, wa, wb, the dense rows of its constraint (the columns after the acceleration block),
low, high, sd, u, K and return codes; and the two tolerances of the GPU tests --
  acc_yardstick / acc_bound [3]: the error of the float64 reference against np.longdouble on the fixture's own w0, wa, wb, in the
      metric of tests/chain_cases.py, and 16 x that;
  sd_tol: 4 x the largest change of sd over 20 seeds when w0, wa, wb are disturbed by noise of the size of the accuracy bound
      (each uniform in +- its acc_bound x its magnitude) and the problem is solved by the CPU restatement under oracle/.
Two fixtures:
  base_wrench_torso_d15_N30: a torso joint that carries two 7-dof arms, on a cart (a platform under the base, the mount frame on
      the floor), BatchBaseWrenchConstraint.surface_contact's 16 rows -- the cart must not tip, slide or spin --, Interpolation:
      2 + 60 + 32 = 94 rows per stage.
  base_wrench_d4_N30_colloc: the SCARA of tools/make_tool_wrench_golden.py on a pedestal, the mount frame at the pedestal's foot,
      a force / moment box (the flange's data sheet), Collocation.  The box is chosen here, on the CPU, per trajectory: the largest
      static |w0| along the path plus half of the largest dynamic part |w - w0| along the reference's own solution WITHOUT the
      constraint -- standing still satisfies it with room, and it is active.
Feasibility of every trajectory and that the constraint is active (the reference's sd differs from its sd without it) are asserted.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden")

from oracle import oracle as orc, ref_loader  # noqa: E402
from tests import base_wrench_cases, base_wrench_ref, chain_cases, second_order_ref as sor, tree_cases, tree_ref  # noqa: E402

ta = ref_loader.load()
if ta is None:
    raise SystemExit("reference not available")
import toppra.algorithm as algo  # noqa: E402
import toppra.constraint as constraint  # noqa: E402
from toppra.algorithm.algorithm import ParameterizationReturnCode as RC  # noqa: E402

from make_tool_wrench_golden import scara  # noqa: E402

STATUS = {RC.Ok: 0, RC.FailUncontrollable: 1, RC.ErrUnknown: 2}
ROBOT_KEYS = ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity", "parent")
MOUNT_KEYS = ("rot", "origin", "mass", "com")
NAMES = ("w0", "wa", "wb")
I3, Z3 = np.eye(3), np.zeros((3, 3))
F_BOX = np.block([[I3, Z3], [-I3, Z3], [Z3, I3], [Z3, -I3]])


def torso_on_a_cart():
    """tests/tree_cases.py's torso shape with tree_ref.random_tree's links under gravity, its base 0.6 m above the floor on a
    40 kg cart whose centre of mass lies low; the mount frame is the floor under the base (normal +z)."""
    tree = tree_ref.random_tree(tree_cases.SHAPES["torso"], seed=77, gravity=True, massless=None)
    tree["gravity"] = np.array([0.0, 0.0, -9.81])
    mount = {"rot": np.eye(3), "origin": np.array([0.0, 0.0, -0.6]), "mass": 40.0, "com": np.array([0.02, -0.01, -0.45])}
    return tree, mount


def scara_on_a_pedestal():
    chain = {k: v for k, v in scara().items() if k != "tool"}
    chain["parent"] = np.arange(4, dtype=np.int32) - 1
    tilt = 0.1  # (the pedestal's flange is not quite level)
    rot = np.array([[np.cos(tilt), 0.0, np.sin(tilt)], [0.0, 1.0, 0.0], [-np.sin(tilt), 0.0, np.cos(tilt)]])
    return chain, {"rot": rot, "origin": np.array([0.05, 0.0, -0.8]), "mass": 0.0, "com": np.zeros(3)}


def fixture(name, B, N, seed, scheme, contact):
    rng = np.random.default_rng(seed)
    robot, mount = torso_on_a_cart() if contact else scara_on_a_pedestal()
    d = len(robot["parent"])
    inv_dyn = lambda q, qd, qdd: base_wrench_ref.base_wrench(robot, q, qd, qdd, mount)  # noqa: E731
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    way = rng.uniform(-1.5, 1.5, (B, 5, d))
    if contact:
        way *= 0.5
    else:
        way[..., 2] *= 0.1  # (the lift: +- 15 cm)
    vmax, amax = 2.0 + 2.0 * rng.random((B, d)), 6.0 + 4.0 * rng.random((B, d))
    vlim, alim = np.stack([-vmax, vmax], -1), np.stack([-amax, amax], -1)
    paths = [ta.SplineInterpolator(knots, way[b]) for b in range(B)]
    q, qs, qss = (np.stack([p(grid, k) for p in paths]) for k in (0, 1, 2))
    zero = np.zeros(d)
    w0 = np.array([[inv_dyn(q_, zero, zero) for q_ in q[b]] for b in range(B)])
    wa = np.array([[inv_dyn(q_, zero, s_) for q_, s_ in zip(q[b], qs[b])] for b in range(B)])
    wb = np.array([[inv_dyn(q_, s_, ss_) for q_, s_, ss_ in zip(q[b], qs[b], qss[b])] for b in range(B)])
    DT = constraint.DiscretizationType(scheme)
    acc_dt = constraint.DiscretizationType.Interpolation

    def base_constraints(b):
        return [constraint.JointVelocityConstraint(vlim[b]), constraint.JointAccelerationConstraint(alim[b], discretization_scheme=acc_dt)]

    # the reference without the constraint, and the dynamic part of the wrench along its solution
    free_sd, along = [], []
    for b in range(B):
        inst = algo.TOPPRA(base_constraints(b), paths[b], gridpoints=grid, solver_wrapper="seidel")
        sdd, sd, _ = inst.compute_parameterization(0, 0)
        assert sd is not None
        free_sd.append(sd)
        along.append((wa[b, :-1] - w0[b, :-1]) * sdd[:, None] + (wb[b, :-1] - w0[b, :-1]) * (sd[:-1] ** 2)[:, None])
    extra = {}
    if contact:
        from toppra_amd.constraint import BatchToolWrenchConstraint
        mu, half = 0.5, (0.30, 0.25)
        F, g1 = BatchToolWrenchConstraint.surface_contact_rows(mu, half)
        g = np.broadcast_to(g1, (B, F.shape[0])).copy()
        extra = {"mu": np.array(mu), "half_extents": np.array(half)}
    else:
        F = F_BOX
        static = np.abs(w0).max(1)  # [B, 6]
        dynamic = np.stack([np.abs(along[b]).max(0) for b in range(B)])
        hi = static + 0.5 * dynamic
        g = np.concatenate((hi[:, :3], hi[:, :3], hi[:, 3:], hi[:, 3:]), -1)  # [upper; -lower] per part, the force first
    assert np.all(np.einsum("mk,bnk->bnm", F, w0) < g[:, None, :]), "%s: standing still violates the limits" % name

    out = {k: [] for k in ("rows_a", "rows_b", "rows_c", "low", "high", "K", "sd", "u", "status")}
    from toppra_amd.solverwrapper import dense_rows
    for b in range(B):
        cons = base_constraints(b) + [constraint.SecondOrderConstraint(inv_dyn, lambda q_: F, lambda q_, b=b: g[b], dof=d,
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
    ref = base_wrench_cases.reference_of(robot, mount, q, qs, qss)
    assert all(np.array_equal(ref[k], v) for k, v in zip(NAMES, (w0, wa, wb))), "batched reference differs from per-point calls"
    yard = np.array([ref["yardstick"][k] for k in NAMES])
    bound = chain_cases.BOUND_FACTOR * yard

    # the end-to-end tolerance of sd: the CPU restatement on rows from disturbed w0, wa, wb
    block = {"F": F, "g": g, "friction": None, "interpolation": bool(scheme)}

    def solve(v0, va, vb):
        rows = sor.dense_problem(coef, breaks, grid, vlim, alim, True, [dict(block, w0=v0, wa=va, wb=vb)])
        return orc.solve_dense_batch(*(rows[k] for k in ("a", "b", "c", "low", "high", "deltas")))
    base = solve(w0, wa, wb)
    # (the reference forms F a, F b, F c with numpy's dot, whose summation order is the BLAS's, the restatement and the kernels
    # sum a row in index order -- the rows agree to rounding, not in bits, and so does sd; the gap must vanish in sd_tol)
    gap = float(np.max(np.abs(base["sd"] - rec["sd"])))
    assert np.array_equal(base["status"], rec["status"]), "the restatement's return codes differ from the reference's"
    worst = 0.0
    for s in range(20):
        nrng = np.random.default_rng(1000 + s)
        noisy = [v + bd * ref[k + "_mag"] * nrng.uniform(-1.0, 1.0, v.shape) for bd, k, v in zip(bound, NAMES, (w0, wa, wb))]
        got = solve(*noisy)
        assert np.array_equal(got["status"], rec["status"])
        worst = max(worst, float(np.max(np.abs(got["sd"] - base["sd"]))))
    print("%s: restatement vs reference sd %.3g, sd_tol %.3g" % (name, gap, 4.0 * worst))
    assert gap <= worst, "%s: the restatement differs from the reference by more than the disturbance moves it" % name
    rec.update({k: np.asarray(robot[k]) for k in ROBOT_KEYS})
    rec.update({"mount_" + k: np.asarray(mount[k], dtype=np.float64) for k in MOUNT_KEYS})
    rec.update(knots=knots, way=way, coef=coef, breaks=breaks, grid=grid, vlim=vlim, alim=alim, F=F, g=g, w0=w0, wa=wa, wb=wb,
               scheme=np.array(scheme), acc_yardstick=yard, acc_bound=bound, sd_tol=np.array(4.0 * worst), **extra)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)
    print(name, "rows", rec["rows_a"].shape, "status", np.bincount(rec["status"], minlength=3), "acc_bound", bound,
          "sd_tol %.3g" % (4.0 * worst), "%.0f KB" % (os.path.getsize(os.path.join(OUT, name + ".npz")) / 1024))
    return {"yardstick": dict(zip(NAMES, yard.tolist())), "bound": dict(zip(NAMES, bound.tolist())), "sd_tol": 4.0 * worst}


if __name__ == "__main__":
    fixtures = {"base_wrench_torso_d15_N30": fixture("base_wrench_torso_d15_N30", 4, 30, 618, 1, True),
                "base_wrench_d4_N30_colloc": fixture("base_wrench_d4_N30_colloc", 4, 30, 612, 0, False)}
    path = os.path.join(ROOT, "profiles", "base_wrench_accuracy.json")
    measured = {}
    if os.path.exists(path):  # (what the kernels were measured to use is written by the GPU run, not here: keep it)
        with open(path) as fh:
            measured = json.load(fh).get("measured", {})
    with open(path, "w") as fh:
        json.dump({"metric": "|got - ref| / (|ref| with every product and sum in absolute value); yardstick = float64 "
                             "tests/base_wrench_ref.py against np.longdouble on the same inputs; bound = %g x yardstick"
                             % chain_cases.BOUND_FACTOR,
                   "cases": base_wrench_cases.accuracy_table(), "fixtures": fixtures, "measured": measured}, fh, indent=1, sort_keys=True)
        fh.write("\n")

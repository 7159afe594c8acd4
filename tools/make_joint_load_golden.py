#!/usr/bin/env python
"""Generate the joint-load fixtures tests/golden/joint_load_*.npz by running the REAL reference (hungpham2511/toppra): its
SecondOrderConstraint with inv_dyn = the numpy joint wrenches of tests/joint_load_ref.py, flattened section-major (one gridpoint
per call, as the reference calls it) in [JointVelocityConstraint, JointAccelerationConstraint, that] through
TOPPRA(solver_wrapper="seidel"), one trajectory at a time; and profiles/joint_load_accuracy.json.

    python tools/make_joint_load_golden.py        # needs the reference; builds oracle/_ref on demand

It follows tools/make_base_wrench_golden.py: B = 4; data only -- the robot's and the sections' parameters, waypoints, coefficient
tables, grid and limits; the reference's w0, wa, wb [B, N+1, S, 6], the dense rows of its constraint (the columns after the
acceleration block), low, high, sd, u, K and return codes; and the two tolerances of the GPU tests --
  acc_yardstick / acc_bound [3]: the error of the float64 reference against np.longdouble on the fixture's own w0, wa, wb, in the
      metric of tests/chain_cases.py, and 16 x that;
  sd_tol: 4 x the largest change of sd over 20 seeds when w0, wa, wb are disturbed by noise of the size of the accuracy bound
      (each uniform in +- its acc_bound x its magnitude) and the problem is solved by the CPU restatement under oracle/.
Two fixtures, sized within the 122 rows of a stage:
  joint_load_torso_d15_N30: a torso joint that carries two 7-dof arms, JointSections.on_axes at the first joint of each arm (the
      shoulder bearings, their centres 4 cm along the axes), BatchJointLoadConstraint.bearing's rows with sides = 6 -- 14 rows per
      section --, Interpolation: 2 + 60 + 56 = 118 rows per stage.  The limits are chosen here, on the CPU, one per section for the
      whole batch: the largest static norm along the paths plus a share of the largest dynamic part along the reference's own
      solutions WITHOUT the constraint, over cos(pi / sides) -- standing still satisfies the polygon with room.
  joint_load_d4_N30_colloc: the SCARA of tools/make_tool_wrench_golden.py, sections at joint 1 (the elbow bearing) and at the
      prismatic joint (a linear guide's carriage), force / moment boxes chosen per trajectory as base_wrench_d4_N30_colloc chooses
      its box, Collocation.
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
from tests import chain_cases, joint_load_cases, joint_load_ref, second_order_ref as sor, tree_cases, tree_ref  # noqa: E402

ta = ref_loader.load()
if ta is None:
    raise SystemExit("reference not available")
import toppra.algorithm as algo  # noqa: E402
import toppra.constraint as constraint  # noqa: E402
from toppra.algorithm.algorithm import ParameterizationReturnCode as RC  # noqa: E402

from make_tool_wrench_golden import scara  # noqa: E402

STATUS = {RC.Ok: 0, RC.FailUncontrollable: 1, RC.ErrUnknown: 2}
ROBOT_KEYS = ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity", "parent")
NAMES = ("w0", "wa", "wb")
SIDES = 6


def torso_with_shoulder_bearings():
    """tests/tree_cases.py's torso shape with tree_ref.random_tree's links under gravity; the sections are the bearings of the
    arms' first joints (links 1 and 8), z along the joint axes, their centres 4 cm along them."""
    from toppra_amd.chain import JointSections
    tree = tree_ref.random_tree(tree_cases.SHAPES["torso"], seed=77, gravity=True, massless=None)
    tree["gravity"] = np.array([0.0, 0.0, -9.81])
    sections = JointSections.on_axes(tree_ref.kinematic_tree(tree), [1, 8], 0.04)
    return tree, {"link": np.asarray(sections.joints, dtype=np.int64), "rot": np.array(sections.rotations), "origin": np.array(sections.origins)}


def scara_with_a_linear_guide():
    chain = {k: v for k, v in scara().items() if k != "tool"}
    chain["parent"] = np.arange(4, dtype=np.int32) - 1
    return chain, {"link": np.array([1, 2], dtype=np.int64), "rot": np.tile(np.eye(3), (2, 1, 1)),
                   "origin": np.array([[0.0, 0.0, 0.05], [0.0, 0.0, -0.05]])}


def fixture(name, B, N, seed, scheme, bearing):
    rng = np.random.default_rng(seed)
    robot, sec = torso_with_shoulder_bearings() if bearing else scara_with_a_linear_guide()
    d, S = len(robot["parent"]), len(sec["link"])
    inv_dyn = lambda q, qd, qdd: joint_load_ref.joint_wrenches(robot, q, qd, qdd, sec).reshape(np.shape(q)[:-1] + (6 * S,))  # noqa: E731
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    way = rng.uniform(-1.5, 1.5, (B, 5, d))
    if bearing:
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

    # the reference without the constraint, and the wrenches along its solution
    free_sd, along = [], []
    for b in range(B):
        inst = algo.TOPPRA(base_constraints(b), paths[b], gridpoints=grid, solver_wrapper="seidel")
        sdd, sd, _ = inst.compute_parameterization(0, 0)
        assert sd is not None
        free_sd.append(sd)
        along.append(w0[b, :-1] + (wa[b, :-1] - w0[b, :-1]) * sdd[:, None] + (wb[b, :-1] - w0[b, :-1]) * (sd[:-1] ** 2)[:, None])
    from toppra_amd.constraint import BatchJointLoadConstraint, _section_limits
    extra = {}
    static = w0.reshape(B, N + 1, S, 6)
    moving = [a.reshape(N, S, 6) for a in along]
    if bearing:
        norm = lambda x, at: np.sqrt(x[..., at] ** 2 + x[..., at + 1] ** 2)  # noqa: E731
        share, lims = 0.35, {}
        for key, at in (("tilting", 3), ("radial", 0)):
            rest = norm(static, at).max((0, 1))  # [S]
            peak = np.max([norm(m, at).max(0) for m in moving], 0)
            lims[key] = (rest + share * np.maximum(peak - rest, 0.0)) / np.cos(np.pi / SIDES)
        rest = np.abs(static[..., 2]).max((0, 1))
        peak = np.max([np.abs(m[..., 2]).max(0) for m in moving], 0)
        lims["axial"] = rest + share * np.maximum(peak - rest, 0.0)
        F, g1 = BatchJointLoadConstraint.bearing_rows(S, lims["tilting"], lims["axial"], lims["radial"], SIDES)
        g = np.broadcast_to(g1, (B, F.shape[0])).copy()
        extra = dict(lims, sides=np.array(SIDES))
    else:
        rest = np.abs(static).max(1)  # [B, S, 6]
        dynamic = np.stack([np.abs(m - static[b, :-1]).max(0) for b, m in enumerate(moving)])
        hi = rest + 0.5 * dynamic
        force, moment = np.stack([-hi[..., :3], hi[..., :3]], -1), np.stack([-hi[..., 3:], hi[..., 3:]], -1)  # [B, S, 3, 2]
        F, g, _ = _section_limits(S, force, moment, None, None)
        extra = {"force": force, "moment": moment}
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
        assert rows["a"].shape[1] <= 122, rows["a"].shape
        for k in "abc":
            out["rows_" + k].append(rows[k][:, first:])
        out["low"].append(rows["low"]); out["high"].append(rows["high"])
        out["K"].append(K); out["sd"].append(sd); out["u"].append(sdd); out["status"].append(st)
    rec = {k: np.stack(v) for k, v in out.items()}
    rec["status"] = rec["status"].astype(np.int32)
    coef = np.stack([np.asarray(p.cspl.c) for p in paths])
    breaks = np.asarray(paths[0].cspl.x)

    # the accuracy yardstick on the fixture's own inputs
    ref = joint_load_cases.reference_of(robot, sec, q, qs, qss)
    shaped = lambda v: v.reshape(B, N + 1, S, 6)  # noqa: E731
    assert all(np.array_equal(ref[k], shaped(v)) for k, v in zip(NAMES, (w0, wa, wb))), "batched reference differs from per-point calls"
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
        noisy = [v + bd * ref[k + "_mag"].reshape(v.shape) * nrng.uniform(-1.0, 1.0, v.shape) for bd, k, v in zip(bound, NAMES, (w0, wa, wb))]
        got = solve(*noisy)
        assert np.array_equal(got["status"], rec["status"])
        worst = max(worst, float(np.max(np.abs(got["sd"] - base["sd"]))))
    print("%s: restatement vs reference sd %.3g, sd_tol %.3g" % (name, gap, 4.0 * worst))
    assert gap <= worst, "%s: the restatement differs from the reference by more than the disturbance moves it" % name
    rec.update({k: np.asarray(robot[k]) for k in ROBOT_KEYS})
    rec.update({"section_" + k: np.asarray(sec[k]) for k in ("link", "rot", "origin")})
    rec.update(knots=knots, way=way, coef=coef, breaks=breaks, grid=grid, vlim=vlim, alim=alim, F=F, g=g, w0=shaped(w0), wa=shaped(wa),
               wb=shaped(wb), scheme=np.array(scheme), acc_yardstick=yard, acc_bound=bound, sd_tol=np.array(4.0 * worst), **extra)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)
    print(name, "rows", rec["rows_a"].shape, "status", np.bincount(rec["status"], minlength=3), "acc_bound", bound,
          "sd_tol %.3g" % (4.0 * worst), "%.0f KB" % (os.path.getsize(os.path.join(OUT, name + ".npz")) / 1024))
    return {"yardstick": dict(zip(NAMES, yard.tolist())), "bound": dict(zip(NAMES, bound.tolist())), "sd_tol": 4.0 * worst}


if __name__ == "__main__":
    fixtures = {"joint_load_torso_d15_N30": fixture("joint_load_torso_d15_N30", 4, 30, 718, 1, True),
                "joint_load_d4_N30_colloc": fixture("joint_load_d4_N30_colloc", 4, 30, 712, 0, False)}
    path = os.path.join(ROOT, "profiles", "joint_load_accuracy.json")
    measured = {}
    if os.path.exists(path):  # (what the kernels were measured to use is written by the GPU run, not here: keep it)
        with open(path) as fh:
            measured = json.load(fh).get("measured", {})
    with open(path, "w") as fh:
        json.dump({"metric": "|got - ref| / (|ref| with every product and sum in absolute value); yardstick = float64 "
                             "tests/joint_load_ref.py against np.longdouble on the same inputs; bound = %g x yardstick; restatement = "
                             "the share of the bound the float64 link-local restatement (the kernels' order) uses on the CPU"
                             % chain_cases.BOUND_FACTOR,
                   "recipe": {"chosen": joint_load_cases.RECIPE,
                              "worst_restatement_fraction_with_gravity": joint_load_cases.worst_restatement(True),
                              "worst_restatement_fraction_without_gravity": joint_load_cases.worst_restatement(False)},
                   "cases": joint_load_cases.accuracy_table(), "fixtures": fixtures, "measured": measured}, fh, indent=1, sort_keys=True)
        fh.write("\n")

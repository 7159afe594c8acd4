#!/usr/bin/env python
"""Generate the tree fixtures tests/golden/tree_torque_*.npz by running the REAL reference (hungpham2511/toppra): its
JointTorqueConstraint and TOPPRA(solver_wrapper="seidel") with inv_dyn taken from tests/tree_ref.py (the numpy recursion over a
kinematic tree, one gridpoint per call as the reference calls it), and profiles/tree_dynamics_accuracy.json.

    python tools/make_tree_golden.py        # needs the reference; builds oracle/_ref on demand

Modelled on tools/make_chain_golden.py, whose procedure for the two tolerances is followed exactly.  Each fixture holds data
only: the tree's parameters and parent table, the paths' waypoints and coefficient tables, grid and limits; the reference's w0,
wa, wb, the dense rows of its torque constraint (the columns after the acceleration block), sd, u, K and return codes; and
  acc_yardstick / acc_bound [3]: the error of the float64 tree_ref against np.longdouble on the fixture's own w0, wa, wb, in the
      metric of tests/chain_cases.py, and 16 x that;
  sd_tol: 4 x the largest change of sd over 20 seeds when w0, wa, wb are disturbed by noise of the size of the accuracy bound
      (each of the three uniform in +- its acc_bound x its magnitude) and the problem is solved by the CPU restatement.
Every trajectory must be feasible in the reference: asserted here.

The torso fixture takes the torque limits under Interpolation and the acceleration limits under Collocation: 4 d + 2 d = 90 rows
per stage at 15 dof and the x and x_next pairs, 94 as the reference's dense rows count them (92 as BatchTOPPRA counts, which takes
the x pair as a box): under the 122 the dense-row kernels hold.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

from oracle import oracle as orc, ref_loader  # noqa: E402
from tests import second_order_ref as sor, tree_cases, tree_ref  # noqa: E402

ta = ref_loader.load()
if ta is None:
    raise SystemExit("reference not available")
import toppra.algorithm as algo  # noqa: E402
import toppra.constraint as constraint  # noqa: E402
from toppra.algorithm.algorithm import ParameterizationReturnCode as RC  # noqa: E402

STATUS = {RC.Ok: 0, RC.FailUncontrollable: 1, RC.ErrUnknown: 2}
TREE_KEYS = ("parent", "joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity")


def fixture(name, B, shape, N, seed, torque_scheme, accel_scheme, per_traj_limits):
    rng = np.random.default_rng(seed)
    tree = tree_ref.random_tree(tree_cases.SHAPES[shape], seed=seed + 1, gravity=True, prismatic_every=4)
    d = len(tree["parent"])
    inv_dyn = lambda q, qd, qdd: tree_ref.rnea(tree, q, qd, qdd)  # noqa: E731
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    way = rng.uniform(-1.5, 1.5, (B, 5, d))
    vmax, amax = 2.0 + 2.0 * rng.random((B, d)), 6.0 + 4.0 * rng.random((B, d))
    vlim, alim = np.stack([-vmax, vmax], -1), np.stack([-amax, amax], -1)
    fric = 0.05 * rng.random(d)
    paths = [ta.SplineInterpolator(knots, way[b]) for b in range(B)]
    q, qs, qss = (np.stack([p(grid, k) for p in paths]) for k in (0, 1, 2))
    zero = np.zeros(d)
    w0 = np.array([[inv_dyn(q_, zero, zero) for q_ in q[b]] for b in range(B)])
    wa = np.array([[inv_dyn(q_, zero, s_) for q_, s_ in zip(q[b], qs[b])] for b in range(B)])
    wb = np.array([[inv_dyn(q_, s_, ss_) for q_, s_, ss_ in zip(q[b], qs[b], qss[b])] for b in range(B)])
    # limits that leave every trajectory feasible: the torque of standing still anywhere on the paths, and headroom to move
    hold = np.abs(w0).max(axis=(0, 1))
    taumax = 1.2 * hold + 1.0 + rng.random((B, d) if per_traj_limits else d)
    taulim = np.stack([-taumax, taumax], -1)  # [d, 2] shared or [B, d, 2]
    DT = constraint.DiscretizationType(torque_scheme)
    out = {k: [] for k in ("rows_a", "rows_b", "rows_c", "low", "high", "K", "sd", "u", "status")}
    from toppra_amd.solverwrapper import dense_rows
    for b in range(B):
        lim = taulim[b] if per_traj_limits else taulim
        cons = [constraint.JointVelocityConstraint(vlim[b]),
                constraint.JointAccelerationConstraint(alim[b], discretization_scheme=constraint.DiscretizationType(accel_scheme)),
                constraint.JointTorqueConstraint(inv_dyn, lim, fric, discretization_scheme=DT)]
        inst = algo.TOPPRA(cons, paths[b], gridpoints=grid, solver_wrapper="seidel")
        sdd, sd, _, K = inst.compute_parameterization(0, 0, return_data=True)
        st = STATUS[inst.problem_data.return_code]
        assert st == 0 and sd is not None, "%s: trajectory %d is not feasible in the reference (status %d)" % (name, b, st)
        rows = dense_rows(cons, paths[b], grid)
        first = 2 + (4 if accel_scheme else 2) * d  # (the x_next pair, the acceleration block)
        for k in "abc":
            out["rows_" + k].append(rows[k][:, first:])
        out["low"].append(rows["low"]); out["high"].append(rows["high"])
        out["K"].append(K); out["sd"].append(sd); out["u"].append(sdd); out["status"].append(st)
        # the constraint's own parameters are tree_ref's values through the reference's expressions
        a, bb, c = cons[2].compute_constraint_params(paths[b], grid)[:3]
        if torque_scheme == 0:
            assert np.array_equal(a, wa[b] - w0[b]) and np.array_equal(bb, wb[b] - w0[b])
    rec = {k: np.stack(v) for k, v in out.items()}
    rec["status"] = rec["status"].astype(np.int32)
    coef = np.stack([np.asarray(p.cspl.c) for p in paths])
    breaks = np.asarray(paths[0].cspl.x)

    # the accuracy yardstick on the fixture's own inputs
    ref = tree_cases.reference_of(tree, q, qs, qss)
    assert all(np.array_equal(ref[k], v) for k, v in (("w0", w0), ("wa", wa), ("wb", wb))), "batched tree_ref differs from per-point calls"
    yard = np.array([ref["yardstick"][k] for k in ("w0", "wa", "wb")])
    bound = tree_cases.BOUND_FACTOR * yard

    # the end-to-end tolerance of sd: the CPU restatement on rows from disturbed w0, wa, wb
    block = {"F": None, "g": np.concatenate((taulim[..., 1], -taulim[..., 0]), -1), "friction": fric,
             "interpolation": bool(torque_scheme)}

    def solve(v0, va, vb):
        rows = sor.dense_problem(coef, breaks, grid, vlim, alim, bool(accel_scheme), [dict(block, w0=v0, wa=va, wb=vb)])
        return orc.solve_dense_batch(*(rows[k] for k in ("a", "b", "c", "low", "high", "deltas")))
    base = solve(w0, wa, wb)
    assert np.array_equal(base["status"], rec["status"]) and np.array_equal(base["sd"], rec["sd"]), "the restatement differs from the reference"
    worst = 0.0
    for s in range(20):
        nrng = np.random.default_rng(1000 + s)
        noisy = [v + bd * ref[k + "_mag"] * nrng.uniform(-1.0, 1.0, v.shape) for bd, (k, v) in zip(bound, (("w0", w0), ("wa", wa), ("wb", wb)))]
        got = solve(*noisy)
        assert np.array_equal(got["status"], rec["status"])
        worst = max(worst, float(np.max(np.abs(got["sd"] - base["sd"]))))
    rec.update({k: np.asarray(tree[k]) for k in TREE_KEYS})
    rec.update(knots=knots, way=way, coef=coef, breaks=breaks, grid=grid, vlim=vlim, alim=alim, taulim=taulim, fric=fric, w0=w0, wa=wa, wb=wb,
               torque_scheme=np.array(torque_scheme), accel_scheme=np.array(accel_scheme), acc_yardstick=yard, acc_bound=bound,
               sd_tol=np.array(4.0 * worst))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)
    print(name, "rows per stage", first + rec["rows_a"].shape[-1] + 2, "torque rows", rec["rows_a"].shape, "status",
          np.bincount(rec["status"], minlength=3), "acc_bound", bound, "sd_tol %.3g" % (4.0 * worst),
          "%.0f KB" % (os.path.getsize(os.path.join(OUT, name + ".npz")) / 1024))
    return {"yardstick": dict(zip(("w0", "wa", "wb"), yard.tolist())), "bound": dict(zip(("w0", "wa", "wb"), bound.tolist())),
            "sd_tol": 4.0 * worst}


if __name__ == "__main__":
    fixtures = {"tree_torque_vee_d3_N30_colloc": fixture("tree_torque_vee_d3_N30_colloc", 4, "vee", 30, 321, 0, 1, True),
                "tree_torque_torso_d15_N30": fixture("tree_torque_torso_d15_N30", 2, "torso", 30, 322, 1, 0, False)}
    with open(os.path.join(ROOT, "profiles", "tree_dynamics_accuracy.json"), "w") as fh:
        json.dump({"metric": "|got - ref| / (|ref| with every product and sum in absolute value); yardstick = float64 tree_ref "
                             "against np.longdouble on the same inputs; bound = %g x yardstick" % tree_cases.BOUND_FACTOR,
                   "cases": tree_cases.accuracy_table(), "fixtures": fixtures}, fh, indent=1, sort_keys=True)
        fh.write("\n")

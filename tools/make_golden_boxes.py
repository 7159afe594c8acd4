#!/usr/bin/env python
"""Generate tests/golden/boxes_*.npz: the REAL reference (hungpham2511/toppra, seidel solver) on constraint lists with
first-order constraints that only tighten the stage boxes -- JointVelocityConstraintVarying, several velocity constraints in
one list, bound-only LinearConstraints (xbound / ubound).

    python tools/make_golden_boxes.py        # build container only: needs the reference, builds oracle/_ref on demand

Four fixtures of 4 trajectories each (a 5-waypoint cubic spline, limits vlim0 (1 + 0.5 sin 9 s)):
  boxes_a  [Varying, Acceleration]                                                   3 dof, N 30
  boxes_b  [JointVelocityConstraint, Varying, Acceleration, bound-only (xbound + ubound)]   9 dof, N 30
  boxes_c  [Acceleration (Collocation), bound-only (xbound)]                       17 dof, N 30
  boxes_d  [Varying, JointTorqueConstraint]                                          7 dof, N 40
Stored per fixture: the spline table and the samples q, qs, qss as the reference's path returned them, vgrid -- the limits as
the reference built them, np.array([vlim_func(s) for s in gridpoints]) -- the bounds, the reference wrapper's own low_arr /
high_arr (read back through solve_stagewise_optim on a wrapper that holds the first-order constraints only: without rows the
LP's optimum is a corner of the box, copied), and the results: the parameterization for (0, 0), for one nonzero pair and for
one uncontrollable start, controllable / feasible / reachable sets, TOPPRAsd at 1.5 x the optimal duration.  Every result comes
from a fresh reference object.  The bound-only constraint is built from the solve WITHOUT it ("free"): x cap = max(0.6
x_free, 1e-3) on 0.3 < s < 0.7 (list b: 0.75 < s < 0.95) and 1e4 elsewhere, u bounds = +-0.5 max |u_free|.

The tool asserts what makes the fixtures binding (tests/stage_boxes_ref.py::binding_conditions; the tests assert it again from
the stored arrays): the varying limit changes the stored (0, 0) sd against the solve of the same list without it at >= 5
gridpoints (and, beside other first-order constraints, the reference's boxes at >= 5 gridpoints), K[:, 1] equals the x cap at >= 5 gridpoints, u equals a
u bound at >= 3 stages, every (0, 0) solve is Ok.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

from oracle import ref_loader  # noqa: E402
from tests import stage_boxes_ref as sbr  # noqa: E402
from tools.rigid_golden import reference_boxes  # noqa: E402  (it lives there, where importing it runs nothing)

ta = ref_loader.load()
if ta is None:
    raise SystemExit("reference not available")
import toppra.algorithm as algo  # noqa: E402
import toppra.constraint as constraint  # noqa: E402
import toppra.parametrizer as tparam  # noqa: E402
from toppra.algorithm.algorithm import ParameterizationReturnCode as RC  # noqa: E402

STATUS = {RC.Ok: 0, RC.FailUncontrollable: 1, RC.ErrUnknown: 2}
B = 4


def solve(cons, path, grid, s0, s1, cls=algo.TOPPRA, desired=None):
    obj = cls(cons, path, gridpoints=grid, solver_wrapper="seidel")
    if desired is not None:
        obj.set_desired_duration(desired)
    sdd, sd, _, K = obj.compute_parameterization(s0, s1, return_data=True)
    st = STATUS[obj.problem_data.return_code]
    N = len(grid) - 1
    if sd is None:
        sd, sdd = np.full(N + 1, np.nan), np.full(N, np.nan)
    return {"sd": sd, "u": sdd, "K": K, "status": np.array(st, dtype=np.int32)}


def fixture(name, kinds, d, N, seed, interpolation=True, sets=(0.0, 1.0), bad_pair=(200.0, 0.0), zone=(0.3, 0.7), ufrac=0.5):
    rng = np.random.default_rng(seed)
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    way = rng.standard_normal((B, 5, d))
    vmax, amax = 1 + 2 * rng.random((B, d)), 2 + 3 * rng.random((B, d))
    f = {"kinds": kinds, "interpolation": interpolation, "knots": knots, "grid": grid, "way": way,
         "vlim0": np.stack([-vmax, vmax], -1), "vlim": np.stack([-vmax, vmax], -1), "alim": np.stack([-amax, amax], -1),
         "sets": np.array(sets), "bad_pair": np.array(bad_pair)}
    if "torque" in kinds:
        f.update(mass=1.0 + rng.random((B, d)), grav=0.5 * rng.standard_normal((B, d)), cori=0.3 * rng.standard_normal((B, d)),
                 taumax=6.0 + 6.0 * rng.random((B, d)), fric=0.1 * rng.random((B, d)))
    paths = [ta.SplineInterpolator(knots, way[b]) for b in range(B)]
    f["coef"] = np.stack([np.asarray(p.cspl.c, dtype=np.float64) for p in paths])
    f["breaks"] = np.asarray(paths[0].cspl.x, dtype=np.float64)
    for k, order in (("q", 0), ("qs", 1), ("qss", 2)):
        f[k] = np.stack([np.asarray(p(grid, order), dtype=np.float64).reshape(N + 1, d) for p in paths])
    if "vary" in kinds:
        f["vgrid"] = np.stack([np.array([sbr.vlim_func(f, b)(s) for s in grid]) for b in range(B)])
    if "bound" in kinds:  # from the solve without the bound-only constraint
        free = [solve(sbr.reference_list(f, b, constraint, skip=("bound",)), paths[b], grid, 0.0, 0.0) for b in range(B)]
        assert all(r["status"] == 0 for r in free)
        inzone = (grid > zone[0]) & (grid < zone[1])
        cap = np.stack([np.where(inzone, np.maximum(0.6 * r["sd"] ** 2, 1e-3), 1e4) for r in free])
        f["xbound"] = np.stack([np.zeros_like(cap), cap], -1)
        if "ubound" in kinds:
            umax = np.stack([np.full(N + 1, ufrac * np.abs(r["u"]).max()) for r in free])
            f["ubound"] = np.stack([-umax, umax], -1)
    f["kinds"] = [k for k in kinds if k != "ubound"]
    rec = {k: [] for k in ("low_ref", "high_ref", "K_set", "X", "L")}
    for b in range(B):
        cons = lambda **kw: sbr.reference_list(f, b, constraint, **kw)  # noqa: E731  (fresh objects for every pass)
        low, high = reference_boxes(cons(), paths[b], grid)
        rec["low_ref"].append(low); rec["high_ref"].append(high)
        inst = lambda: algo.TOPPRA(cons(), paths[b], gridpoints=grid, solver_wrapper="seidel")  # noqa: E731
        rec["K_set"].append(inst().compute_controllable_sets(*sets))
        rec["X"].append(inst().compute_feasible_sets())
        rec["L"].append(inst().compute_reachable_sets(*sets))
        # the nonzero pair: end at 0.01, start in the middle of what is controllable from there
        pair = (0.5 * float(np.sqrt(inst().compute_controllable_sets(0.01, 0.01)[0, 1])), 0.01)
        rec.setdefault("pair", []).append(np.array(pair))
        for tag, (s0, s1) in (("zero", (0.0, 0.0)), ("pair", pair), ("bad", bad_pair)):
            for k, v in solve(cons(), paths[b], grid, s0, s1).items():
                rec.setdefault(tag + "_" + k, []).append(v)
        assert rec["zero_status"][-1] == 0 and rec["pair_status"][-1] == 0 and rec["bad_status"][-1] == 1, (name, b)
        t_opt = tparam.ParametrizeConstAccel(paths[b], grid, rec["zero_sd"][-1]).duration
        rec.setdefault("sd_desired", []).append(1.5 * t_opt)
        for k, v in solve(cons(), paths[b], grid, 0.0, 0.0, algo.TOPPRAsd, 1.5 * t_opt).items():
            rec.setdefault("sd_" + k, []).append(v)
        if "vary" in kinds:
            # the varying limit must matter: the solve of the same list without it, and the reference's boxes without it
            rec.setdefault("novary_sd", []).append(solve(cons(skip=("vary",)), paths[b], grid, 0.0, 0.0)["sd"])
            if any(k in kinds for k in ("vel", "bound")):
                rec.setdefault("novary_high_ref", []).append(reference_boxes(cons(skip=("vary",)), paths[b], grid)[1])
    f.update({k: np.stack(v) for k, v in rec.items()})
    f["kinds"] = np.array(",".join(f["kinds"]))
    f["interpolation"] = np.array(interpolation)
    for k in [k for k in ("vlim", "alim") if {"vlim": "vel", "alim": "acc"}[k] not in kinds]:
        del f[k]
    if "vary" not in kinds:
        del f["vlim0"]
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **f)
    g = sbr.load(name)
    cond = sbr.binding_conditions(g)
    assert cond["ok"] and min(cond.get("vary", [5])) >= 5 and min(cond.get("vary_box", [5])) >= 5 and min(cond.get("xcap", [5])) >= 5 and min(cond.get("ucap", [3])) >= 3, (name, cond)
    assert os.path.getsize(path) < 100 * 1024, os.path.getsize(path)
    print("%-22s %6d bytes  %s  pair status %s  sd status %s" % (name, os.path.getsize(path), cond, g["pair_status"], g["sd_status"]))


def main():
    fixture("boxes_a_d3_N30", ["vary", "acc"], 3, 30, 11)
    # (the varying limit is the tighter of the two velocity limits on 0.35 < s < 0.70: the cap zone of this list lies beside that
    # interval, so that both velocity constraints and both bounds shape the stored profile)
    fixture("boxes_b_d9_N30", ["vel", "vary", "acc", "bound", "ubound"], 9, 30, 12, zone=(0.75, 0.95))
    fixture("boxes_c_d17_N30", ["acc", "bound"], 17, 30, 13, interpolation=False)
    fixture("boxes_d_d7_N40", ["vary", "torque"], 7, 40, 14)


if __name__ == "__main__":
    main()

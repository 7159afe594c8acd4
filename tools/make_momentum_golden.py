#!/usr/bin/env python
"""Generate the momentum fixtures tests/golden/momentum_*.npz by running the REAL reference (hungpham2511/toppra): a host
LinearConstraint that returns (None, None, None, None, None, None, xbound) -- the bound on x = sd^2 made from the numpy momentum
and kinetic energy of tests/momentum_ref.py -- in [JointVelocityConstraint, JointAccelerationConstraint, that] through
TOPPRA(solver_wrapper="seidel"), one trajectory at a time; and profiles/momentum_accuracy.json.

    python tools/make_momentum_golden.py        # needs the reference; builds oracle/_ref on demand

B = 4; data only -- the robot's and the mount's parameters, the link set, waypoints, coefficient tables, grid and limits; the
reference's momentum, energy2 (with their all-absolute magnitudes) and xbound, the reference wrapper's own low / high, sd, u, K
and return codes; and the two tolerances of the GPU test --
  acc_yardstick / acc_bound [2]: the error of the float64 reference against np.longdouble on the fixture's own momentum and
      energy2, in the metric of tests/chain_cases.py, and 16 x that;
  sd_tol: 4 x the largest change of sd over 20 seeds when momentum and energy2 are disturbed by noise of the size of the accuracy
      bound (each uniform in +- its acc_bound x its magnitude), the bound made again from them, and the problem solved by the CPU
      restatement under oracle/.
Two fixtures:
  momentum_d6_N40: a 6-dof chain, every link, a linear-momentum and an energy limit, per trajectory, about the base frame.
  momentum_torso_d15_N30: a torso joint that carries two 7-dof arms; the second arm's links alone, an angular- and a
      linear-momentum limit about a tilted mount frame away from the base.
The limits are chosen here, on the CPU, in physical units: a fraction of each quantity's peak along the reference's own solution
WITHOUT the constraint, lowered until the new bound is the active upper bound on x -- the controllable set's upper end K[i, 1]
equals it, below what the velocity limits leave -- at at least a quarter of the stages of every trajectory.  That, and that the
reference's status is 0 for every trajectory, are asserted.
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
from tests import chain_cases, chain_ref, momentum_cases as mc, momentum_ref as mr, second_order_ref as sor, tree_cases, tree_ref  # noqa: E402
from tests.stage_boxes_ref import bound_only  # noqa: E402

ta = ref_loader.load()
if ta is None:
    raise SystemExit("reference not available")
import toppra.algorithm as algo  # noqa: E402
import toppra.constraint as constraint  # noqa: E402
from toppra.algorithm.algorithm import ParameterizationReturnCode as RC  # noqa: E402

from make_golden_boxes import reference_boxes  # noqa: E402

STATUS = {RC.Ok: 0, RC.FailUncontrollable: 1, RC.ErrUnknown: 2}
ROBOT_KEYS = ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity", "parent")
NAMES = ("momentum", "energy2")
KINDS = ("linear", "angular", "energy")


def chain6():
    chain = {k: v for k, v in chain_ref.random_chain(6, seed=711, gravity=True, prismatic_every=4).items() if k != "tool"}
    chain["parent"] = np.arange(6, dtype=np.int32) - 1
    return chain, dict(mr.NO_MOUNT), None, ("linear", "energy")


def torso_arm():
    tree = tree_ref.random_tree(tree_cases.SHAPES["torso"], seed=77, gravity=True, massless=None)
    tilt = 0.15
    rot = np.array([[np.cos(tilt), 0.0, np.sin(tilt)], [0.0, 1.0, 0.0], [-np.sin(tilt), 0.0, np.cos(tilt)]])
    return tree, {"rot": rot, "origin": np.array([0.1, -0.05, -0.4])}, tuple(range(8, 15)), ("angular", "linear")


def squared(limits, B):
    """[B, 3] = (p_max^2, L_max^2, 2 E_max) of physical limits {kind: [B]}: what the kernel divides; +inf where none is given."""
    lim = np.full((B, 3), np.inf)
    for kind, value in limits.items():
        k = KINDS.index(kind)
        lim[:, k] = 2.0 * value if kind == "energy" else value * value
    return lim


def fixture(name, B, N, seed, make):
    rng = np.random.default_rng(seed)
    robot, mount, links, kinds = make()
    d = len(robot["parent"])
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    way = rng.uniform(-1.5, 1.5, (B, 5, d)) * (0.5 if d > 8 else 1.0)
    vmax, amax = 2.0 + 2.0 * rng.random((B, d)), 6.0 + 4.0 * rng.random((B, d))
    vlim, alim = np.stack([-vmax, vmax], -1), np.stack([-amax, amax], -1)
    paths = [ta.SplineInterpolator(knots, way[b]) for b in range(B)]
    q, qs, qss = (np.stack([p(grid, k) for p in paths]) for k in (0, 1, 2))
    ref = mc.reference_of(robot, mount, q, qs, links)
    h, e2 = ref["momentum"], ref["energy2"]
    acc_dt = constraint.DiscretizationType.Interpolation

    def base_constraints(b):
        return [constraint.JointVelocityConstraint(vlim[b]), constraint.JointAccelerationConstraint(alim[b], discretization_scheme=acc_dt)]

    # the reference without the constraint, and each quantity's peak along its solution, in physical units
    free, peak = [], {k: np.zeros(B) for k in KINDS}
    for b in range(B):
        inst = algo.TOPPRA(base_constraints(b), paths[b], gridpoints=grid, solver_wrapper="seidel")
        _, sd, _, K = inst.compute_parameterization(0, 0, return_data=True)
        assert sd is not None
        free.append(sd)
        peak["linear"][b] = np.max(np.sqrt((h[b, :, :3] ** 2).sum(-1)) * sd)
        peak["angular"][b] = np.max(np.sqrt((h[b, :, 3:] ** 2).sum(-1)) * sd)
        peak["energy"][b] = np.max(0.5 * e2[b] * sd * sd)
    vel_high = sor.velocity_box(qs, vlim)[1][..., 1]

    def solve_reference(limits):
        lim = squared(limits, B)
        xb = mr.xbound(h, e2, lim)
        out = {k: [] for k in ("low", "high", "K", "sd", "u", "status", "active")}
        for b in range(B):
            cons = base_constraints(b) + [bound_only(constraint, None, xb[b])]
            inst = algo.TOPPRA(cons, paths[b], gridpoints=grid, solver_wrapper="seidel")
            sdd, sd, _, K = inst.compute_parameterization(0, 0, return_data=True)
            st = STATUS[inst.problem_data.return_code]
            assert st == 0 and sd is not None, "%s: trajectory %d is not feasible in the reference (status %d)" % (name, b, st)
            low, high = reference_boxes(cons, paths[b], grid)
            out["low"].append(low); out["high"].append(high)
            out["K"].append(K); out["sd"].append(sd); out["u"].append(sdd); out["status"].append(st)
            out["active"].append(int(np.sum((K[:, 1] == xb[b, :, 1]) & (xb[b, :, 1] < vel_high[b]))))
        return lim, xb, out

    fraction = 0.9
    while True:
        limits = {kind: fraction * peak[kind] * (1.0 + 0.1 * np.arange(B) / B) for kind in kinds}  # (per trajectory: no two alike)
        lim, xb, out = solve_reference(limits)
        print("%s: fraction %.3f of the peak -> the bound is active at %s of %d stages" % (name, fraction, out["active"], N + 1))
        if min(out["active"]) >= (N + 1 + 3) // 4:
            break
        fraction *= 0.85
        assert fraction > 0.05, "%s: the bound never becomes active at a quarter of the stages" % name
    assert all(4 * a >= N + 1 for a in out["active"])
    for b in range(B):
        assert not np.array_equal(out["sd"][b], free[b])
        print("%s trajectory %d: largest sd %.4f, without the constraint %.4f" % (name, b, out["sd"][b].max(), free[b].max()))
    rec = {k: np.stack(v) for k, v in out.items() if k != "active"}
    rec["status"] = rec["status"].astype(np.int32)
    rec["active"] = np.array(out["active"], dtype=np.int32)
    coef = np.stack([np.asarray(p.cspl.c) for p in paths])
    breaks = np.asarray(paths[0].cspl.x)

    # the accuracy yardstick on the fixture's own inputs
    yard = np.array([ref["yardstick"][k] for k in NAMES])
    bound = chain_cases.BOUND_FACTOR * yard
    assert np.all(yard > 0)

    # the end-to-end tolerance of sd: the CPU restatement on the box made from disturbed momentum and energy2
    rows = sor.dense_problem(coef, breaks, grid, vlim, alim, True, [])

    def solve(hv, ev):
        cap = mr.xbound(hv, ev, lim)[..., 1]
        high = rows["high"].copy()
        high[..., 1] = np.where(high[..., 1] < cap, high[..., 1], cap)  # (dbl_min with the running value first, as the fold spells it)
        return high, orc.solve_dense_batch(rows["a"], rows["b"], rows["c"], rows["low"], high, rows["deltas"])
    high0, base = solve(h, e2)
    assert np.array_equal(high0, rec["high"]) and np.array_equal(rows["low"], rec["low"]), "the restated boxes differ from the reference's"
    assert np.array_equal(base["status"], rec["status"]) and np.array_equal(base["sd"], rec["sd"]), "the restatement differs from the reference"
    worst = 0.0
    for s in range(20):
        nrng = np.random.default_rng(1000 + s)
        noisy = [v + bd * ref[k + "_mag"] * nrng.uniform(-1.0, 1.0, v.shape) for bd, k, v in zip(bound, NAMES, (h, e2))]
        _, got = solve(*noisy)
        assert np.array_equal(got["status"], rec["status"])
        worst = max(worst, float(np.max(np.abs(got["sd"] - base["sd"]))))
    assert worst > 0
    rec.update({k: np.asarray(robot[k]) for k in ROBOT_KEYS})
    rec.update({"mount_" + k: np.asarray(mount[k], dtype=np.float64) for k in ("rot", "origin")})
    rec.update({"limit_" + kind: limits[kind] for kind in kinds})
    rec.update(links=np.array(mr.link_set(robot, links), dtype=np.int32), knots=knots, way=way, coef=coef, breaks=breaks, grid=grid,
               vlim=vlim, alim=alim, limit=lim, momentum=h, energy2=e2, momentum_mag=ref["momentum_mag"], energy2_mag=ref["energy2_mag"],
               xbound=xb, acc_yardstick=yard, acc_bound=bound, sd_tol=np.array(4.0 * worst))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 200 * 1024, os.path.getsize(path)
    print(name, "active", rec["active"], "status", np.bincount(rec["status"], minlength=3), "acc_bound", bound,
          "sd_tol %.3g" % (4.0 * worst), "%.0f KB" % (os.path.getsize(path) / 1024))
    return {"yardstick": dict(zip(NAMES, yard.tolist())), "bound": dict(zip(NAMES, bound.tolist())), "sd_tol": 4.0 * worst,
            "fraction_of_peak": fraction}


if __name__ == "__main__":
    fixtures = {"momentum_d6_N40": fixture("momentum_d6_N40", 4, 40, 811, chain6),
                "momentum_torso_d15_N30": fixture("momentum_torso_d15_N30", 4, 30, 812, torso_arm)}
    path = os.path.join(ROOT, "profiles", "momentum_accuracy.json")
    measured = {}
    if os.path.exists(path):  # (what the kernel was measured to use is written by the GPU run, not here: keep it)
        with open(path) as fh:
            measured = json.load(fh).get("measured", {})
    with open(path, "w") as fh:
        json.dump({"metric": "|got - ref| / (|ref| with every product and sum in absolute value); yardstick = float64 "
                             "tests/momentum_ref.py against np.longdouble on the same inputs; bound = %g x yardstick"
                             % chain_cases.BOUND_FACTOR,
                   "cases": mc.accuracy_table(), "fixtures": fixtures, "measured": measured}, fh, indent=1, sort_keys=True)
        fh.write("\n")

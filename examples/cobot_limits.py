"""Retime paths of a 7-dof collaborative arm that carries a workpiece, under the limits its safety controller is configured with:
a cap on the arm's momentum (kg m / s), a cap on the kinetic energy it could transfer on contact (J), and a speed limit on the
elbow and the tool point (m / s).  A heavy forearm moving slowly passes every point-speed limit and still trips the momentum
limit, so the three are different constraints; the example prints where each of them is the one that binds.

The momentum and the energy are those of the whole moving structure, workpiece included (``with_payload``), from one launch per
batch; the limits are given in physical units (the point-speed constraint takes the SQUARE of a speed).

    python examples/cobot_limits.py [--batch 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toppra_amd as ta  # noqa: E402
from toppra_amd.constraint import BatchPointSpeedConstraint  # noqa: E402


def arm():
    """The arm of examples/control_points.py with masses that grow towards the base (12 kg of links, a heavy forearm), thin-rod
    inertias, and a 3 kg workpiece at the tool."""
    axes = np.array([[0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1]], dtype=float)
    offsets = np.array([[0, 0, 0.35], [0, 0, 0], [0, 0, 0], [0.045, 0, 0.55], [-0.045, 0, 0.3], [0, 0, 0], [0, 0, 0.06]])
    masses = np.array([3.0, 2.5, 2.0, 2.5, 1.0, 0.6, 0.4])
    coms = np.array([[0, 0, -0.1], [0, 0, 0.2], [0, 0, 0.4], [0, 0, 0.15], [0, 0, 0.2], [0, 0, 0.02], [0, 0, 0.03]])
    inertias = np.stack([np.array([0.02, 0.02, 0.004, 0, 0, 0]) * m for m in masses])
    chain = ta.SerialChain(["revolute"] * 7, axes, np.stack([np.eye(3)] * 7), offsets, masses, coms, inertias, tool=(0, 0, 0.12))
    return chain.with_payload(ta.Payload(3.0, com=(0.0, 0.0, 0.16), inertia=[0.01, 0.01, 0.006, 0, 0, 0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    B = ap.parse_args().batch
    np.random.seed(9)
    chain, d, N = arm(), 7, 100
    points = ta.ControlPoints([3, -1], [[0.0, 0.0, 0.0], chain.tool])  # the elbow, the tool point
    waypoints = np.random.randn(B, 5, d) * 0.6
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    vlim = np.tile([-2.0, 2.0], (B, d, 1))
    alim = np.tile([-8.0, 8.0], (B, d, 1))
    p_max, e_max, v_max = 8.0, 4.0, np.array([0.7, 1.25])  # kg m / s, J, m / s (elbow, tool)

    momentum = ta.BatchMomentumConstraint(chain, linear=p_max)
    energy = ta.BatchMomentumConstraint(chain, energy=e_max)
    speed = BatchPointSpeedConstraint(chain, points, v_max ** 2)
    named = (("momentum", momentum), ("energy", energy), ("point speed", speed))
    make = lambda cons: ta.algorithm.BatchTOPPRA.from_waypoints(knots, waypoints, grid, vlim, alim, **({"constraints": cons} if cons else {}))  # noqa: E731
    bt, free = make([c for _, c in named]), make([])
    out, ref = bt.compute_parameterization(), free.compute_parameterization()
    ok = out["status"] == 0

    # which limit binds where: the stage box of all three against the box of each one alone
    high = bt.stage_boxes()[1][..., 1]
    joint = free.stage_boxes()[1][..., 1]
    alone = {name: make([c]).stage_boxes()[1][..., 1] for name, c in named}
    tight = high < joint
    print("%d paths of %d gridpoints: %d Ok; a safety limit is tighter than the joint velocity limits at %.0f %% of the gridpoints"
          % (B, N + 1, int(ok.sum()), 100.0 * tight.mean()))
    for name, box in alone.items():
        binds = tight & (box == high)
        active = binds & (np.abs(out["sd"] ** 2 - high) <= 2e-6 * high)  # (the solver keeps the reference's small margins below a bound)
        print("%-11s binds the box at %5.1f %% of the gridpoints, and holds the solution there at %5.1f %%"
              % (name, 100.0 * binds.mean(), 100.0 * active[ok].mean()))

    # the limits hold along the solution: qd = q' sd
    pe = ta.batch.path_eval_batch(bt.coef, bt.breaks, grid)
    for res, label in ((out, "with the limits"), (ref, "joint limits alone")):
        qd = pe["qs"] * res["sd"][..., None]
        p = np.sqrt((chain.momentum(pe["q"], qd)[..., :3] ** 2).sum(-1))
        e = chain.kinetic_energy(pe["q"], qd)
        v = np.sqrt(chain.point_speeds(pe["q"], qd, points))
        print("%-19s largest momentum %.3f kg m/s (limit %.1f), energy %.3f J (%.1f), elbow %.3f m/s (%.2f), tool %.3f m/s (%.2f)"
              % (label, np.nanmax(p[ok]), p_max, np.nanmax(e[ok]), e_max, np.nanmax(v[ok][..., 0]), v_max[0], np.nanmax(v[ok][..., 1]), v_max[1]))
        if res is out:
            assert np.nanmax(p[ok]) <= p_max * (1 + 1e-9) and np.nanmax(e[ok]) <= e_max * (1 + 1e-9)
            assert np.all(np.nanmax(v[ok], axis=(0, 1)) <= v_max * (1 + 1e-9))
    dur, dur0 = bt.compute_trajectory().duration, free.compute_trajectory().duration
    print("mean duration %.3f s, %.3f s with joint velocity and acceleration limits alone" % (np.nanmean(dur[ok]), np.nanmean(dur0[ok])))
    assert ok.all() and np.nanmean(dur[ok]) > np.nanmean(dur0[ok])
    assert all((tight & (box == high)).any() for box in alone.values()), "one of the three limits never binds: not much of an example"


if __name__ == "__main__":
    main()

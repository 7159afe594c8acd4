"""Retime paths of a 7-dof arm under a limit on the Cartesian acceleration of its tool point: the problem of the reference's
examples-old/cartesian_accel.py -- a SecondOrderConstraint whose inv_dyn returns a link's acceleration, F = [I; -I], g = 0.5 --
with the arm given by its parameters.  The SerialChain is evaluated on the GPU at every gridpoint of every trajectory, so no
kinematics has to be written for the batch.

    python examples/cartesian_accel.py [--batch 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toppra_amd as ta  # noqa: E402
from toppra_amd.constraint import BatchCartesianAccelerationConstraint  # noqa: E402


def arm():
    """A 7-dof arm in the layout of a cable-driven manipulator: revolute joints about z, y, z, y, z, y, z of the frames they sit
    in, upper arm 0.55 m, forearm 0.3 m with a 45 mm elbow offset, the tool point 0.12 m past the last joint.  The acceleration
    limit reads no masses: they are placeholders."""
    axes = np.array([[0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1]], dtype=float)
    offsets = np.array([[0, 0, 0.35], [0, 0, 0], [0, 0, 0], [0.045, 0, 0.55], [-0.045, 0, 0.3], [0, 0, 0], [0, 0, 0.06]])
    rotations = np.stack([np.eye(3)] * 7)
    return ta.SerialChain(["revolute"] * 7, axes, rotations, offsets, np.ones(7), np.zeros((7, 3)), np.tile([0.01, 0.01, 0.01, 0, 0, 0], (7, 1)),
                          tool=(0, 0, 0.12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    B = ap.parse_args().batch
    np.random.seed(9)  # (the reference example's seed and waypoints for the first path)
    chain, d, N = arm(), 7, 100
    waypoints = np.random.randn(B, 5, d) * 0.6
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    vlim = np.tile([-2.0, 2.0], (B, d, 1))
    alim = np.tile([-8.0, 8.0], (B, d, 1))
    a_max = 0.5  # m/s^2 on each world axis: -0.5 <= a <= 0.5

    cons = [BatchCartesianAccelerationConstraint(chain, linear=a_max)]
    bt = ta.algorithm.BatchTOPPRA.from_waypoints(knots, waypoints, grid, vlim, alim, constraints=cons)
    free = ta.algorithm.BatchTOPPRA.from_waypoints(knots, waypoints, grid, vlim, alim)
    out, ref = bt.compute_parameterization(), free.compute_parameterization()
    ok = out["status"] == 0
    pe = ta.batch.path_eval_batch(bt.coef, bt.breaks, grid)

    def tool_acceleration(res):
        """Along a parameterization, at the gridpoints it was solved on: qd = q' sd, qdd = q'' sd^2 + q' u."""
        sd, u = res["sd"][:, :-1, None], res["u"][..., None]
        q, qs, qss = (pe[k][:, :-1] for k in ("q", "qs", "qss"))
        return chain.tool_acceleration(q, qs * sd, qss * sd ** 2 + qs * u)[..., :3]
    acc, acc0 = np.abs(tool_acceleration(out)), np.abs(tool_acceleration(ref))
    print("%d paths: %d Ok" % (B, int(ok.sum())))
    print("largest |tool acceleration| per world axis: %s m/s^2 (limit %.2f); with joint limits alone: %s"
          % (np.round(np.nanmax(acc[ok], axis=(0, 1)), 4), a_max, np.round(np.nanmax(acc0[ok], axis=(0, 1)), 2)))
    dur, dur0 = bt.compute_trajectory().duration, free.compute_trajectory().duration
    print("mean duration %.3f s, %.3f s with joint velocity and acceleration limits alone" % (np.nanmean(dur[ok]), np.nanmean(dur0[ok])))
    assert ok.any() and np.nanmax(acc[ok]) <= a_max * (1 + 1e-9)
    assert (ref["sd"][ok] >= out["sd"][ok] - 1e-9).all()


if __name__ == "__main__":
    main()

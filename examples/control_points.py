"""Retime paths of a 7-dof arm under whole-arm limits: the elbow, a camera bracket on the forearm and the tool point are each held
to a speed and to a Cartesian acceleration on every world axis.  The points are fixed to different links of the arm; the
SerialChain evaluates all of them in one pass over its links at every gridpoint of every trajectory, so neither truncated models
nor per-point callbacks have to be written for the batch.

    python examples/control_points.py [--batch 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toppra_amd as ta  # noqa: E402
from toppra_amd.constraint import BatchPointAccelerationConstraint, BatchPointSpeedConstraint  # noqa: E402


def arm():
    """The arm of examples/cartesian_accel.py: revolute joints about z, y, z, y, z, y, z of the frames they sit in, upper arm
    0.55 m, forearm 0.3 m with a 45 mm elbow offset, the tool point 0.12 m past the last joint.  The limits read no masses:
    they are placeholders."""
    axes = np.array([[0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1]], dtype=float)
    offsets = np.array([[0, 0, 0.35], [0, 0, 0], [0, 0, 0], [0.045, 0, 0.55], [-0.045, 0, 0.3], [0, 0, 0], [0, 0, 0.06]])
    rotations = np.stack([np.eye(3)] * 7)
    return ta.SerialChain(["revolute"] * 7, axes, rotations, offsets, np.ones(7), np.zeros((7, 3)), np.tile([0.01, 0.01, 0.01, 0, 0, 0], (7, 1)),
                          tool=(0, 0, 0.12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    B = ap.parse_args().batch
    np.random.seed(9)
    chain, d, N = arm(), 7, 100
    # the elbow (the origin of link 3), a camera bracket 8 cm off the forearm (link 4), the tool point (the last link)
    points = ta.ControlPoints([3, 4, -1], [[0.0, 0.0, 0.0], [0.08, 0.0, 0.15], chain.tool])
    names = ("elbow", "camera", "tool")
    waypoints = np.random.randn(B, 5, d) * 0.6
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    vlim = np.tile([-2.0, 2.0], (B, d, 1))
    alim = np.tile([-8.0, 8.0], (B, d, 1))
    v_max = np.array([0.4, 0.5, 0.8])  # m/s per point; the constraint takes the SQUARE of a speed
    a_max = np.array([0.6, 0.8, 1.0])  # m/s^2 on each world axis, per point

    cons = [BatchPointSpeedConstraint(chain, points, v_max ** 2), BatchPointAccelerationConstraint(chain, points, linear=a_max)]
    bt = ta.algorithm.BatchTOPPRA.from_waypoints(knots, waypoints, grid, vlim, alim, constraints=cons)
    free = ta.algorithm.BatchTOPPRA.from_waypoints(knots, waypoints, grid, vlim, alim)
    out, ref = bt.compute_parameterization(), free.compute_parameterization()
    ok = out["status"] == 0
    pe = ta.batch.path_eval_batch(bt.coef, bt.breaks, grid)

    def along(res):
        """Speeds [B, N, P] and accelerations [B, N, P, 3] along a parameterization, at the gridpoints it was solved on:
        qd = q' sd, qdd = q'' sd^2 + q' u."""
        sd, u = res["sd"][:, :-1, None], res["u"][..., None]
        q, qs, qss = (pe[k][:, :-1] for k in ("q", "qs", "qss"))
        return np.sqrt(chain.point_speeds(q, qs * sd, points)), np.abs(chain.point_accelerations(q, qs * sd, qss * sd ** 2 + qs * u, points))
    (speed, acc), (speed0, acc0) = along(out), along(ref)
    print("%d paths: %d Ok" % (B, int(ok.sum())))
    for p, name in enumerate(names):
        print("%-6s largest speed %.4f m/s (limit %.2f; %.2f with joint limits alone), largest |acceleration| on an axis %.4f m/s^2 "
              "(limit %.2f; %.2f)" % (name, np.nanmax(speed[ok][..., p]), v_max[p], np.nanmax(speed0[ok][..., p]),
                                      np.nanmax(acc[ok][..., p, :]), a_max[p], np.nanmax(acc0[ok][..., p, :])))
    dur, dur0 = bt.compute_trajectory().duration, free.compute_trajectory().duration
    print("mean duration %.3f s, %.3f s with joint velocity and acceleration limits alone" % (np.nanmean(dur[ok]), np.nanmean(dur0[ok])))
    assert ok.any()
    assert np.all(np.nanmax(speed[ok], axis=(0, 1)) <= v_max * (1 + 1e-9))
    assert np.all(np.nanmax(acc[ok], axis=(0, 1, 3)) <= a_max * (1 + 1e-9))
    assert (ref["sd"][ok] >= out["sd"][ok] - 1e-9).all()


if __name__ == "__main__":
    main()

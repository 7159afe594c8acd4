"""Retime a batch of paths of one 6-dof arm under joint torque limits and a tool-speed limit, the arm given by its parameters:
a SerialChain is evaluated on the GPU at every gridpoint of every trajectory -- recursive Newton-Euler for the torque rows, the
forward recursion for the tool's velocity -- so no inverse dynamics has to be written for the batch.

    python examples/torque_chain.py [--batch 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toppra_amd as ta  # noqa: E402
from toppra_amd.constraint import BatchCartesianVelocityNormConstraint, BatchJointTorqueConstraint  # noqa: E402


def arm():
    """An elbow arm with a spherical wrist: revolute joints about z, y, y, x, y, x of the frames they sit in; lengths in m,
    masses in kg, each link a slender rod along the direction to the next joint."""
    axes = np.array([[0, 0, 1], [0, 1, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0]], dtype=float)
    offsets = np.array([[0, 0, 0.0], [0, 0, 0.35], [0.4, 0, 0], [0.35, 0, 0], [0.1, 0, 0], [0.08, 0, 0]])
    rotations = np.stack([np.eye(3)] * 6)
    masses = np.array([6.0, 5.0, 3.0, 1.5, 1.0, 0.5])
    coms = np.array([[0, 0, 0.2], [0.2, 0, 0], [0.17, 0, 0], [0.05, 0, 0], [0.04, 0, 0], [0.03, 0, 0]])
    length = np.array([0.35, 0.4, 0.35, 0.1, 0.08, 0.06])
    rod = masses * length ** 2 / 12
    inertias = np.stack([np.array([rod[0], rod[0], 0.01, 0, 0, 0])] + [np.array([0.002, rod[i], rod[i], 0, 0, 0]) for i in range(1, 6)])
    return ta.SerialChain(["revolute"] * 6, axes, rotations, offsets, masses, coms, inertias, gravity=(0, 0, -9.81), tool=(0.1, 0, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    B = ap.parse_args().batch
    rng = np.random.default_rng(0)
    chain, d, N = arm(), 6, 100
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    waypoints = rng.uniform(-1.2, 1.2, (B, 5, d))
    vlim = np.tile([-3.0, 3.0], (B, d, 1))
    alim = np.tile([-15.0, 15.0], (B, d, 1))
    tau_max = np.array([120.0, 120.0, 60.0, 20.0, 10.0, 5.0])
    tau_lim = np.stack([-tau_max, tau_max], -1)
    v_tool = 1.0  # m/s: the constraint bounds |v|^2 sd^2, so its limit is the square

    cons = [BatchJointTorqueConstraint(chain, tau_lim, fs_coef=np.full(d, 0.2)), BatchCartesianVelocityNormConstraint(chain, v_tool ** 2)]
    bt = ta.algorithm.BatchTOPPRA.from_waypoints(knots, waypoints, grid, vlim, alim, constraints=cons)
    free = ta.algorithm.BatchTOPPRA.from_waypoints(knots, waypoints, grid, vlim, alim)
    out, ref = bt.compute_parameterization(), free.compute_parameterization()
    ok = out["status"] == 0
    pe = ta.batch.path_eval_batch(bt.coef, bt.breaks, grid)
    sd = out["sd"]
    u = np.concatenate([out["u"], out["u"][:, -1:]], 1)
    # the torques and the tool speed along the retimed trajectories: qd = q' sd, qdd = q'' sd^2 + q' u
    qd, qdd = pe["qs"] * sd[..., None], pe["qss"] * (sd ** 2)[..., None] + pe["qs"] * u[..., None]
    tau = chain.inverse_dynamics(pe["q"], qd, qdd)
    speed = np.sqrt(chain.tool_velocity_norm(pe["q"], pe["qs"])) * sd
    print("%d paths: %d Ok" % (B, int(ok.sum())))
    print("largest |torque| / limit per joint:", np.round(np.nanmax(np.abs(tau[ok][:, :-1]) / tau_max, axis=(0, 1)), 3))
    print("largest tool speed %.3f m/s (limit %.1f)" % (np.nanmax(speed[ok]), v_tool))
    dur, dur0 = bt.compute_trajectory().duration, free.compute_trajectory().duration
    print("mean duration %.3f s, %.3f s with joint velocity and acceleration limits alone" % (np.nanmean(dur[ok]), np.nanmean(dur0[ok])))
    assert ok.any() and np.nanmax(speed[ok]) <= v_tool * (1 + 1e-9)
    assert (ref["sd"][ok] >= sd[ok] - 1e-9).all()


if __name__ == "__main__":
    main()

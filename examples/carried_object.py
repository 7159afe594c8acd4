"""Retime pick-and-place paths of a SCARA-like arm that carries a box on a tray, so that the box neither slides, tips nor twists:
the contact wrench cone of the box's footprint as a limit on the wrench the last link transmits to it
(``BatchToolWrenchConstraint.surface_contact``), beside joint-torque limits on the arm with the box merged into its last link
(``SerialChain.with_payload``).  The arm's revolute axes and its prismatic joint are vertical, so the tray stays level.

    python examples/carried_object.py [--batch 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toppra_amd as ta  # noqa: E402
from toppra_amd.constraint import BatchJointTorqueConstraint, BatchToolWrenchConstraint  # noqa: E402


def arm():
    """Shoulder and elbow about z (0.35 m and 0.3 m), a vertical lift, a wrist about z; the tray's centre is the tool point."""
    d = 4
    return ta.SerialChain(["revolute", "revolute", "prismatic", "revolute"], np.tile([0.0, 0.0, 1.0], (d, 1)), np.stack([np.eye(3)] * d),
                          [[0.0, 0.0, 0.4], [0.35, 0.0, 0.0], [0.3, 0.0, 0.0], [0.0, 0.0, -0.1]], [6.0, 4.0, 1.5, 0.5],
                          [[0.17, 0.0, 0.0], [0.15, 0.0, 0.0], [0.0, 0.0, -0.1], [0.0, 0.0, 0.0]],
                          [[0.02, 0.08, 0.08, 0, 0, 0], [0.01, 0.04, 0.04, 0, 0, 0], [0.005, 0.005, 0.001, 0, 0, 0], [0.0005, 0.0005, 0.0005, 0, 0, 0]],
                          gravity=(0.0, 0.0, -9.81), tool=(0.05, 0.0, 0.02))


def box(chain):
    """A 0.8 kg box of 10 x 6 x 8 cm standing on the tray: the contact frame is the tray's (default: the tool point, link axes)."""
    m, sx, sy, sz = 0.8, 0.10, 0.06, 0.08
    inertia = [m * (sy ** 2 + sz ** 2) / 12, m * (sx ** 2 + sz ** 2) / 12, m * (sx ** 2 + sy ** 2) / 12, 0.0, 0.0, 0.0]
    return ta.Payload(m, com=chain.tool + np.array([0.0, 0.0, sz / 2]), inertia=inertia), (sx / 2, sy / 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    B = ap.parse_args().batch
    rng = np.random.default_rng(3)
    chain, d, N, mu = arm(), 4, 100, 0.3
    obj, half_extents = box(chain)
    waypoints = rng.uniform(-1.5, 1.5, (B, 5, d))
    waypoints[..., 2] *= 0.1  # the lift: +- 15 cm
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    vlim, alim = np.tile([-3.0, 3.0], (B, d, 1)), np.tile([-10.0, 10.0], (B, d, 1))
    taulim = np.array([[-40.0, 40.0], [-20.0, 20.0], [-60.0, 60.0], [-5.0, 5.0]])  # (the lift holds 2.8 kg against gravity: 27 N)

    torque = BatchJointTorqueConstraint(chain.with_payload(obj), taulim, np.zeros(d))
    contact = BatchToolWrenchConstraint.surface_contact(chain, obj, mu, half_extents)
    bt = ta.algorithm.BatchTOPPRA.from_waypoints(knots, waypoints, grid, vlim, alim, constraints=[torque, contact])
    free = ta.algorithm.BatchTOPPRA.from_waypoints(knots, waypoints, grid, vlim, alim, constraints=[torque])
    out, ref = bt.compute_parameterization(), free.compute_parameterization()
    ok = (out["status"] == 0) & (ref["status"] == 0)
    pe = ta.batch.path_eval_batch(bt.coef, bt.breaks, grid)

    def friction_margin(res):
        """Along a parameterization, at the gridpoints it was solved on (qd = q' sd, qdd = q'' sd^2 + q' u): the smallest of
        mu fz - |fx|, mu fz - |fy|, in newtons -- negative where the box would slide."""
        sd, u = res["sd"][:, :-1, None], res["u"][..., None]
        q, qs, qss = (pe[k][:, :-1] for k in ("q", "qs", "qss"))
        w = chain.tool_wrench(q, qs * sd, qss * sd ** 2 + qs * u, obj)
        return (mu * w[..., 2:3] - np.abs(w[..., :2])).min(-1), (contact.F @ w[..., None])[..., 0].max(-1)
    margin, worst_row = friction_margin(out)
    margin0, _ = friction_margin(ref)
    dur, dur0 = bt.compute_trajectory().duration, free.compute_trajectory().duration
    print("%d paths: %d Ok" % (B, int(ok.sum())))
    print("mean duration %.3f s with the contact constraint, %.3f s with joint and torque limits alone" % (np.nanmean(dur[ok]), np.nanmean(dur0[ok])))
    print("smallest friction margin along the result: %.4f N (without the constraint: %.2f N -- the box slides)"
          % (np.nanmin(margin[ok]), np.nanmin(margin0[ok])))
    assert ok.any() and np.nanmax(worst_row[ok]) <= 1e-8 and np.nanmin(margin[ok]) >= -1e-8
    assert np.nanmean(dur[ok]) >= np.nanmean(dur0[ok])


if __name__ == "__main__":
    main()

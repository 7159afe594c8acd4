"""Retime a batch of paths of a light 6-dof arm that carries a heavy tool, so that not only the joint torques stay within their
ratings but also what the gearboxes' output bearings carry ACROSS their axes: the tilting moment and the axial and radial force at
the shoulder (joint 1) and at the wrist (joint 4).  Data sheets give these limits next to the rated torque, and an arm with a
heavy tool oversteps them first.  The wrenches across the two joints are evaluated on the GPU at every gridpoint of every
trajectory (KinematicTree / SerialChain.joint_wrenches) and held inside the bearings' limits
(BatchJointLoadConstraint.bearing), beside the torque limits of the loaded arm.

    python examples/bearing_loads.py [--batch 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toppra_amd as ta  # noqa: E402
from toppra_amd.constraint import BatchJointLoadConstraint, BatchJointTorqueConstraint  # noqa: E402
from torque_chain import arm  # noqa: E402  (the elbow arm with a spherical wrist of examples/torque_chain.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    B = ap.parse_args().batch
    rng = np.random.default_rng(0)
    d, N, sides = 6, 100, 8
    # a 4 kg spindle, its centre of mass 12 cm in front of the flange
    tool = ta.Payload(4.0, com=(0.12, 0.0, 0.0), inertia=[0.004, 0.02, 0.02, 0.0, 0.0, 0.0])
    chain = arm().with_payload(tool)
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    waypoints = rng.uniform(-1.0, 1.0, (B, 5, d))
    vlim = np.tile([-3.0, 3.0], (B, d, 1))
    alim = np.tile([-15.0, 15.0], (B, d, 1))
    tau_max = np.array([150.0, 150.0, 80.0, 30.0, 20.0, 10.0])
    # the bearings: z along the joint axes, their centres 3 cm (shoulder) and 1 cm (wrist) along them
    sections = ta.JointSections.on_axes(chain, [1, 4], [0.03, 0.01])

    coef, breaks = ta.batch.spline_fit_batch(knots, waypoints, "not-a-knot")
    pe = ta.batch.path_eval_batch(coef, breaks, grid)
    zero = np.zeros_like(pe["q"])
    w0 = chain.joint_wrenches(pe["q"], zero, zero, sections)  # [B, N+1, 2, 6]: what the bearings carry at rest
    tilt = lambda w: np.hypot(w[..., 3], w[..., 4])  # noqa: E731
    radial = lambda w: np.hypot(w[..., 0], w[..., 1])  # noqa: E731
    # data-sheet limits: the largest static load of these paths plus a small dynamic allowance (a real sheet is fixed; here it follows
    # the paths so that standing still satisfies the rows at every gridpoint, without which no retiming can help).  The shoulder's
    # axis stays horizontal, so its axial load is purely dynamic: the allowance is all of its limit.
    room = 1.0 / np.cos(np.pi / sides)
    limits = dict(tilting=room * (tilt(w0).max((0, 1)) + 3.0), radial=room * (radial(w0).max((0, 1)) + 15.0),
                  axial=np.abs(w0[..., 2]).max((0, 1)) + 25.0)
    torque = BatchJointTorqueConstraint(chain, np.stack([-tau_max, tau_max], -1), np.zeros(d))
    bearing = BatchJointLoadConstraint.bearing(chain, sections, sides=sides, **limits)
    assert (np.einsum("mk,bnk->bnm", bearing.F, w0.reshape(B, N + 1, 12)) - bearing.g).max() < 0
    bt = ta.algorithm.BatchTOPPRA(coef, breaks, grid, vlim, alim, constraints=[torque, bearing])
    free = ta.algorithm.BatchTOPPRA(coef, breaks, grid, vlim, alim, constraints=[torque])
    out, ref = bt.compute_parameterization(), free.compute_parameterization()
    ok = (out["status"] == 0) & (ref["status"] == 0)

    def loads(res):
        """The bearings' wrenches along a retimed batch, at the gridpoints it was solved on: qd = q' sd, qdd = q'' sd^2 + q' u."""
        sd, u = res["sd"][:, :-1, None], res["u"][..., None]
        q, qs, qss = (pe[k][:, :-1] for k in ("q", "qs", "qss"))
        return chain.joint_wrenches(q, qs * sd, qss * sd ** 2 + qs * u, sections)

    w, w_free = loads(out), loads(ref)
    print("%s with a %.0f kg tool: %d paths, %d Ok" % (chain, tool.mass, B, int(ok.sum())))
    for k, name in enumerate(("shoulder", "wrist")):
        print("%-8s tilting limit %6.1f N m: largest along the retimed paths %6.1f, with torque limits alone %6.1f"
              % (name, limits["tilting"][k], tilt(w[ok])[..., k].max(), tilt(w_free[ok])[..., k].max()))
        print("%-8s radial  limit %6.1f N:   largest along the retimed paths %6.1f, with torque limits alone %6.1f"
              % (name, limits["radial"][k], radial(w[ok])[..., k].max(), radial(w_free[ok])[..., k].max()))
    worst = (np.einsum("mk,bnk->bnm", bearing.F, w[ok].reshape(int(ok.sum()), N, 12)) - bearing.g).max()
    print("largest F w - g along the retimed paths: %.3g (the limits hold where it is <= 0)" % worst)
    dur, dur0 = bt.compute_trajectory().duration, free.compute_trajectory().duration
    print("mean duration %.3f s, %.3f s with torque limits alone" % (np.nanmean(dur[ok]), np.nanmean(dur0[ok])))
    scale = np.einsum("mk,bnk->bnm", np.abs(bearing.F), np.abs(w[ok].reshape(int(ok.sum()), N, 12))).max()
    assert ok.any() and worst <= 1e-9 * scale, worst
    # the polygon is inscribed: what the rows allow never exceeds the data sheet
    assert np.all(tilt(w[ok]).max((0, 1)) <= limits["tilting"] * (1 + 1e-9)) and np.all(radial(w[ok]).max((0, 1)) <= limits["radial"] * (1 + 1e-9))
    assert np.nanmean(dur[ok]) >= np.nanmean(dur0[ok])


if __name__ == "__main__":
    main()

"""Retime a batch of paths of a two-armed robot that stands on a cart -- a torso joint carrying two 7-dof arms, planned as one
15-dof path -- so that the cart neither tips over an edge of its footprint, nor slides, nor spins on the floor.  What the floor
must supply is the base reaction: the wrench on the robot's mount, summed over BOTH arms and the torso, plus the cart's own
weight.  It is evaluated on the GPU at every gridpoint of every trajectory and held inside the contact wrench cone of the
footprint (BatchBaseWrenchConstraint.surface_contact).

    python examples/mobile_base.py [--batch 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toppra_amd as ta  # noqa: E402
from dual_arm import robot  # noqa: E402  (the torso with two arms of examples/dual_arm.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    B = ap.parse_args().batch
    rng = np.random.default_rng(0)
    d, N = 15, 100
    tree = robot()
    # the cart: 25 kg, its centre of mass 0.35 m under the robot's base; the floor is 0.5 m under the base, the footprint
    # 0.5 m x 0.4 m around the point under the torso axis; rubber wheels on concrete
    mount = ta.Mount(origin=(0.0, 0.0, -0.5), mass=25.0, com=(0.0, 0.0, -0.35))
    mu, half_extents = 0.6, (0.25, 0.20)
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    waypoints = rng.uniform(-1.0, 1.0, (B, 5, d))
    vlim = np.tile([-3.0, 3.0], (B, d, 1))
    alim = np.tile([-15.0, 15.0], (B, d, 1))

    coef, breaks = ta.batch.spline_fit_batch(knots, waypoints, "not-a-knot")
    pe = ta.batch.path_eval_batch(coef, breaks, grid)
    con = ta.BatchBaseWrenchConstraint.surface_contact(tree, mu, half_extents, mount=mount)
    # standing still must lie inside the cone at every gridpoint, or no retiming can help: F w(q, 0, 0) <= g
    w0 = tree.base_wrench(pe["q"], np.zeros_like(pe["q"]), np.zeros_like(pe["q"]), mount)
    still = np.einsum("mk,bnk->bnm", con.F, w0) - con.g
    assert still.max() < 0, "a pose of these paths tips the cart at rest: a wider footprint or a heavier cart is needed"
    bt = ta.algorithm.BatchTOPPRA(coef, breaks, grid, vlim, alim, constraints=[con])
    free = ta.algorithm.BatchTOPPRA(coef, breaks, grid, vlim, alim)
    out, ref = bt.compute_parameterization(), free.compute_parameterization()
    ok = out["status"] == 0

    def reaction(res):
        """The base reaction along a retimed batch: qd = q' sd, qdd = q'' sd^2 + q' u."""
        sd, u = res["sd"], np.concatenate([res["u"], res["u"][:, -1:]], 1)
        qd, qdd = pe["qs"] * sd[..., None], pe["qss"] * (sd ** 2)[..., None] + pe["qs"] * u[..., None]
        return tree.base_wrench(pe["q"], qd, qdd, mount)

    w, w_free = reaction(out), reaction(ref)
    # where the floor's force acts: the centre of pressure (-ty / fz, tx / fz) must stay inside the footprint
    cop = np.stack([-w[..., 4] / w[..., 2], w[..., 3] / w[..., 2]], -1)[:, :-1]
    cop_free = np.stack([-w_free[..., 4] / w_free[..., 2], w_free[..., 3] / w_free[..., 2]], -1)[:, :-1]
    print("%s on a %.0f kg cart, footprint %.2f m x %.2f m, mu %.1f\n%d paths: %d Ok" % (tree, mount.mass, 2 * half_extents[0], 2 * half_extents[1], mu, B, int(ok.sum())))
    print("weight carried at rest %.1f N; largest |centre of pressure| / half extent along the retimed paths: x %.3f, y %.3f"
          % (w0[..., 2].mean(), np.abs(cop[..., 0]).max() / half_extents[0], np.abs(cop[..., 1]).max() / half_extents[1]))
    print("with joint velocity and acceleration limits alone: x %.3f, y %.3f (above 1: the cart tips)"
          % (np.abs(cop_free[..., 0]).max() / half_extents[0], np.abs(cop_free[..., 1]).max() / half_extents[1]))
    worst = (np.einsum("mk,bnk->bnm", con.F, w[:, :-1]) - con.g).max()
    print("largest F w - g along the retimed paths: %.3g (the cone holds where it is <= 0)" % worst)
    dur, dur0 = bt.compute_trajectory().duration, free.compute_trajectory().duration
    print("mean duration %.3f s, %.3f s with joint velocity and acceleration limits alone" % (np.nanmean(dur[ok]), np.nanmean(dur0[ok])))
    assert ok.all() and (ref["status"] == 0).all() and np.nanmean(dur) > np.nanmean(dur0)
    scale = np.abs(np.einsum("mk,bnk->bnm", np.abs(con.F), np.abs(w[:, :-1]))).max()
    assert worst <= 1e-9 * scale, worst
    assert np.abs(cop[..., 0]).max() <= half_extents[0] * (1 + 1e-9) and np.abs(cop[..., 1]).max() <= half_extents[1] * (1 + 1e-9)


if __name__ == "__main__":
    main()

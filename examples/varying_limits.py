"""Retime a batch under limits that depend on the position along the path: joint velocity limits halved in a slow zone in the
middle of the path, and a Cartesian tool-speed limit -- a bound on x = sd^2 alone -- beside constant acceleration limits.  Such
constraints only tighten the box of a stage's variables; BatchTOPPRA folds them into stage boxes on the GPU once per object.

    python examples/varying_limits.py [--batch 1024]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toppra_amd as ta  # noqa: E402
from toppra_amd.constraint import BatchBoundConstraint, BatchJointVelocityConstraintVarying  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    B = ap.parse_args().batch
    rng = np.random.default_rng(0)
    d, N = 6, 200
    s = np.linspace(0, 1, N + 1)
    # analytic paths q_k(s) = A_k sin(w_k s + phi_k), handed over as samples at the gridpoints
    A, w, phi = 0.5 + rng.random((B, 1, d)), 1 + 3 * rng.random((B, 1, d)), 6 * rng.random((B, 1, d))
    arg = w * s[None, :, None] + phi
    q, qs, qss = A * np.sin(arg), A * w * np.cos(arg), -A * w * w * np.sin(arg)
    alim = np.stack([-8 * np.ones((B, d)), 8 * np.ones((B, d))], -1)

    # a slow zone: half the joint speed on 0.4 < s < 0.6.  The callable is called once, with every gridpoint.
    def vlim_func(grid):
        vmax = np.where((grid > 0.4) & (grid < 0.6), 1.5, 3.0)[:, None, None] * np.ones((1, d, 1))
        return np.concatenate([-vmax, vmax], -1)  # [N+1, d, 2]: one grid of limits for the whole batch

    # a tool-speed limit |J q'| sd <= v_tool with the "tool" at the first three joints: x <= v_tool^2 / |J q'|^2
    v_tool = 2.0
    speed2 = (qs[:, :, :3] ** 2).sum(-1)
    xbound = np.stack([np.zeros((B, N + 1)), v_tool ** 2 / np.maximum(speed2, 1e-12)], -1)

    vlim = np.stack([-3 * np.ones((B, d)), 3 * np.ones((B, d))], -1)
    free = ta.algorithm.BatchTOPPRA.from_path_samples(s, q, qs, qss, vlim, alim)  # constant limits: the fused sampled entries
    bt = ta.algorithm.BatchTOPPRA.from_path_samples(s, q, qs, qss, None, alim,
                                                    constraints=[BatchJointVelocityConstraintVarying(vlim_func), BatchBoundConstraint(xbound=xbound)])
    out, ref = bt.compute_parameterization(), free.compute_parameterization()
    codes = ta.algorithm.BatchTOPPRA.return_codes(out["status"])
    zone = (s > 0.4) & (s < 0.6)
    jv = np.abs(qs * out["sd"][:, :, None])
    print("%d paths: %d Ok" % (B, sum(c.name == "Ok" for c in codes)))
    print("max joint speed in the slow zone %.3f (limit 1.5), outside %.3f (limit 3)" % (np.nanmax(jv[:, zone]), np.nanmax(jv[:, ~zone])))
    print("max tool speed %.3f (limit %.1f)" % (np.nanmax(np.sqrt(speed2) * out["sd"]), v_tool))
    dur, dur0 = bt.compute_trajectory().duration, free.compute_trajectory().duration
    print("mean duration %.3f s, %.3f s without the slow zone and the tool-speed limit" % (np.nanmean(dur), np.nanmean(dur0)))
    assert (ref["sd"] >= out["sd"] - 1e-9)[out["status"] == 0].all()


if __name__ == "__main__":
    main()

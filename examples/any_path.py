"""Retime paths that are not cubic splines: a ``SimplePath`` through the drop-in classes, and a batch of analytic paths given
as samples at the gridpoints -- the solver reads a path only through path(gridpoints, 0 / 1 / 2), so any path class works.

    python examples/any_path.py [--batch 1024]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toppra_amd as ta  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    B = ap.parse_args().batch
    rng = np.random.default_rng(0)

    # one SimplePath: positions and velocities at five points, as the reference's SimplePath takes them
    x = np.linspace(0, 1, 5)
    path = ta.SimplePath(x, rng.standard_normal((5, 3)), rng.standard_normal((5, 3)))
    cons = [ta.constraint.JointVelocityConstraint(2.0 * np.ones(3)), ta.constraint.JointAccelerationConstraint(5.0 * np.ones(3))]
    inst = ta.algorithm.TOPPRA(cons, path, gridpoints=np.linspace(0, 1, 101))
    traj = inst.compute_trajectory(0, 0)
    print("SimplePath: %s, duration %.3f s (%s)" % (inst.problem_data.return_code.name, traj.duration,
                                                    type(inst.solver_wrapper).__name__))

    # a batch of analytic paths q_k(s) = A_k sin(w_k s + phi_k), handed over as samples at the gridpoints
    d, N = 6, 200
    s = np.linspace(0, 1, N + 1)
    A, w, phi = 0.5 + rng.random((B, 1, d)), 1 + 3 * rng.random((B, 1, d)), 6 * rng.random((B, 1, d))
    arg = w * s[None, :, None] + phi
    q, qs, qss = A * np.sin(arg), A * w * np.cos(arg), -A * w * w * np.sin(arg)
    vlim = np.stack([-3 * np.ones((B, d)), 3 * np.ones((B, d))], -1)
    alim = np.stack([-8 * np.ones((B, d)), 8 * np.ones((B, d))], -1)
    bt = ta.algorithm.BatchTOPPRA.from_path_samples(s, q, qs, qss, vlim, alim)
    trajs = bt.compute_trajectory()
    dur = trajs.duration
    codes = ta.algorithm.BatchTOPPRA.return_codes(trajs.status)
    print("%d sampled paths: %d Ok, durations min %.3f  mean %.3f  max %.3f s" % (
        B, sum(c.name == "Ok" for c in codes), np.nanmin(dur), np.nanmean(dur), np.nanmax(dur)))
    qd = trajs(np.linspace(0, 1, 50)[None, :] * dur[:, None], order=1)
    print("max |dq/dt| over the batch: %.3f (limit 3)" % np.nanmax(np.abs(qd)))


if __name__ == "__main__":
    main()

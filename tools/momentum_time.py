#!/usr/bin/env python
"""Time the momentum kernel and, in the same run on the same points and stream, what it is measured against:

  momentum        batch.momentum_batch with a limit: momentum, energy2 and xbound in one launch -- rate on the algorithmic bytes
                  (2 d + 9) 8 per point
  momentum_bound  batch.momentum_bound_batch: the same launch asked for xbound alone, what BatchMomentumConstraint costs --
                  (2 d + 2) 8 bytes per point
  replaced        the route it replaces, pieced together from entries that existed before it: base_wrench_batch on a gravity-free
                  copy of the robot at (q, 0, qs) for the momentum, torque_terms at (q, qs, qss) and sum_j qs_j (wa - w0)_j for
                  energy2, and the torch reductions and divisions that make xbound
  points_speed    chain_points_speed_batch with 4 control points and a limit, a first-order peer -- on a chain alone (the entry
                  takes no tree): (2 d + 6) 8 bytes per point

    python tools/momentum_time.py [--batch 65536] [--grid 200] [--out profiles/momentum_time.json]

The models: a 7-dof chain, the 15-dof torso with two 7-dof arms (one fork), an 18-dof tree with one fork.  Protocol (that of
tools/base_wrench_time.py): device tensors, inputs resident, warm-up of every shape, then `--rounds` rounds in which the variants
are timed in turn, each timing `--reps` calls between two events on the stream; the figure is the median over the rounds and the
spread their (max - min) / median.  Before anything is timed the two routes are compared: xbound alone equals the full call's bit
for bit, and the replaced route's momentum and energy2 agree with the kernel's to 1e-9 of their largest value (two different
recursions: rounding, not bits; its bound is made from them by the same divisions).  Prints one JSON line per model and writes them to --out.  The expectation is a
comparison within the run, with the run's spread as its allowance:
  momentum_vs_replaced   momentum / replaced: below 1 by more than the two spreads"""
import os
import sys

import numpy as np

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toppra_amd import batch  # noqa: E402
from toppra_amd.chain import ControlPoints, KinematicTree, Mount, SerialChain  # noqa: E402

from base_wrench_time import models  # noqa: E402


def frame():
    c, s = np.cos(0.3), np.sin(0.3)
    return Mount(rotation=[[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], origin=(0.1, -0.2, -0.6))


def gravity_free(robot):
    """A copy of the robot without gravity: what the replaced route evaluates the base reaction on."""
    if isinstance(robot, SerialChain):
        return SerialChain(robot.joint_types, robot.axes, robot.rotations, robot.translations, robot.masses, robot.coms, robot.inertias,
                           gravity=(0.0, 0.0, 0.0), tool=robot.tool)
    return KinematicTree(robot.parents, robot.joint_types, robot.axes, robot.rotations, robot.translations, robot.masses, robot.coms,
                         robot.inertias, gravity=(0.0, 0.0, 0.0))


def main():
    import torch
    args = timing.parser(rounds=7, reps=5).parse_args()
    B, N = args.batch, args.grid
    dev = timing.device()
    mount = frame()
    results = []
    for name, robot in models():
        d = robot.dof
        q, qs, qss = timing.inputs(dev, B, N, d)
        zero = torch.zeros_like(q)
        floating = gravity_free(robot)
        limit = torch.tensor([4.0, 1.0, 6.0], dtype=torch.float64, device=dev).expand(B, 3).contiguous()

        def replaced():
            h = batch.base_wrench_batch(floating, q, zero, qs, mount)
            w0, wa, _ = robot.torque_terms(q, qs, qss)
            e2 = (qs * (wa - w0)).sum(-1)
            pp, ll = (h[..., :3] * h[..., :3]).sum(-1), (h[..., 3:] * h[..., 3:]).sum(-1)
            best = torch.minimum(torch.minimum(limit[:, None, 0] / pp, limit[:, None, 1] / ll), limit[:, None, 2] / e2)
            return h, e2, torch.stack((torch.zeros_like(best), best), -1)
        runs = {"momentum": lambda: batch.momentum_batch(robot, q, qs, mount, None, limit),
                "momentum_bound": lambda: batch.momentum_bound_batch(robot, q, qs, limit, mount),
                "replaced": replaced}
        if isinstance(robot, SerialChain):
            pts = ControlPoints([1, 3, 5, -1], np.full((4, 3), 0.1))
            runs["points_speed"] = lambda: batch.chain_points_speed_batch(robot, q, qs, pts, 0.25)
        outs = timing.warm_up(runs)
        assert torch.equal(outs["momentum"][2], outs["momentum_bound"]), (name, "xbound alone vs the full call")
        assert bool(torch.isfinite(outs["momentum"][2]).all()) and bool(torch.isfinite(outs["replaced"][2]).all()), name
        for k, what in enumerate(("momentum", "energy2")):
            a, b = outs["momentum"][k], outs["replaced"][k]
            assert bool(torch.isfinite(a).all()), (name, what)
            scale = float(a.abs().max())
            assert float((a - b).abs().max()) <= 1e-9 * scale, (name, what, float((a - b).abs().max()), scale)
        del outs
        torch.cuda.empty_cache()
        ms = timing.measure(runs, args.rounds, args.reps)
        points = B * (N + 1)
        rec = dict({"model": name, "forks": len(getattr(robot, "forks", ()))}, **timing.header(args, d))
        # (the replaced route: the base reaction reads three arrays and writes 6, the torque terms read three and write 3 d, the
        # reductions are counted as nothing)
        rec.update({"momentum_bytes": points * (2 * d + 9) * 8, "momentum_bound_bytes": points * (2 * d + 2) * 8,
                    "replaced_bytes": points * ((3 * d + 6) + 6 * d) * 8, "points_speed_bytes": points * (2 * d + 6) * 8})
        timing.record(rec, ms, gbps=True)
        rec["momentum_TBps"] = round(rec["momentum_GBps"] / 1e3, 3)
        rec["momentum_Mpoints_per_s"] = round(points / rec["momentum_ms"] / 1e3, 1)
        rec["momentum_vs_replaced"] = round(rec["momentum_ms"] / rec["replaced_ms"], 3)
        rec["faster_than_replaced"] = bool(rec["momentum_vs_replaced"] < 1.0 - rec["momentum_spread"] - rec["replaced_spread"])
        if "points_speed_ms" in rec:
            rec["momentum_vs_points_speed"] = round(rec["momentum_ms"] / rec["points_speed_ms"], 3)
        else:
            del rec["points_speed_bytes"]
        timing.emit(rec, results)
        del q, qs, qss, zero, limit
        torch.cuda.empty_cache()
    timing.write(results, args.out)


if __name__ == "__main__":
    main()

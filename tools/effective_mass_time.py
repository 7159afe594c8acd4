#!/usr/bin/env python
"""Time the effective-mass kernel and, in the same run on the same points and stream, two first-order peers for scale:

  effective_mass        contact.effective_mass_batch with 4 control points and a limit: speed2, mobility and xbound in one launch
  effective_mass_bound  contact.effective_mass_bound_batch: the same launch asked for xbound alone, what BatchContactEnergyConstraint
                        costs
  momentum              batch.momentum_batch with a limit (tpr_tree_momentum_batch): the forward-only walk the total-energy limit
                        costs
  points_speed          chain_points_speed_batch with the same 4 points and a limit -- on a chain alone (the entry takes no tree)

    python tools/effective_mass_time.py [--batch 65536] [--grid 200] [--out profiles/effective_mass_time.json]

The models: a 7-dof chain, the 15-dof torso with two 7-dof arms (one fork), an 18-dof tree with one fork; the points sit on the
last link, two middle links and link 1.  Protocol (tools/timing.py): device tensors, inputs resident, warm-up of every shape, then
`--rounds` rounds in which the variants are timed in turn, each timing `--reps` calls between two events on the stream; the figure
is the median over the rounds and the spread their (max - min) / median.  Before anything is timed xbound alone is compared with
the full call's bit for bit, the outputs are checked to be finite, and speed2 is compared with the control-point kernel's to 1e-12
of its largest value (two kernels, two orders of the sums).  The walk is set by arithmetic, not by memory: the rate is reported in
gridpoints per second, and the bytes moved only for scale.  Prints one JSON line per model and writes them to --out.  There is no
threshold on the time: the figures are measured and reported."""
import os
import sys

import numpy as np

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toppra_amd import batch, contact  # noqa: E402
from toppra_amd.chain import ControlPoints, SerialChain  # noqa: E402

from base_wrench_time import models  # noqa: E402

POINTS = 4


def main():
    import torch
    args = timing.parser(rounds=7, reps=5).parse_args()
    B, N = args.batch, args.grid
    dev = timing.device()
    results = []
    for name, robot in models():
        d = robot.dof
        q, qs, _ = timing.inputs(dev, B, N, d)
        pts = ControlPoints([-1, d // 2, d // 3, 1], np.array([[0.1, 0.0, 0.2], [0.0, 0.1, 0.1], [0.05, -0.1, 0.0], [0.1, 0.1, 0.1]]))
        limit = torch.tensor([[0.5, 0.1]], dtype=torch.float64, device=dev).expand(POINTS, 2).contiguous()
        mlimit = torch.tensor([4.0, 1.0, 6.0], dtype=torch.float64, device=dev).expand(B, 3).contiguous()
        runs = {"effective_mass": lambda: contact.effective_mass_batch(robot, q, qs, pts, limit),
                "effective_mass_bound": lambda: contact.effective_mass_bound_batch(robot, q, qs, pts, limit),
                "momentum": lambda: batch.momentum_batch(robot, q, qs, None, None, mlimit)}
        if isinstance(robot, SerialChain):
            runs["points_speed"] = lambda: batch.chain_points_speed_batch(robot, q, qs, pts, 0.25)
        outs = timing.warm_up(runs)
        assert torch.equal(outs["effective_mass"][2], outs["effective_mass_bound"]), (name, "xbound alone vs the full call")
        for k, what in enumerate(("speed2", "mobility", "xbound")):
            assert bool(torch.isfinite(outs["effective_mass"][k]).all()), (name, what)
        assert bool((outs["effective_mass"][1] > 0).all()), name
        if "points_speed" in outs:
            a, b = outs["effective_mass"][0], outs["points_speed"][0]
            assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max()), (name, "speed2 vs the control-point kernel")
        del outs
        torch.cuda.empty_cache()
        ms = timing.measure(runs, args.rounds, args.reps)
        points = B * (N + 1)
        rec = dict({"model": name, "forks": len(getattr(robot, "forks", ())), "control_points": POINTS}, **timing.header(args, d))
        rec.update({"effective_mass_bytes": points * (2 * d + 2 * POINTS + 2) * 8, "effective_mass_bound_bytes": points * (2 * d + 2) * 8,
                    "momentum_bytes": points * (2 * d + 9) * 8, "points_speed_bytes": points * (2 * d + POINTS + 2) * 8})
        timing.record(rec, ms, gbps=True)
        rec["effective_mass_Mpoints_per_s"] = round(points / rec["effective_mass_ms"] / 1e3, 1)
        rec["effective_mass_vs_momentum"] = round(rec["effective_mass_ms"] / rec["momentum_ms"], 3)
        if "points_speed_ms" in rec:
            rec["effective_mass_vs_points_speed"] = round(rec["effective_mass_ms"] / rec["points_speed_ms"], 3)
        else:
            del rec["points_speed_bytes"]
        timing.emit(rec, results)
        del q, qs, limit, mlimit
        torch.cuda.empty_cache()
    timing.write(results, args.out)


if __name__ == "__main__":
    main()

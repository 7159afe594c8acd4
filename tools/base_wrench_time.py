#!/usr/bin/env python
"""Time the base-reaction kernels and, in the same run on the same points and stream, what they are measured against:

  wrench_terms  batch.base_wrench_terms_batch: w0, wa, wb in one launch           -- rate on the algorithmic bytes (3 d + 18) 8
  wrench        batch.base_wrench_batch: one evaluation                           -- (3 d + 6) 8 bytes per point
  callback      the batched-callback route: three single launches (q, 0, 0), (q, 0, qs), (q, qs, qss)
  torque_terms  the robot's torque terms (chain_torque_terms_batch / tree_torque_terms_batch): the same recursion on the way up,
                a backward pass and a per-link state on top -- (6 d) 8 bytes per point

    python tools/base_wrench_time.py [--batch 65536] [--grid 200] [--out profiles/base_wrench_time.json]

The models: a 7-dof chain, the 15-dof torso with two 7-dof arms (one fork), an 18-dof tree with one fork (where the tree's torque
kernel runs its evaluations one after another).  Protocol (that of tools/tool_wrench_time.py): device tensors, inputs resident,
warm-up of every shape, then `--rounds` rounds in which the variants are timed in turn, each timing `--reps` calls between two
events on the stream; the figure is the median over the rounds and the spread their (max - min) / median.  Before anything is
timed the fused outputs are compared with the single entry bit for bit.  Prints one JSON line per model and writes them to
--out.  The two expectations are comparisons within the run, each with the run's spread as its allowance:
  fused_vs_callback   wrench_terms / callback: at most 1 + the two spreads
  fused_vs_torque     wrench_terms / torque_terms: at most 1 + the two spreads"""
import os
import sys

import numpy as np

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toppra_amd import batch  # noqa: E402
from toppra_amd.chain import Mount  # noqa: E402


def models():
    """(name, model) -- the test suite's random links (mixed joint types, tilted axes, rotated joint frames)."""
    from tests import chain_ref, tree_cases, tree_ref
    return [("chain7", chain_ref.serial_chain(chain_ref.random_chain(7, 20240924 + 7, prismatic_every=4))),
            ("torso15", tree_ref.kinematic_tree(tree_ref.random_tree(tree_cases.SHAPES["torso"], 20240924 + 15, prismatic_every=4))),
            ("y18", tree_ref.kinematic_tree(tree_ref.random_tree(tree_cases.SHAPES["y18"], 20240924 + 18, prismatic_every=4)))]


def mount():
    c, s = np.cos(0.3), np.sin(0.3)
    return Mount(rotation=[[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], origin=(0.1, -0.2, -0.6), mass=35.0, com=(0.02, 0.01, -0.4))


def main():
    import torch
    args = timing.parser(rounds=7, reps=5).parse_args()
    B, N = args.batch, args.grid
    dev = timing.device()
    frame = mount()
    results = []
    for name, robot in models():
        d = robot.dof
        q, qs, qss = timing.inputs(dev, B, N, d)
        zero = torch.zeros_like(q)

        def callback():
            return tuple(batch.base_wrench_batch(robot, *a, frame) for a in ((q, zero, zero), (q, zero, qs), (q, qs, qss)))
        runs = {"wrench_terms": lambda: batch.base_wrench_terms_batch(robot, q, qs, qss, frame),
                "wrench": lambda: batch.base_wrench_batch(robot, q, qs, qss, frame),
                "callback": callback,
                "torque_terms": lambda: robot.torque_terms(q, qs, qss)}
        outs = timing.warm_up(runs)
        for k, what in enumerate(("w0", "wa", "wb")):
            assert torch.equal(outs["wrench_terms"][k], outs["callback"][k]), (name, "fused %s vs the single entry" % what)
        assert torch.equal(outs["wrench_terms"][2], outs["wrench"]) and bool(torch.isfinite(outs["wrench"]).all())
        del outs
        torch.cuda.empty_cache()
        ms = timing.measure(runs, args.rounds, args.reps)
        points = B * (N + 1)
        rec = dict({"model": name, "forks": len(getattr(robot, "forks", ()))}, **timing.header(args, d))
        rec.update({"wrench_terms_bytes": points * (3 * d + 18) * 8, "wrench_bytes": points * (3 * d + 6) * 8,
                    "callback_bytes": 3 * points * (3 * d + 6) * 8, "torque_terms_bytes": points * 6 * d * 8})
        timing.record(rec, ms, gbps=True)
        rec["wrench_terms_Mpoints_per_s"] = round(points / rec["wrench_terms_ms"] / 1e3, 1)
        rec["fused_vs_callback"] = round(rec["wrench_terms_ms"] / rec["callback_ms"], 3)
        rec["fused_vs_torque"] = round(rec["wrench_terms_ms"] / rec["torque_terms_ms"], 3)
        rec["not_slower_than_callback"] = bool(rec["fused_vs_callback"] <= 1.0 + rec["wrench_terms_spread"] + rec["callback_spread"])
        rec["not_slower_than_torque_terms"] = bool(rec["fused_vs_torque"] <= 1.0 + rec["wrench_terms_spread"] + rec["torque_terms_spread"])
        timing.emit(rec, results)
        del q, qs, qss, zero
        torch.cuda.empty_cache()
    timing.write(results, args.out)


if __name__ == "__main__":
    main()

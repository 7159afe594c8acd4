#!/usr/bin/env python
"""Time the tool-wrench kernels and, in the same run on the same points and stream, what they are measured against:

  wrench_terms  batch.chain_tool_wrench_terms_batch: w0, wa, wb in one launch     -- rate on the algorithmic bytes (3 d + 18) 8
  wrench        batch.chain_tool_wrench_batch: one evaluation                     -- (3 d + 6) 8 bytes per point
  callback      the batched-callback route: three single launches (q, 0, 0), (q, 0, qs), (q, qs, qss)
  accel_terms   batch.chain_tool_acceleration_terms_batch: wa, wb in one launch (the yardstick: two evaluations with the
                accumulated world rotation, where wrench_terms runs three without it)

    python tools/tool_wrench_time.py [--batch 65536] [--grid 200] [--dofs 7 12 20] [--out profiles/tool_wrench_time.json]

Protocol (that of tools/tool_accel_time.py): device tensors, inputs resident, warm-up of every shape, then `--rounds` rounds in
which the variants are timed in turn, each timing `--reps` calls between two events on the stream; the figure is the median
over the rounds and the spread their (max - min) / median.  Before anything is timed the fused outputs are compared with the
single entry bit for bit.  Prints one JSON line per dof and writes them to --out.  The two expectations are comparisons within
the run, each with the run's spread as its allowance:
  fused_vs_callback        wrench_terms / callback: at most 1 + the two spreads
  fused_vs_accel_scaled    wrench_terms / (1.5 accel_terms), the yardstick scaled for the third evaluation: at most 1 + the two spreads"""
import os
import sys

import numpy as np

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toppra_amd import batch  # noqa: E402
from toppra_amd.chain import Payload  # noqa: E402


def random_chain(d, seed):
    """The test suite's random chain (mixed joint types, tilted axes, rotated joint frames) as a SerialChain."""
    from tests import chain_ref
    return chain_ref.serial_chain(chain_ref.random_chain(d, seed, prismatic_every=4))


def payload():
    c, s = np.cos(0.3), np.sin(0.3)
    return Payload(1.7, com=(0.02, -0.05, 0.11), inertia=(0.03, 0.04, 0.05, 0.002, -0.003, 0.004),
                   frame_rotation=[[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], frame_origin=(0.01, 0.02, 0.03))


def main():
    import torch
    args = timing.parser(rounds=7, reps=5, dofs=(7, 12, 20)).parse_args()
    B, N = args.batch, args.grid
    dev = timing.device()
    obj = payload()
    results = []
    for d in args.dofs:
        chain = random_chain(d, 20240924 + d)
        q, qs, qss = timing.inputs(dev, B, N, d)
        zero = torch.zeros_like(q)

        def callback():
            return tuple(batch.chain_tool_wrench_batch(chain, *a, obj) for a in ((q, zero, zero), (q, zero, qs), (q, qs, qss)))
        runs = {"wrench_terms": lambda: batch.chain_tool_wrench_terms_batch(chain, q, qs, qss, obj),
                "wrench": lambda: batch.chain_tool_wrench_batch(chain, q, qs, qss, obj),
                "callback": callback,
                "accel_terms": lambda: batch.chain_tool_acceleration_terms_batch(chain, q, qs, qss)}
        outs = timing.warm_up(runs)
        for k, what in enumerate(("w0", "wa", "wb")):
            assert torch.equal(outs["wrench_terms"][k], outs["callback"][k]), (d, "fused %s vs the single entry" % what)
        assert torch.equal(outs["wrench_terms"][2], outs["wrench"]) and bool(torch.isfinite(outs["wrench"]).all())
        del outs
        torch.cuda.empty_cache()
        ms = timing.measure(runs, args.rounds, args.reps)
        points = B * (N + 1)
        rec = timing.header(args, d)
        rec.update({"wrench_terms_bytes": points * (3 * d + 18) * 8, "wrench_bytes": points * (3 * d + 6) * 8,
                    "callback_bytes": 3 * points * (3 * d + 6) * 8, "accel_terms_bytes": points * (3 * d + 12) * 8})
        timing.record(rec, ms, gbps=True)
        rec["wrench_terms_Mpoints_per_s"] = round(points / rec["wrench_terms_ms"] / 1e3, 1)
        rec["fused_vs_callback"] = round(rec["wrench_terms_ms"] / rec["callback_ms"], 3)
        rec["fused_vs_accel_scaled"] = round(rec["wrench_terms_ms"] / (1.5 * rec["accel_terms_ms"]), 3)
        rec["not_slower_than_callback"] = bool(rec["fused_vs_callback"] <= 1.0 + rec["wrench_terms_spread"] + rec["callback_spread"])
        rec["within_scaled_accel_terms"] = bool(rec["fused_vs_accel_scaled"] <= 1.0 + rec["wrench_terms_spread"] + rec["accel_terms_spread"])
        timing.emit(rec, results)
        del q, qs, qss, zero
        torch.cuda.empty_cache()
    timing.write(results, args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time the tool-acceleration kernels and, in the same run on the same points and stream, the chain kernels they are measured
against:

  accel_terms   batch.chain_tool_acceleration_terms_batch: wa, wb in one launch   -- rate on the algorithmic bytes (3 d + 12) 8
  accel         batch.chain_tool_acceleration_batch: one evaluation               -- (3 d + 6) 8 bytes per point
  torque_terms  batch.chain_torque_terms_batch: w0, wa, wb of the torque constraint (the yardstick: three evaluations with a
                backward pass and per-link state, where accel_terms runs two forward recursions in registers)
  tool_velocity batch.chain_tool_bound_batch: vSv and the bound

    python tools/tool_accel_time.py [--batch 65536] [--grid 200] [--dofs 7 12 20] [--out profiles/tool_accel_time.json]

Protocol (that of tools/chain_dynamics_time.py): device tensors, inputs resident, warm-up of every shape, then `--rounds`
rounds in which the variants are timed in turn, each timing `--reps` calls between two events on the stream; the figure is the
median over the rounds and the spread their (max - min) / median.  Before anything is timed the fused outputs are compared
with the single entry bit for bit.  Prints one JSON line per dof and writes them to --out.  `ratio_to_torque_terms` is
accel_terms over torque_terms: above 1 the new kernel takes longer than the yardstick."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toppra_amd import batch  # noqa: E402


def random_chain(d, seed):
    """The test suite's random chain (mixed joint types, tilted axes, rotated joint frames) as a SerialChain."""
    from tests import chain_ref
    return chain_ref.serial_chain(chain_ref.random_chain(d, seed, prismatic_every=4))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--dofs", type=int, nargs="+", default=[7, 12, 20])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, N = args.batch, args.grid
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda", 0)
    results = []
    for d in args.dofs:
        chain = random_chain(d, 20240924 + d)
        gen = torch.Generator(device=dev).manual_seed(d)
        q = 6.0 * torch.rand((B, N + 1, d), dtype=torch.float64, device=dev, generator=gen) - 3.0
        qs = torch.randn((B, N + 1, d), dtype=torch.float64, device=dev, generator=gen)
        qss = 2.0 * torch.randn((B, N + 1, d), dtype=torch.float64, device=dev, generator=gen)
        runs = {"accel_terms": lambda: batch.chain_tool_acceleration_terms_batch(chain, q, qs, qss),
                "accel": lambda: batch.chain_tool_acceleration_batch(chain, q, qs, qss),
                "torque_terms": lambda: batch.chain_torque_terms_batch(chain, q, qs, qss),
                "tool_velocity": lambda: batch.chain_tool_bound_batch(chain, q, qs, 0.25)}
        outs = {name: fn() for name, fn in runs.items()}  # warm-up of every shape, and the values
        torch.cuda.synchronize()
        assert torch.equal(outs["accel_terms"][1], outs["accel"]), (d, "fused wb vs the single entry")
        assert torch.equal(outs["accel_terms"][0], batch.chain_tool_acceleration_batch(chain, q, torch.zeros_like(q), qs)), (d, "fused wa")
        assert bool(torch.isfinite(outs["accel"]).all())
        del outs
        torch.cuda.empty_cache()
        ms = {name: [] for name in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / args.reps)
        points = B * (N + 1)
        rec = {"B": B, "N": N, "d": d, "rounds": args.rounds, "reps": args.reps, "date": time.strftime("%Y-%m-%d"),
               "accel_terms_bytes": points * (3 * d + 12) * 8, "accel_bytes": points * (3 * d + 6) * 8,
               "torque_terms_bytes": points * 6 * d * 8, "tool_velocity_bytes": points * (2 * d + 3) * 8}
        for name, v in ms.items():
            med = float(np.median(v))
            rec[name + "_ms"] = round(med, 4)
            rec[name + "_spread"] = round((max(v) - min(v)) / med, 4)
            rec[name + "_GBps"] = round(rec[name + "_bytes"] / med / 1e6, 1)
        rec["accel_terms_Mpoints_per_s"] = round(points / rec["accel_terms_ms"] / 1e3, 1)
        rec["ratio_to_torque_terms"] = round(rec["accel_terms_ms"] / rec["torque_terms_ms"], 3)
        rec["not_slower_than_torque_terms"] = bool(rec["accel_terms_ms"] <= rec["torque_terms_ms"])
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del q, qs, qss
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

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
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toppra_amd import batch  # noqa: E402


def random_chain(d, seed):
    """The test suite's random chain (mixed joint types, tilted axes, rotated joint frames) as a SerialChain."""
    from tests import chain_ref
    return chain_ref.serial_chain(chain_ref.random_chain(d, seed, prismatic_every=4))


def main():
    import torch
    args = timing.parser(rounds=7, reps=5, dofs=(7, 12, 20)).parse_args()
    B, N = args.batch, args.grid
    dev = timing.device()
    results = []
    for d in args.dofs:
        chain = random_chain(d, 20240924 + d)
        q, qs, qss = timing.inputs(dev, B, N, d)
        runs = {"accel_terms": lambda: batch.chain_tool_acceleration_terms_batch(chain, q, qs, qss),
                "accel": lambda: batch.chain_tool_acceleration_batch(chain, q, qs, qss),
                "torque_terms": lambda: batch.chain_torque_terms_batch(chain, q, qs, qss),
                "tool_velocity": lambda: batch.chain_tool_bound_batch(chain, q, qs, 0.25)}
        outs = timing.warm_up(runs)
        assert torch.equal(outs["accel_terms"][1], outs["accel"]), (d, "fused wb vs the single entry")
        assert torch.equal(outs["accel_terms"][0], batch.chain_tool_acceleration_batch(chain, q, torch.zeros_like(q), qs)), (d, "fused wa")
        assert bool(torch.isfinite(outs["accel"]).all())
        del outs
        torch.cuda.empty_cache()
        ms = timing.measure(runs, args.rounds, args.reps)
        points = B * (N + 1)
        rec = timing.header(args, d)
        rec.update({"accel_terms_bytes": points * (3 * d + 12) * 8, "accel_bytes": points * (3 * d + 6) * 8,
                    "torque_terms_bytes": points * 6 * d * 8, "tool_velocity_bytes": points * (2 * d + 3) * 8})
        timing.record(rec, ms, gbps=True)
        rec["accel_terms_Mpoints_per_s"] = round(points / rec["accel_terms_ms"] / 1e3, 1)
        rec["ratio_to_torque_terms"] = round(rec["accel_terms_ms"] / rec["torque_terms_ms"], 3)
        rec["not_slower_than_torque_terms"] = bool(rec["accel_terms_ms"] <= rec["torque_terms_ms"])
        timing.emit(rec, results)
        del q, qs, qss
        torch.cuda.empty_cache()
    timing.write(results, args.out)


if __name__ == "__main__":
    main()

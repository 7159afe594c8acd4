#!/usr/bin/env python
"""Time the control-point kernels with P points and, in the same run on the same path points and stream, the P launches of the
tool kernels on cut chains that they replace (what the batched-callback route costs without them):

  points_terms   batch.chain_points_acceleration_terms_batch: wa, wb of P points in one launch
  tool_terms_xP  P x batch.chain_tool_acceleration_terms_batch, each on the chain cut after its point's link, fed q[..., :k+1]
                 (as the callback route feeds them: a strided view, which the entry copies to a contiguous tensor first)
  points_speed   batch.chain_points_speed_batch with a limit: the squared speeds and the one bound of the set
  tool_speed_xP  P x batch.chain_tool_bound_batch with a limit on the cut chains, plus the P - 1 minima that fold their bounds

    python tools/control_points_time.py [--batch 65536] [--grid 200] [--dofs 7 12 20] [--points 4] [--out profiles/control_points_time.json]

The points sit on links round(d (p + 1) / P) - 1, p = 0 .. P-1: spread over the chain, the last one on the last link.

Protocol (that of tools/tool_accel_time.py): device tensors, inputs resident, warm-up of every shape, then `--rounds` rounds in
which the variants are timed in turn, each timing `--reps` calls between two events on the stream; the figure is the median over
the rounds and the spread their (max - min) / median.  Before anything is timed the fused outputs are compared with the tool
kernels' bit for bit.  Prints one JSON line per dof and writes them to --out.  `terms_ratio` / `speed_ratio` are the fused launch
over the P launches: above 1 the new kernel takes longer than what it replaces; `*_not_slower` allows the run's own spread (the
larger of the two variants')."""
import os
import sys
import time

import numpy as np

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toppra_amd import batch  # noqa: E402
from toppra_amd.chain import ControlPoints  # noqa: E402


def main():
    import torch
    from tests import chain_ref, control_points_cases as cp
    ap = timing.parser(rounds=7, reps=5, dofs=(7, 12, 20))
    ap.add_argument("--points", type=int, default=4)
    args = ap.parse_args()
    B, N, P = args.batch, args.grid, args.points
    dev = timing.device()
    results = []
    for d in args.dofs:
        model = chain_ref.random_chain(d, 20240924 + d, prismatic_every=4)
        chain = chain_ref.serial_chain(model)
        links = [max(int(round(d * (p + 1) / P)) - 1, 0) for p in range(P)]
        offsets = np.random.default_rng(d).uniform(-0.25, 0.25, (P, 3))
        points = ControlPoints(links, offsets)
        cuts = [(k, chain_ref.serial_chain(cp.truncated(model, k, r))) for k, r in zip(links, offsets)]
        q, qs, qss = timing.inputs(dev, B, N, d)
        limit = torch.full((B, P), 0.25, dtype=torch.float64, device=dev)

        def tool_terms():
            return [batch.chain_tool_acceleration_terms_batch(sc, q[..., :k + 1], qs[..., :k + 1], qss[..., :k + 1]) for k, sc in cuts]

        def tool_speed():
            outs = [batch.chain_tool_bound_batch(sc, q[..., :k + 1], qs[..., :k + 1], limit[:, p].contiguous()) for p, (k, sc) in enumerate(cuts)]
            bound = outs[0][1]
            for o in outs[1:]:
                bound = torch.minimum(bound, o[1])
            return outs, bound

        runs = {"points_terms": lambda: batch.chain_points_acceleration_terms_batch(chain, q, qs, qss, points),
                "tool_terms_xP": tool_terms,
                "points_speed": lambda: batch.chain_points_speed_batch(chain, q, qs, points, limit),
                "tool_speed_xP": tool_speed}
        outs = timing.warm_up(runs)
        for p in range(P):
            for i in range(2):
                assert torch.equal(outs["points_terms"][i][..., p, :], outs["tool_terms_xP"][p][i][..., :3]), (d, p, "terms")
            assert torch.equal(outs["points_speed"][0][..., p], outs["tool_speed_xP"][0][p][0]), (d, p, "speed")
        assert torch.equal(outs["points_speed"][1], outs["tool_speed_xP"][1]), (d, "bound")
        assert bool(torch.isfinite(outs["points_terms"][1]).all())
        del outs
        torch.cuda.empty_cache()
        for fn in runs.values():  # once more, untimed: the outputs' memory comes back from the allocator's cache, not the driver
            fn()
        torch.cuda.synchronize()
        ms = timing.measure(runs, args.rounds, args.reps)
        npoints = B * (N + 1)
        rec = {"B": B, "N": N, "d": d, "P": P, "links": links, "rounds": args.rounds, "reps": args.reps, "date": time.strftime("%Y-%m-%d"),
               "points_terms_bytes": npoints * (3 * (max(links) + 1) + 6 * P) * 8, "points_speed_bytes": npoints * (2 * (max(links) + 1) + P + 2) * 8}
        timing.record(rec, ms)
        for fused, many, key in (("points_terms", "tool_terms_xP", "terms"), ("points_speed", "tool_speed_xP", "speed")):
            rec[fused + "_GBps"] = round(rec[fused + "_bytes"] / rec[fused + "_ms"] / 1e6, 1)
            rec[key + "_ratio"] = round(rec[fused + "_ms"] / rec[many + "_ms"], 3)
            spread = max(rec[fused + "_spread"], rec[many + "_spread"])
            rec[key + "_not_slower"] = bool(rec[fused + "_ms"] <= rec[many + "_ms"] * (1.0 + spread))
        timing.emit(rec, results)
        del q, qs, qss
        torch.cuda.empty_cache()
    timing.write(results, args.out)


if __name__ == "__main__":
    main()

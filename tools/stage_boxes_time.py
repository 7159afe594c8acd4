#!/usr/bin/env python
"""Time the stage-box kernel and the boxed sampled solve against their alternatives, in one process, on the same problem and
stream:

  boxes            batch.stage_boxes_batch with one grid source (limits per gridpoint)      -- bandwidth on 8 (d + 2 d) + 32 bytes
  params           batch.constraint_params_batch (params_tile_kernel: the row-writing yardstick) -- bandwidth on the bytes it writes
  boxes+boxed      batch.stage_boxes_batch + batch.solve_sampled_boxed_batch                 (the new route for varying limits)
  rows+dense       batch.sampled_rows_batch (no vlim) + the boxes copied into low / high + batch.solve_dense_batch
                   (the route a user had before, with the boxes themselves for free)
  boxed const      batch.solve_sampled_boxed_batch on the boxes of a CONSTANT grid of limits   (boxes built once, not timed)
  sampled const    batch.solve_sampled_batch with the same constant vlim                       (the bound recomputed per stage)

    python tools/stage_boxes_time.py [--batch 65536] [--grid 200] [--dofs 7 12 20] [--out profiles/stage_boxes_time.json]

Protocol (that of tools/sampled_path_time.py): device tensors, warm-up of every shape, then `--rounds` rounds in which the
variants are timed in turn (so that drift hits all alike), each timing `--reps` calls between two events on the stream; the
figure is the median over the rounds and the spread their (max - min) / median.  Results are compared bit for bit before
anything is timed.  Prints one JSON line per dof and writes them to --out."""
import os
import sys

import numpy as np

import timing

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from toppra_amd import batch  # noqa: E402


def main():
    import torch
    args = timing.parser(rounds=7, reps=3, dofs=(7, 12, 20)).parse_args()
    B, N = args.batch, args.grid
    results = []

    def same(x, y, what):
        for key in ("sd2", "u", "K", "status"):
            kind = torch.int64 if key != "status" else torch.int32
            assert torch.equal(x[key].view(kind), y[key].view(kind)), (what, key)

    for d in args.dofs:
        data = batch.make_synthetic_batch(B, d, N, seed=20240924 + d)
        dev = {k: torch.from_numpy(np.ascontiguousarray(data[k])).cuda() for k in ("coef", "breaks", "grid", "vlim", "alim")}
        pe = batch.path_eval_batch(dev["coef"], dev["breaks"], dev["grid"], orders=(1, 2))
        grid, qs, qss, vlim, alim = dev["grid"], pe["qs"], pe["qss"], dev["vlim"], dev["alim"]
        scale = 1 + 0.5 * torch.sin(9 * grid)  # limits that depend on the position along the path
        vgrid = (vlim[:, None] * scale[None, :, None, None]).contiguous()
        vconst = vlim[:, None].expand(B, N + 1, d, 2).contiguous()
        low_c, high_c = batch.stage_boxes_batch(qs, [("vlim_grid", vconst)])
        del vconst
        keys = ("a", "b", "c", "low", "high", "deltas")

        def boxes():
            return batch.stage_boxes_batch(qs, [("vlim_grid", vgrid)])

        def params():
            return batch.constraint_params_batch(dev["coef"], dev["breaks"], grid, vlim, alim)

        def boxes_boxed():
            low, high = batch.stage_boxes_batch(qs, [("vlim_grid", vgrid)])
            return batch.solve_sampled_boxed_batch(grid, qs, qss, alim, low, high)

        low_v, high_v = boxes()

        def rows_dense():
            r = batch.sampled_rows_batch(grid, qs, qss, None, alim)
            r["low"].copy_(low_v); r["high"].copy_(high_v)
            return batch.solve_dense_batch(*[r[k] for k in keys])

        def boxed_const():
            return batch.solve_sampled_boxed_batch(grid, qs, qss, alim, low_c, high_c)

        def sampled_const():
            return batch.solve_sampled_batch(grid, qs, qss, vlim, alim)

        runs = {"boxes": boxes, "params": params, "boxes+boxed": boxes_boxed, "rows+dense": rows_dense, "boxed_const": boxed_const,
                "sampled_const": sampled_const}
        outs = timing.warm_up(runs)
        same(outs["boxes+boxed"], outs["rows+dense"], (d, "boxes+boxed vs rows+dense"))
        same(outs["boxed_const"], outs["sampled_const"], (d, "boxed vs sampled, constant limits"))
        params_bytes = sum(v.numel() * 8 for v in outs["params"].values())
        ok = int((outs["boxes+boxed"]["status"] == 0).sum())
        del outs
        ms = timing.measure(runs, args.rounds, args.reps)
        boxes_bytes = (8 * 3 * d + 32) * B * (N + 1)
        rec = timing.header(args, d)
        rec.update({"ok": ok, "boxes_bytes": boxes_bytes, "params_bytes": params_bytes})
        timing.record(rec, ms)
        rec["boxes_GBps"] = round(boxes_bytes / rec["boxes_ms"] / 1e6, 1)
        rec["params_GBps"] = round(params_bytes / rec["params_ms"] / 1e6, 1)
        rec["boxes+boxed_not_slower_than_rows+dense"] = bool(
            rec["boxes+boxed_ms"] <= rec["rows+dense_ms"] * (1 + max(rec["boxes+boxed_spread"], rec["rows+dense_spread"])))
        rec["boxed_const_over_sampled_const"] = round(rec["boxed_const_ms"] / rec["sampled_const_ms"], 4)
        timing.emit(rec, results)
        del dev, pe, qs, qss, vgrid, low_c, high_c, low_v, high_v
        torch.cuda.empty_cache()
    timing.write(results, args.out)


if __name__ == "__main__":
    main()

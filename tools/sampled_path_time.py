#!/usr/bin/env python
"""Time the fused sampled solve against its alternatives, in one process, on the same problem and stream:

  sampled        batch.solve_sampled_batch                       (rows produced in registers from q', q'')
  rows+dense     batch.sampled_rows_batch + batch.solve_dense_batch   (rows materialised, then read back)
  dense          batch.solve_dense_batch alone on the spline-built rows (what the library could do before: the yardstick)

    python tools/sampled_path_time.py [--batch 65536] [--grid 200] [--dofs 7 12 20] [--out profiles/NAME.json]

Protocol: device tensors, warm-up of every shape, then `--rounds` rounds in which the three are timed in turn (so that drift hits
all three alike), each timing `--reps` calls between two events on the stream; the figure is the median over the rounds and the
spread their (max - min) / median.  The three results are compared bit for bit before anything is timed.  Prints one JSON line
per dof and writes them to --out."""
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
    for d in args.dofs:
        data = batch.make_synthetic_batch(B, d, N, seed=20240924 + d)
        dev = {k: torch.from_numpy(np.ascontiguousarray(data[k])).cuda() for k in ("coef", "breaks", "grid", "vlim", "alim")}
        pe = batch.path_eval_batch(dev["coef"], dev["breaks"], dev["grid"], orders=(1, 2))
        sargs = (dev["grid"], pe["qs"], pe["qss"], dev["vlim"], dev["alim"])
        rows = batch.sampled_rows_batch(*sargs)
        keys = ("a", "b", "c", "low", "high", "deltas")

        def sampled():
            return batch.solve_sampled_batch(*sargs)

        def rows_dense():
            r = batch.sampled_rows_batch(*sargs)
            return batch.solve_dense_batch(*[r[k] for k in keys])

        def dense():
            return batch.solve_dense_batch(*[rows[k] for k in keys])

        runs = {"sampled": sampled, "rows+dense": rows_dense, "dense": dense}
        outs = timing.warm_up(runs)
        for name in ("rows+dense", "dense"):
            for key in ("sd2", "u", "K", "status"):
                assert torch.equal(outs["sampled"][key].view(torch.int64 if key != "status" else torch.int32),
                                   outs[name][key].view(torch.int64 if key != "status" else torch.int32)), (d, name, key)
        del outs
        ms = timing.measure(runs, args.rounds, args.reps)
        rec = timing.header(args, d)
        rec.update({"bytes_samples": 2 * 8 * B * (N + 1) * d, "bytes_rows": 3 * 8 * B * (N + 1) * (2 + 4 * d)})
        timing.record(rec, ms)
        rec["sampled_not_slower_than_rows+dense"] = bool(
            rec["sampled_ms"] <= rec["rows+dense_ms"] * (1 + max(rec["sampled_spread"], rec["rows+dense_spread"])))
        timing.emit(rec, results)
        del dev, pe, rows, sargs
        torch.cuda.empty_cache()
    timing.write(results, args.out)


if __name__ == "__main__":
    main()

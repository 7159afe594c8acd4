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
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from toppra_amd import batch  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--dofs", type=int, nargs="+", default=[7, 12, 20])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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
        outs = {name: fn() for name, fn in runs.items()}  # warm-up of every shape, and the bits
        torch.cuda.synchronize()
        for name in ("rows+dense", "dense"):
            for key in ("sd2", "u", "K", "status"):
                assert torch.equal(outs["sampled"][key].view(torch.int64 if key != "status" else torch.int32),
                                   outs[name][key].view(torch.int64 if key != "status" else torch.int32)), (d, name, key)
        del outs
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
        rec = {"B": B, "N": N, "d": d, "rounds": args.rounds, "reps": args.reps, "date": time.strftime("%Y-%m-%d"),
               "bytes_samples": 2 * 8 * B * (N + 1) * d, "bytes_rows": 3 * 8 * B * (N + 1) * (2 + 4 * d)}
        for name, v in ms.items():
            med = float(np.median(v))
            rec[name + "_ms"] = round(med, 4)
            rec[name + "_spread"] = round((max(v) - min(v)) / med, 4)
        rec["sampled_not_slower_than_rows+dense"] = bool(
            rec["sampled_ms"] <= rec["rows+dense_ms"] * (1 + max(rec["sampled_spread"], rec["rows+dense_spread"])))
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del dev, pe, rows, sargs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()

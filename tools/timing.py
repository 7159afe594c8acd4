"""The measurement protocol the timing tools share (tools/*_time.py): device tensors, inputs resident, a warm-up call of every
variant, then ``--rounds`` rounds in which the variants are timed in turn, each timing ``--reps`` calls between two events on the
stream; a variant's figure is the median over the rounds and its spread their (max - min) / median.  A tool keeps what is its own:
models, variants, byte counts, the bit-equality asserts before anything is timed, derived ratios and verdicts."""
import argparse
import json
import os
import time

import numpy as np


def parser(rounds, reps, dofs=None):
    """--batch, --grid, --rounds, --reps, --out, and --dofs where the tool runs one model per dof."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--grid", type=int, default=200)
    if dofs is not None:
        ap.add_argument("--dofs", type=int, nargs="+", default=list(dofs))
    ap.add_argument("--rounds", type=int, default=rounds)
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--out", default=None)
    return ap


def device():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    return torch.device("cuda", 0)


def inputs(dev, B, N, d):
    """q in [-3, 3), q' ~ N(0, 1), q'' ~ N(0, 4), [B, N+1, d] float64 on the device, seeded by the dof."""
    import torch
    gen = torch.Generator(device=dev).manual_seed(d)
    q = 6.0 * torch.rand((B, N + 1, d), dtype=torch.float64, device=dev, generator=gen) - 3.0
    qs = torch.randn((B, N + 1, d), dtype=torch.float64, device=dev, generator=gen)
    qss = 2.0 * torch.randn((B, N + 1, d), dtype=torch.float64, device=dev, generator=gen)
    return q, qs, qss


def _fn(run):
    return run[0] if isinstance(run, tuple) else run


def warm_up(runs):
    """One call of every variant -- the warm-up of every shape -- and its values, for the caller's asserts."""
    import torch
    outs = {name: _fn(run)() for name, run in runs.items()}
    torch.cuda.synchronize()
    return outs


def measure(runs, rounds, reps):
    """{variant: [ms per call, one per round]}; ``runs`` is {variant: fn}, or (fn, reps of its own) for a variant that takes long."""
    import torch
    ms = {name: [] for name in runs}
    for _ in range(rounds):
        for name, run in runs.items():
            fn, n = run if isinstance(run, tuple) else (run, reps)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / n)
    return ms


def header(args, d):
    return {"B": args.batch, "N": args.grid, "d": d, "rounds": args.rounds, "reps": args.reps, "date": time.strftime("%Y-%m-%d")}


def record(rec, ms, gbps=False):
    """<variant>_ms (the median) and <variant>_spread into ``rec``; with ``gbps`` also <variant>_GBps from rec[<variant>_bytes]."""
    for name, v in ms.items():
        med = float(np.median(v))
        rec[name + "_ms"] = round(med, 4)
        rec[name + "_spread"] = round((max(v) - min(v)) / med, 4)
        if gbps:
            rec[name + "_GBps"] = round(rec[name + "_bytes"] / med / 1e6, 1)


def emit(rec, results):
    print(json.dumps(rec), flush=True)
    results.append(rec)


def write(results, out):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            json.dump(results, fh, indent=1)
            fh.write("\n")

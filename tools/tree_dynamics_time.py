#!/usr/bin/env python
"""Time the tree kernels against the chain kernels, in one process, on the same points and stream:

  15 dof   tree_torso    batch.tree_torque_terms_batch on a torso joint carrying two 7-dof arms (one fork: the fused state)
           tree_chain    the same entry on a chain-shaped 15-dof tree (no fork: what the walk itself costs)
           chain         batch.chain_torque_terms_batch on that chain (chain_torque_terms_lds_kernel: the yardstick)
  18 dof   tree_y18      one fork at 18 dof: the three evaluations one after another in one launch
           tree_chain    a chain-shaped 18-dof tree (no fork: still the fused state)
           chain         the 18-dof chain

    python tools/tree_dynamics_time.py [--batch 65536] [--grid 200] [--out profiles/tree_dynamics_time.json]

Protocol (that of tools/chain_dynamics_time.py): device tensors, warm-up of every shape, then `--rounds` rounds in which the
variants are timed in turn, each timing `--reps` calls between two events on the stream; the figure is the median over the
rounds and the spread their (max - min) / median.  Before anything is timed the chain-shaped tree's outputs are compared with
the chain's bit for bit.  Prints one JSON line per dof and writes them to --out."""
import os
import sys
import time

import numpy as np

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toppra_amd import batch  # noqa: E402
from toppra_amd.chain import KinematicTree  # noqa: E402


def main():
    import torch
    from tests import chain_ref, tree_cases, tree_ref
    args = timing.parser(rounds=5, reps=3).parse_args()
    B, N = args.batch, args.grid
    dev = timing.device()
    results = []
    for d, shape in ((15, "torso"), (18, "y18")):
        links = chain_ref.random_chain(d, 20240924 + d, prismatic_every=4)
        chain = chain_ref.serial_chain(links)
        branched = tree_ref.kinematic_tree(dict(links, parent=np.array(tree_cases.SHAPES[shape], dtype=np.int32)))
        straight = KinematicTree.from_chain(chain)
        q, qs, qss = timing.inputs(dev, B, N, d)
        runs = {"tree_" + shape: lambda: batch.tree_torque_terms_batch(branched, q, qs, qss),
                "tree_chain": lambda: batch.tree_torque_terms_batch(straight, q, qs, qss),
                "chain": lambda: batch.chain_torque_terms_batch(chain, q, qs, qss)}
        outs = timing.warm_up(runs)
        for x, y in zip(outs["tree_chain"], outs["chain"]):
            assert torch.equal(x, y), (d, "chain-shaped tree vs chain")
        assert all(bool(torch.isfinite(x).all()) for x in outs["tree_" + shape])
        del outs
        torch.cuda.empty_cache()
        ms = timing.measure(runs, args.rounds, args.reps)
        points = B * (N + 1)
        rec = {"B": B, "N": N, "d": d, "shape": shape, "forks": len(branched.forks), "rounds": args.rounds, "reps": args.reps,
               "date": time.strftime("%Y-%m-%d"), "bytes": 6 * points * d * 8}
        timing.record(rec, ms)
        rec["tree_%s_over_chain" % shape] = round(rec["tree_%s_ms" % shape] / rec["chain_ms"], 3)
        rec["tree_chain_over_chain"] = round(rec["tree_chain_ms"] / rec["chain_ms"], 3)
        rec["chain_GBps"] = round(rec["bytes"] / rec["chain_ms"] / 1e6, 1)
        rec["tree_%s_GBps" % shape] = round(rec["bytes"] / rec["tree_%s_ms" % shape] / 1e6, 1)
        timing.emit(rec, results)
        del q, qs, qss
        torch.cuda.empty_cache()
    timing.write(results, args.out)


if __name__ == "__main__":
    main()

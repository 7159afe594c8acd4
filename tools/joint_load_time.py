#!/usr/bin/env python
"""Time the joint-wrench kernels and, in the same run on the same points and stream, what they are measured against:

  wrench_terms  batch.joint_wrench_terms_batch: w0, wa, wb of S sections in one launch   -- (3 d + 18 S) 8 bytes per point
  wrench        batch.joint_wrench_batch: one evaluation                                 -- (3 d + 6 S) 8 bytes per point
  callback      the batched-callback route: three single launches (q, 0, 0), (q, 0, qs), (q, qs, qss)
  torque_terms  the same robot's tree torque terms (tpr_tree_torque_terms_batch; a chain as the tree -1, 0, 1, ...): the same
                recursion up and down on the same per-link state, d outputs per evaluation -- (6 d) 8 bytes per point

    python tools/joint_load_time.py [--batch 65536] [--grid 200] [--out profiles/joint_load_time.json]

The models: a 7-dof chain with 2 sections, the 15-dof torso with two 7-dof arms (one fork) with 4, an 18-dof tree with one fork
(where the evaluations run one after another) with 4.  Protocol (that of tools/base_wrench_time.py): device tensors, inputs
resident, warm-up of every shape, then `--rounds` rounds in which the variants are timed in turn, each timing `--reps` calls
between two events on the stream; the figure is the median over the rounds and the spread their (max - min) / median.  Before
anything is timed the fused outputs are compared with the single entry bit for bit.  Prints one JSON line per model and writes
them to --out.  The yardstick is the torque-terms kernel: the new kernel does its recursion, drops 3 d stored doubles per point
and adds 18 S plus the frame changes, so
  fused_vs_torque     wrench_terms / torque_terms: at most (3 d + 18 S) / (6 d) where that exceeds 1, else 1, plus the two spreads
and, as for every fused kernel of the family,
  fused_vs_callback   wrench_terms / callback: at most 1 + the two spreads"""
import os
import sys

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toppra_amd import batch  # noqa: E402
from toppra_amd.chain import JointSections, KinematicTree  # noqa: E402


def models():
    """(name, model, its tree, sections) -- the test suite's random links (mixed joint types, tilted axes, rotated joint frames);
    the sections are bearings along joint axes (JointSections.on_axes)."""
    from tests import chain_ref, tree_cases, tree_ref
    chain = chain_ref.serial_chain(chain_ref.random_chain(7, 20240924 + 7, prismatic_every=4))
    torso = tree_ref.kinematic_tree(tree_ref.random_tree(tree_cases.SHAPES["torso"], 20240924 + 15, prismatic_every=4))
    y18 = tree_ref.kinematic_tree(tree_ref.random_tree(tree_cases.SHAPES["y18"], 20240924 + 18, prismatic_every=4))
    return [("chain7", chain, KinematicTree.from_chain(chain), JointSections.on_axes(chain, [1, -1], [0.05, 0.02])),
            ("torso15", torso, torso, JointSections.on_axes(torso, [1, 8, 7, 14], [0.05, 0.05, 0.02, 0.02])),
            ("y18", y18, y18, JointSections.on_axes(y18, [0, 5, 12, 17], 0.03))]


def main():
    import torch
    args = timing.parser(rounds=7, reps=5).parse_args()
    B, N = args.batch, args.grid
    dev = timing.device()
    results = []
    for name, robot, tree, sections in models():
        d, S = robot.dof, sections.count
        q, qs, qss = timing.inputs(dev, B, N, d)
        zero = torch.zeros_like(q)

        def callback():
            return tuple(batch.joint_wrench_batch(robot, *a, sections) for a in ((q, zero, zero), (q, zero, qs), (q, qs, qss)))
        runs = {"wrench_terms": lambda: batch.joint_wrench_terms_batch(robot, q, qs, qss, sections),
                "wrench": lambda: batch.joint_wrench_batch(robot, q, qs, qss, sections),
                "callback": callback,
                "torque_terms": lambda: batch.tree_torque_terms_batch(tree, q, qs, qss)}
        outs = timing.warm_up(runs)
        for k, what in enumerate(("w0", "wa", "wb")):
            assert torch.equal(outs["wrench_terms"][k], outs["callback"][k]), (name, "fused %s vs the single entry" % what)
        assert torch.equal(outs["wrench_terms"][2], outs["wrench"]) and bool(torch.isfinite(outs["wrench"]).all())
        del outs
        torch.cuda.empty_cache()
        ms = timing.measure(runs, args.rounds, args.reps)
        points = B * (N + 1)
        rec = dict({"model": name, "forks": len(getattr(robot, "forks", ())), "sections": S, "section_links": sections.on(robot).tolist()},
                   **timing.header(args, d))
        rec.update({"wrench_terms_bytes": points * (3 * d + 18 * S) * 8, "wrench_bytes": points * (3 * d + 6 * S) * 8,
                    "callback_bytes": 3 * points * (3 * d + 6 * S) * 8, "torque_terms_bytes": points * 6 * d * 8})
        timing.record(rec, ms, gbps=True)
        rec["wrench_terms_Mpoints_per_s"] = round(points / rec["wrench_terms_ms"] / 1e3, 1)
        rec["fused_vs_callback"] = round(rec["wrench_terms_ms"] / rec["callback_ms"], 3)
        rec["fused_vs_torque"] = round(rec["wrench_terms_ms"] / rec["torque_terms_ms"], 3)
        rec["bytes_vs_torque"] = round(rec["wrench_terms_bytes"] / rec["torque_terms_bytes"], 3)
        rec["not_slower_than_callback"] = bool(rec["fused_vs_callback"] <= 1.0 + rec["wrench_terms_spread"] + rec["callback_spread"])
        rec["within_the_added_bytes_of_torque_terms"] = bool(
            rec["fused_vs_torque"] <= max(1.0, rec["bytes_vs_torque"]) + rec["wrench_terms_spread"] + rec["torque_terms_spread"])
        timing.emit(rec, results)
        del q, qs, qss, zero
        torch.cuda.empty_cache()
    timing.write(results, args.out)


if __name__ == "__main__":
    main()

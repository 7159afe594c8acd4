#!/usr/bin/env python
"""Time the chain kernels against their alternatives, in one process, on the same points and stream:

  fused       batch.chain_torque_terms_batch: w0, wa, wb in one launch          -- rate on the algorithmic bytes 6 B (N+1) d 8
  singles     three batch.chain_inverse_dynamics_batch launches (what inv_dyn=chain.inverse_dynamics costs a constraint)
  torch       what a user had before: BatchJointTorqueConstraint.block() through a callback written as batched torch ops on the
              device -- the same recursion, below
  tool        batch.chain_tool_bound_batch: vSv and the bound                      -- rate on 2 B (N+1) d 8 + 24 B (N+1)

    python tools/chain_dynamics_time.py [--batch 65536] [--grid 200] [--dofs 7 12 20] [--out profiles/chain_dynamics_time.json]

Protocol (that of tools/stage_boxes_time.py): device tensors, warm-up of every shape, then `--rounds` rounds in which the
variants are timed in turn, each timing `--reps` calls between two events on the stream (the torch callback once per round: it
takes seconds); the figure is the median over the rounds and the spread their (max - min) / median.  The fused outputs are
compared with the singles bit for bit and with the torch recursion to rounding before anything is timed.  Prints one JSON line
per dof and writes them to --out."""
import os
import sys

import numpy as np

import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from toppra_amd import batch, constraint  # noqa: E402


def random_chain(d, seed):
    """The test suite's random chain (mixed joint types, tilted axes, rotated joint frames, full inertias) as a SerialChain."""
    from tests import chain_ref
    return chain_ref.serial_chain(chain_ref.random_chain(d, seed, prismatic_every=4))


def torch_inverse_dynamics(chain, device):
    """The recursion of csrc/tpr_chain_rnea.hip.inc as batched torch ops: inv_dyn(q, qd, qdd) on [B, N+1, d] device tensors."""
    import torch
    t = lambda x: torch.as_tensor(np.array(x), dtype=torch.float64, device=device)  # noqa: E731
    rot, trans, axis, com, mass = t(chain.rotations), t(chain.translations), t(chain.axes), t(chain.coms), chain.masses
    I = chain.inertias
    inertia = t(np.stack([np.array([[v[0], v[3], v[4]], [v[3], v[1], v[5]], [v[4], v[5], v[2]]]) for v in I]))
    prismatic = [ty == "prismatic" for ty in chain.joint_types]
    gravity, d = t(chain.gravity), chain.dof
    eye = torch.eye(3, dtype=torch.float64, device=device)
    skew = lambda k: t([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])  # noqa: E731
    K = [skew(chain.axes[i]) for i in range(d)]
    KK = [torch.outer(axis[i], axis[i]) for i in range(d)]
    cross = lambda a, b: torch.linalg.cross(a, b, dim=-1)  # noqa: E731

    def inv_dyn(q, qd, qdd):
        shape = q.shape
        q, qd, qdd = (v.reshape(-1, d) for v in (q, qd, qdd))
        P = q.shape[0]
        w = wd = q.new_zeros((P, 3))
        a = (-gravity).expand(P, 3)
        E, r, F, Nm = [], [], [], []
        for i in range(d):
            z = axis[i]
            if prismatic[i]:
                Ei = rot[i].expand(P, 3, 3)
                ri = trans[i] + (rot[i] @ z) * q[:, i:i + 1]
            else:
                s, c = torch.sin(q[:, i])[:, None, None], torch.cos(q[:, i])[:, None, None]
                Ei = rot[i] @ (c * eye + s * K[i] + (1 - c) * KK[i])
                ri = trans[i].expand(P, 3)
            Et = Ei.transpose(1, 2)
            ar = a + cross(wd, ri) + cross(w, cross(w, ri))
            a = (Et @ ar[:, :, None])[:, :, 0]
            wl = (Et @ w[:, :, None])[:, :, 0]
            wdl = (Et @ wd[:, :, None])[:, :, 0]
            if prismatic[i]:
                w, wd = wl, wdl
                a = a + z * qdd[:, i:i + 1] + cross(wl, z.expand(P, 3)) * (2 * qd[:, i:i + 1])
            else:
                w = wl + z * qd[:, i:i + 1]
                wd = wdl + z * qdd[:, i:i + 1] + cross(wl, z.expand(P, 3)) * qd[:, i:i + 1]
            ci = com[i].expand(P, 3)
            ac = a + cross(wd, ci) + cross(w, cross(w, ci))
            E.append(Ei); r.append(ri); F.append(ac * mass[i]); Nm.append(wd @ inertia[i] + cross(w, w @ inertia[i]))
        tau = q.new_empty((P, d))
        fc = nc = q.new_zeros((P, 3))
        for i in range(d - 1, -1, -1):
            f = F[i] + fc
            n = Nm[i] + cross(com[i].expand(P, 3), F[i]) + nc
            tau[:, i] = (f if prismatic[i] else n) @ axis[i]
            fc = (E[i] @ f[:, :, None])[:, :, 0]
            nc = (E[i] @ n[:, :, None])[:, :, 0] + cross(r[i], fc)
        return tau.reshape(shape)
    return inv_dyn


def main():
    import torch
    args = timing.parser(rounds=5, reps=3, dofs=(7, 12, 20)).parse_args()
    B, N = args.batch, args.grid
    dev = timing.device()
    results = []
    for d in args.dofs:
        chain = random_chain(d, 20240924 + d)
        q, qs, qss = timing.inputs(dev, B, N, d)
        zero = torch.zeros_like(q)
        taulim = np.tile([-1e3, 1e3], (d, 1))
        con = constraint.BatchJointTorqueConstraint(torch_inverse_dynamics(chain, dev), taulim, np.zeros(d))

        def fused():
            return batch.chain_torque_terms_batch(chain, q, qs, qss)

        def singles():
            return (batch.chain_inverse_dynamics_batch(chain, q, zero, zero), batch.chain_inverse_dynamics_batch(chain, q, zero, qs),
                    batch.chain_inverse_dynamics_batch(chain, q, qs, qss))

        def torch_block():
            blk = con.block(q, qs, qss)
            return blk["w0"], blk["wa"], blk["wb"]

        def tool():
            return batch.chain_tool_bound_batch(chain, q, qs, 0.25)

        runs = {"fused": fused, "singles": singles, "torch": (torch_block, 1), "tool": tool}  # (the torch callback once per round)
        outs = timing.warm_up(runs)
        for x, y in zip(outs["fused"], outs["singles"]):
            assert torch.equal(x, y), (d, "fused vs singles")
        worst = max(float(((x - y).abs().max() / y.abs().max())) for x, y in zip(outs["fused"], outs["torch"]))
        assert worst < 1e-9, (d, "fused vs the torch recursion", worst)
        del outs
        torch.cuda.empty_cache()
        ms = timing.measure(runs, args.rounds, args.reps)
        points = B * (N + 1)
        rec = timing.header(args, d)
        rec.update({"fused_bytes": 6 * points * d * 8, "tool_bytes": 2 * points * d * 8 + 24 * points, "fused_vs_torch_max_rel": worst})
        timing.record(rec, ms)
        rec["fused_GBps"] = round(rec["fused_bytes"] / rec["fused_ms"] / 1e6, 1)
        rec["fused_Mpoints_per_s"] = round(points / rec["fused_ms"] / 1e3, 1)
        rec["tool_GBps"] = round(rec["tool_bytes"] / rec["tool_ms"] / 1e6, 1)
        rec["singles_over_fused"] = round(rec["singles_ms"] / rec["fused_ms"], 3)
        rec["torch_over_fused"] = round(rec["torch_ms"] / rec["fused_ms"], 2)
        rec["fused_faster_than_singles"] = bool(rec["fused_ms"] * (1 + rec["fused_spread"]) < rec["singles_ms"] * (1 - rec["singles_spread"]))
        rec["fused_faster_than_torch"] = bool(rec["fused_ms"] * (1 + rec["fused_spread"]) < rec["torch_ms"] * (1 - rec["torch_spread"]))
        timing.emit(rec, results)
        del q, qs, qss, zero
        torch.cuda.empty_cache()
    timing.write(results, args.out)
    if not all(r["fused_faster_than_singles"] and r["fused_faster_than_torch"] for r in results):
        raise SystemExit("the fused kernel is not faster than its alternatives")


if __name__ == "__main__":
    main()

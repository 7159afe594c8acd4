"""Time the GPU row build of a torque-limited batch against its yardstick and the solve it feeds, on one MI355X:

    python tools/second_order_rows_time.py [--out profiles/second_order_rows.json] [--batch 65536]

65536 x 7 dof x 200 stages, velocity + joint torque limits under Interpolation (nC = 2 + 4 * 7 = 30 rows per stage), a
multiply / add only torch dynamics model.  Device events around each step, five repetitions after two warm-up calls:
path evaluation (tpr_path_eval_batch), the three model calls (torch, for scale), row assembly (tpr_second_order_rows_batch),
tpr_constraint_params_batch at the headline shape (velocity + acceleration limits under Interpolation: the same nC, the same
bytes written; a, b, c, low, high only) and the dense solve (tpr_solve_dense_batch) on the rows built here."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS, WARMUP = 5, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "second_order_rows.json"))
    ap.add_argument("--batch", type=int, default=65536)
    args = ap.parse_args()
    import torch
    from toppra_amd import _capi, batch
    from toppra_amd.algorithm import BatchTOPPRA
    from toppra_amd.constraint import BatchJointTorqueConstraint, DiscretizationType
    B, d, N = args.batch, 7, 200
    dev = torch.device("cuda", 0)
    data = batch.make_synthetic_batch(B, d, N)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    coef, breaks, grid, vlim, alim = (t(data[k]) for k in ("coef", "breaks", "grid", "vlim", "alim"))
    rng = np.random.default_rng(7)
    mass, grav, cori = (t(v)[:, None, :] for v in (1.0 + rng.random((B, d)), 0.5 * rng.standard_normal((B, d)), 0.3 * rng.standard_normal((B, d))))
    taumax, fric = 20.0 + 20.0 * rng.random((B, d)), t(0.1 * rng.random((B, d)))
    taulim = t(np.stack([-taumax, taumax], -1))
    model = lambda q, qd, qdd: mass * qdd + cori * q * (1.0 + qd * qd) + grav * q  # noqa: E731
    con = BatchJointTorqueConstraint(model, taulim, fric, discretization_scheme=DiscretizationType.Interpolation)
    inst = BatchTOPPRA(coef, breaks, grid, vlim, None, constraints=[con])

    def timed(fn):
        """[ms] of REPS calls, each between two events on the current stream, after WARMUP calls."""
        for _ in range(WARMUP):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms, out

    res = {}
    res["path_eval"], pe = timed(lambda: batch.path_eval_batch(coef, breaks, grid))
    res["inverse_dynamics_3_calls_torch"], blk = timed(lambda: con.block(pe["q"], pe["qs"], pe["qss"]))
    res["row_assembly"], rows = timed(lambda: batch.second_order_rows_batch(coef, breaks, grid, vlim, None, [blk]))
    nC = int(rows["a"].shape[2])
    assert nC == 30
    dense = tuple(rows[k] for k in ("a", "b", "c", "low", "high", "deltas"))
    res["dense_solve"], sol = timed(lambda: batch.solve_dense_batch(*dense))
    ok = int((sol["status"] == 0).sum())
    # the yardstick: params_tile_kernel at the headline shape, the same five outputs into the buffers just written
    p, keep = _capi.make_problem(coef, breaks, grid, vlim, alim, None, None, True)
    lib, stream = _capi.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    outs = [_capi.ptr(rows[k]) for k in ("a", "b", "c", "low", "high")]
    res["constraint_params_same_bytes"], _ = timed(lambda: _capi.check(lib.tpr_constraint_params_batch(C.byref(p), *outs, None, None, None, stream)))

    pts = B * (N + 1)
    written = pts * (3 * nC + 4) * 8 + B * N * 8
    table = int(coef.numel() + breaks.numel() + grid.numel()) * 8
    rec = {
        "device": torch.cuda.get_device_name(0), "shape": {"B": B, "dof": d, "N": N, "nC": nC, "constraints": "velocity + joint torque, Interpolation"},
        "reps": REPS, "warmup": WARMUP, "ms": res, "ok_trajectories": ok,
        "median_ms": {k: float(np.median(v)) for k, v in res.items()},
        "spread_ms": {k: float(max(v) - min(v)) for k, v in res.items()},
        "row_assembly_bytes": {"written_rows_boxes_deltas": written, "read_w_arrays": 3 * pts * d * 8, "read_spline_table_grid_limits": table + B * d * 3 * 8},
        "constraint_params_bytes": {"written_rows_boxes": pts * (3 * nC + 4) * 8, "read_spline_table_grid_limits": table + B * d * 4 * 8},
    }
    total_rows = sum(rec["row_assembly_bytes"].values())
    total_params = sum(rec["constraint_params_bytes"].values())
    rec["row_assembly_GBps"] = total_rows / np.median(res["row_assembly"]) / 1e6
    rec["constraint_params_GBps"] = total_params / np.median(res["constraint_params_same_bytes"]) / 1e6
    rec["path_eval_GBps"] = (3 * pts * d * 8 + table) / np.median(res["path_eval"]) / 1e6
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(rec["median_ms"]), "rows %.0f GB/s, params %.0f GB/s" % (rec["row_assembly_GBps"], rec["constraint_params_GBps"]))


if __name__ == "__main__":
    main()

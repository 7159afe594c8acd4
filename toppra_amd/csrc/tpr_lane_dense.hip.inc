// tpr_lane_dense.hip.inc -- the one-trajectory-per-lane kernel (family 1, tpr_lane.hip.inc) on dense rows.
// Included by tpr_kernels.hip only: a static kernel is emitted by every unit that sees it.

#pragma once
#include "tpr_dense_args.hpp"
namespace tpr {

// compute_reachable_sets (reachability_algorithm.py:378-431) on dense rows: lane_reachable_kernel (tpr_lane.hip.inc: one
// trajectory per lane, the reference's solve_stagewise_optim with its stateful warm start, the deltas[i - 1] quirk of
// _one_step_forward) with the stage rows copied from the arrays instead of generated.
static __global__ void __launch_bounds__(64) lane_dense_reachable_kernel(DenseArgs A, const double *sdmin, const double *sdmax,
                                                                  double *L, double *X) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= A.B) return;
    const int N = A.N, nC = A.nC;
    const double *ga = A.a + (size_t)b * (N + 1) * nC, *gb = A.b + (size_t)b * (N + 1) * nC, *gc = A.c + (size_t)b * (N + 1) * nC;
    const double *glow = A.low + (size_t)b * 2 * (N + 1), *ghigh = A.high + (size_t)b * 2 * (N + 1);
    const double *deltas = A.deltas + (size_t)b * N;
    StageRows R;
    WarmStart W = {{0, 0}, {0, 0}};
    if (A.active) { const int32_t *st = A.active + (size_t)b * 4; W.up[0] = st[0]; W.up[1] = st[1]; W.down[0] = st[2]; W.down[1] = st[3]; }
    auto put_state = [&]() {
        if (A.active) { int32_t *st = A.active + (size_t)b * 4; st[0] = W.up[0]; st[1] = W.up[1]; st[2] = W.down[0]; st[3] = W.down[1]; }
    };
    unsigned char order[kMaxRows];
    auto rows = [&](int i) {
        R.nC = nC;
        for (int r = 2; r < nC; ++r) { R.a[r] = ga[(size_t)i * nC + r]; R.b[r] = gb[(size_t)i * nC + r]; R.c[r] = gc[(size_t)i * nC + r]; }
        R.low0 = glow[2 * i]; R.high0 = ghigh[2 * i]; R.low1 = glow[2 * i + 1]; R.high1 = ghigh[2 * i + 1];
    };
    double *Xb = X + (size_t)b * 2 * (N + 1), *Lb = L + (size_t)b * 2 * (N + 1);
    for (int i = 0; i <= N; ++i) {  // feasible sets (:131-164), on the same wrapper object
        const bool last = i == N;
        rows(i);
        set_next_rows(R, last, last ? 0.0 : deltas[i], -kFeasMaxX, kFeasMaxX);
        double uu, lo, hi;
        stage_solve(R, W, 1e-9, 1.0, -kFeasMaxX, kFeasMaxX, 1, order, uu, lo);
        stage_solve(R, W, -1e-9, -1.0, -kFeasMaxX, kFeasMaxX, 1, order, uu, hi);
        if (lo < 0) lo = 0;
        Xb[2 * i] = lo; Xb[2 * i + 1] = hi;
    }
    for (int i = 0; i <= N; ++i) { Lb[2 * i] = 0.0; Lb[2 * i + 1] = 0.0; }
    double l0 = boundary_x(A.flags, sdmin[b]), l1 = boundary_x(A.flags, sdmax[b]);
    Lb[0] = l0; Lb[1] = l1;
    for (int i = 0; i < N; ++i) {
        const double delta = deltas[i];
        const double dprev = i > 0 ? deltas[i - 1] : deltas[N - 1];  // get_deltas()[i - 1]: Python's negative index at i = 0
        double lo, hi;
        if (isnan(l0) || isnan(l1)) { lo = qnan(); hi = qnan(); }
        else {
            rows(i);
            set_next_rows(R, false, delta, Xb[2 * (i + 1)], Xb[2 * (i + 1) + 1]);
            double uu, xx;
            stage_solve(R, W, -2 * dprev, -1.0, l0, l1, 1, order, uu, xx);
            hi = xx + 2 * dprev * uu;
            stage_solve(R, W, 2 * dprev, 1.0, l0, l1, 1, order, uu, xx);
            lo = xx + 2 * dprev * uu;
        }
        if (lo < 0) lo = 0;
        Lb[2 * (i + 1)] = lo; Lb[2 * (i + 1) + 1] = hi;
        if (isnan(lo) || isnan(hi)) break;
        l0 = lo; l1 = hi;
    }
    put_state();
}

}  // namespace tpr

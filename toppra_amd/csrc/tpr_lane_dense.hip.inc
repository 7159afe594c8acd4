// tpr_lane_dense.hip.inc -- the one-trajectory-per-lane kernel (family 1, tpr_lane.hip.inc) on dense rows.
// Included by tpr_kernels.hip only: a static kernel is emitted by every unit that sees it.

#pragma once
#include <type_traits>
#include "tpr_boxed_args.hpp"
namespace tpr {

// compute_reachable_sets (reachability_algorithm.py:378-431) on dense rows: lane_reachable_kernel (tpr_lane.hip.inc: one
// trajectory per lane, the reference's solve_stagewise_optim with its stateful warm start, the deltas[i - 1] quirk of
// _one_step_forward) with the stage rows copied from the arrays instead of generated.
// Args = DenseArgs: the rows of tpr_dense_problem; Args = SampledArgs: the rows second_order_rows_kernel (nblocks = 0) would
// write for the path samples, generated in place; Args = BoxedArgs: those rows without a velocity constraint, the variable
// box of a stage read from the arrays tpr_stage_boxes_batch writes.
template <class Args>
static __global__ void __launch_bounds__(64) lane_dense_reachable_kernel(Args A, const double *sdmin, const double *sdmax,
                                                                  double *L, double *X) {
    constexpr bool kBoxed = std::is_same<Args, BoxedArgs>::value;
    constexpr bool kSampled = std::is_same<Args, SampledArgs>::value || kBoxed;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= A.B) return;
    const int N = A.N, nC = A.nC;
    const size_t row0 = kSampled ? 0 : (size_t)b * (N + 1) * nC, box0 = kSampled && !kBoxed ? 0 : (size_t)b * 2 * (N + 1);  // (kSampled: no arrays)
    const double *ga = A.a + row0, *gb = A.b + row0, *gc = A.c + row0;
    const double *glow = A.low + box0, *ghigh = A.high + box0;
    const double *deltas = A.deltas + (kSampled ? 0 : (size_t)b * N);
    Traj T{};  // kSampled: the limits and the gridpoints of trajectory b
    const double *gqs = nullptr, *gqss = nullptr;
    if constexpr (kSampled) {
        T.d = A.d; T.N = N;
        T.has_vel = A.flags & TPR_HAS_VELOCITY; T.has_acc = A.flags & TPR_HAS_ACCELERATION; T.interp = A.flags & TPR_ACC_INTERPOLATION;
        T.grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)b * (N + 1) : 0);
        T.vlim = T.has_vel ? A.vlim + (size_t)b * 2 * A.d : nullptr;
        T.alim = T.has_acc ? A.alim + (size_t)b * 2 * A.d : nullptr;
        gqs = A.qs + (size_t)b * (N + 1) * A.d; gqss = A.qss + (size_t)b * (N + 1) * A.d;
    }
    auto step = [&](int i) { if constexpr (kSampled) return T.grid[i + 1] - T.grid[i]; else return deltas[i]; };
    StageRows R;
    WarmStart W = {{0, 0}, {0, 0}};
    if (A.active) { const int32_t *st = A.active + (size_t)b * 4; W.up[0] = st[0]; W.up[1] = st[1]; W.down[0] = st[2]; W.down[1] = st[3]; }
    auto put_state = [&]() {
        if (A.active) { int32_t *st = A.active + (size_t)b * 4; st[0] = W.up[0]; st[1] = W.up[1]; st[2] = W.down[0]; st[3] = W.down[1]; }
    };
    unsigned char order[kMaxRows];
    auto rows = [&](int i) {
        R.nC = nC;
        if constexpr (kSampled) {
            const int d = T.d;
            const bool nxt = i < N;  // (the last stage repeats itself)
            const double two_delta = nxt ? 2 * (T.grid[i + 1] - T.grid[i]) : 0.0;
            for (int r = 2; r < nC; ++r) {
                const int m = r - 2, blk = m / d, k = m - blk * d;
                const bool neg = blk & 1, nx = blk >= 2 && nxt;
                const double q1 = gqs[(size_t)(i + (nx ? 1 : 0)) * d + k], q2 = gqss[(size_t)(i + (nx ? 1 : 0)) * d + k];
                const double ra = nx ? q1 + two_delta * q2 : q1;
                R.a[r] = neg ? -ra : ra; R.b[r] = neg ? -q2 : q2; R.c[r] = neg ? T.alim[2 * k] : -T.alim[2 * k + 1];
            }
            R.low0 = kVarMin; R.high0 = kVarMax; R.low1 = kVarMin; R.high1 = kVarMax;
            if constexpr (kBoxed) {
                R.low0 = glow[2 * i]; R.high0 = ghigh[2 * i]; R.low1 = glow[2 * i + 1]; R.high1 = ghigh[2 * i + 1];
            } else if (T.has_vel) {
                double xlo, xhi;
                velocity_xbound(T, gqs + (size_t)i * d, xlo, xhi);
                R.low1 = R.low1 > xlo ? R.low1 : xlo;
                R.high1 = R.high1 < xhi ? R.high1 : xhi;
            }
        } else {
            for (int r = 2; r < nC; ++r) { R.a[r] = ga[(size_t)i * nC + r]; R.b[r] = gb[(size_t)i * nC + r]; R.c[r] = gc[(size_t)i * nC + r]; }
            R.low0 = glow[2 * i]; R.high0 = ghigh[2 * i]; R.low1 = glow[2 * i + 1]; R.high1 = ghigh[2 * i + 1];
        }
    };
    double *Xb = X + (size_t)b * 2 * (N + 1), *Lb = L + (size_t)b * 2 * (N + 1);
    for (int i = 0; i <= N; ++i) {  // feasible sets (:131-164), on the same wrapper object
        const bool last = i == N;
        rows(i);
        set_next_rows(R, last, last ? 0.0 : step(i), -kFeasMaxX, kFeasMaxX);
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
        const double delta = step(i);
        const double dprev = i > 0 ? step(i - 1) : step(N - 1);  // get_deltas()[i - 1]: Python's negative index at i = 0
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

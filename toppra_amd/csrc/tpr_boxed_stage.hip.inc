// tpr_boxed_stage.hip.inc -- the third stage source of the dense-row kernels (tpr_dense.hip.inc, included before this file):
// acceleration rows GENERATED from path samples as SampledStage generates them, the per-stage variable box READ from arrays
// as DenseStage reads it.  The box arrays are what tpr_stage_boxes_batch writes -- seidelWrapper's low_arr / high_arr for a
// list of first-order constraints (cy_seidel_solverwrapper.pyx:477-478, 512-520) -- so a stage costs four loads where
// SampledStage recomputes the velocity bound in every scan: no fp64 quotients, no fp32 group reductions, no loop with a
// run-time bound in front of the rows.  Results are the bits of the dense pass on the rows tpr_sampled_rows_batch writes
// (without a velocity constraint) with these boxes as low / high.
// Included by tpr_boxed_tu.hip.
#pragma once
#include "tpr_boxed_args.hpp"

namespace tpr {

template <int D, int L>
struct BoxedSampledStage {
    using C = GroupCfg<D, L>;
    using Args = BoxedArgs;
    int dof[C::S];      // dof of an acceleration row, -1 otherwise
    bool neg[C::S];     // row is the negated half of its +- pair
    bool nextpt[C::S];  // row is evaluated at s_{i+1} (the Interpolation block)
    double climit[C::S];
    const double *qs, *qss, *grid, *low, *high;
    int d;
    double *rowbuf;
    __device__ inline void init(const BoxedArgs &A, int bb, int gl, double *rb) {
        d = A.d;
        const int N = A.N;
        qs = A.qs + (size_t)bb * (N + 1) * d; qss = A.qss + (size_t)bb * (N + 1) * d;
        grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)bb * (N + 1) : 0);
        low = A.low + (size_t)bb * 2 * (N + 1); high = A.high + (size_t)bb * 2 * (N + 1);
        const double *alim = (A.flags & TPR_HAS_ACCELERATION) ? A.alim + (size_t)bb * 2 * d : nullptr;
        const int nacc = A.nC - 2;  // (4 | 2 | 0) d
        rowbuf = rb;
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
            const int m = s * L + gl - 6;
            const bool acc = m >= 0 && m < nacc;
            const int blk = acc ? m / d : 0;
            dof[s] = acc ? m - blk * d : -1;
            neg[s] = blk & 1;
            nextpt[s] = blk >> 1;
            climit[s] = acc ? ((blk & 1) ? alim[2 * dof[s]] : -alim[2 * dof[s] + 1]) : 0.0;
        }
    }
    __device__ inline double delta(int i) const { return grid[i + 1] - grid[i]; }
    template <bool MIRROR>
    __device__ inline void build(Slots<D, L> &R, int gl, int i, double delta, double n0, double n1, double &low0,
                                 double &high0, double &low1, double &high1, bool last, double xcap) const {
        const double *q1i = qs + (size_t)i * d, *q2i = qss + (size_t)i * d;
        low0 = low[2 * i]; high0 = high[2 * i];
        low1 = low[2 * i + 1]; high1 = high[2 * i + 1];
        // (feasible sets: x_min / x_max of solve_stagewise_optim intersect the box, cy_seidel_solverwrapper.pyx:598-601)
        low1 = low1 > -xcap ? low1 : -xcap;
        high1 = high1 < xcap ? high1 : xcap;
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
            const int vi = s * L + gl;
            double ra = 0, rb = 0, rc = -1;
            if (s == 0) {  // the box rows and the x_next pair live in slot 0 (L >= 8)
                const double ta[6] = {-1.0, 1.0, 0.0, 0.0, last ? 0.0 : -2 * delta, last ? 0.0 : 2 * delta};
                const double tb[6] = {0.0, 0.0, -1.0, 1.0, last ? 0.0 : -1.0, last ? 0.0 : 1.0};
                const double tc[6] = {low0, -high0, low1, -high1, last ? -1.0 : n0, last ? -1.0 : -n1};
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const bool hit = vi == j;
                    ra = hit ? ta[j] : ra;
                    rb = hit ? tb[j] : rb;
                    rc = hit ? tc[j] : rc;
                }
            }
            {
                const bool acc = dof[s] >= 0;
                const bool nx = nextpt[s] & !last;  // (the last stage repeats itself: linear_constraint.py:172,177)
                const int at = (acc ? dof[s] : 0) + (nx ? d : 0);
                const double q1 = q1i[at], q2 = q2i[at];
                const double av = nx ? q1 + (2 * delta) * q2 : q1;
                ra = acc ? (neg[s] ? -av : av) : ra;
                rb = acc ? (neg[s] ? -q2 : q2) : rb;
                rc = acc ? climit[s] : rc;
            }
            R.a[s] = ra; R.b[s] = rb; R.c[s] = rc;
            if (MIRROR && vi < C::nV) {
                rowbuf[vi] = ra; rowbuf[C::nV + vi] = rb; rowbuf[2 * C::nV + vi] = rc;
            }
        }
        if (MIRROR) {  // rows are read back by other lanes of the wave: stores before, loads after, in the memory model too
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
};

}  // namespace tpr

// tpr_boxes.hip.inc -- the per-stage variable boxes of seidelWrapper, built on the GPU from an ordered list of bound sources.
//
// The reference folds every constraint's ubound / xbound into low_arr / high_arr [N+1][2] in its constructor
// (solverwrapper/cy_seidel_solverwrapper.pyx:477-478, 512-520): the boxes start at VAR_MIN / VAR_MAX = -+1e8 and constraint j
// tightens them, in list order, with dbl_max(a, b) = a > b ? a : b and dbl_min(a, b) = a < b ? a : b, the running value being
// a -- the spelling decides which zero survives a tie of +0.0 and -0.0.  The xbound of JointVelocityConstraint and of
// JointVelocityConstraintVarying comes from _create_velocity_constraint(_varying) (toppra/_CythonUtils.pyx:16-100,
// constraint/linear_joint_velocity.py:43-53, 76-87): fp64 quotients limit / q', running bounds that are C floats (every
// assignment rounds to fp32, start -+1e8f), the upper bound squared in fp32, max(sdmin, 0)^2 in fp64, joints with q' == 0
// skipped -- velocity_xbound's expressions (tpr_device.hpp).  A running fp32 minimum of values rounded on assignment is the
// minimum of the rounded values in any order (rounding is monotonic; a NaN quotient loses every comparison), which is what
// SampledStage's group reduction relies on too.
//
// Work layout.  The gridpoints of the whole batch are one flat run of B (N+1): q' [.][d], a grid source [.][d][2] and the outputs
// [.][2] are contiguous across trajectory boundaries, so a block of 256 threads takes `tile` (256 where the LDS allows)
// CONSECUTIVE gridpoints wherever they fall.  Per VLIM* source, pass 1 walks the tile's (gridpoint, joint) pairs with
// consecutive threads on consecutive pairs: a wave's loads are 512 B of q' and 1 KB of limits, whole cache lines, and the two
// fp64 divisions of a pair -- the arithmetic of this kernel -- spread over all 256 threads instead of d of them per gridpoint;
// the fp32-rounded candidates go to LDS (pitch d | 1: the reads of pass 2, one gridpoint per thread, hit distinct banks).
// Pass 2: thread t reduces gridpoint t's d candidates, squares, and folds the result into the box it keeps in four registers
// across the source list; X / U sources are one 16-byte load per thread, adjacent threads adjacent pairs (two 8-byte loads from an
// array that is not 16-byte aligned).  The boxes leave as 16 bytes per thread and array,
// 4 KB contiguous per block.
// Rejected: one thread per gridpoint reading its own d (or 2 d) doubles -- lanes 8 d (16 d) bytes apart, every load
// instruction touching 64 cache lines, d sequential divisions per thread; and rows_tile's geometry (a block per trajectory
// and tile of <= 32 gridpoints) whose box pass keeps 32 of 256 threads busy.
#pragma once
#include "tpr_device.hpp"
#include "tpr_boxed_args.hpp"

namespace tpr {

constexpr int kBoxesTile = 256;  // gridpoints per block, at most (= threads per block)

static __global__ void __launch_bounds__(256) stage_boxes_kernel(BoxesArgs A) {
    extern __shared__ float boxes_lds[];  // sdmax candidates [tile][dp], then sdmin candidates [tile][dp]
    const int tid = threadIdx.x, n1 = A.N + 1, d = A.d, dp = A.dp, tile = A.tile;
    const long long total = (long long)A.B * n1;
    const long long g0 = (long long)blockIdx.x * tile;  // first gridpoint of the tile in the flat [B (N+1)] run
    const int npts = total - g0 < tile ? (int)(total - g0) : tile;
    const bool mine = tid < npts;
    const long long g = g0 + (mine ? tid : 0);
    const int gi = (int)g % n1;  // gridpoint of this thread's box within its trajectory (B (N+1) < 2^31: checked by the entry)
    float *cmax = boxes_lds, *cmin = boxes_lds + (size_t)tile * dp;
    double low0 = kVarMin, high0 = kVarMax, low1 = kVarMin, high1 = kVarMax;
    for (int j = 0; j < A.nsrc; ++j) {  // (the source index is the same for every lane: descriptors stay in scalar registers)
        const BoxSource S = A.src[j];
        const bool shared = S.flags & TPR_BOUND_SHARED;
        // (lower, upper) pairs are fetched as 16 bytes where the caller's array is 16-byte aligned (a view into a larger
        // tensor may start on an odd double): the same for every lane
        const bool pairs16 = (reinterpret_cast<uintptr_t>(S.data) & 15) == 0;
        if (S.kind == TPR_BOUND_X || S.kind == TPR_BOUND_U) {
            if (mine) {
                const double *v = S.data + 2 * (size_t)(shared ? gi : g);
                double lo, hi;
                if (pairs16) { const double2 w = *reinterpret_cast<const double2 *>(v); lo = w.x; hi = w.y; }
                else { lo = v[0]; hi = v[1]; }
                if (S.kind == TPR_BOUND_U) {
                    low0 = low0 > lo ? low0 : lo;
                    high0 = high0 < hi ? high0 : hi;
                } else {
                    low1 = low1 > lo ? low1 : lo;
                    high1 = high1 < hi ? high1 : hi;
                }
            }
            continue;
        }
        const bool per_point = S.kind == TPR_BOUND_VLIM_GRID;
        __syncthreads();  // the candidates of an earlier VLIM* source have been read
        for (int idx = tid; idx < npts * d; idx += blockDim.x) {
            const int pp = idx / d, k = idx - pp * d;
            const double q1 = A.qs[(size_t)g0 * d + idx];
            size_t at;
            if (per_point && !shared) at = (size_t)g0 * d + idx;
            else {
                const int gp = (int)g0 + pp, b = gp / n1, i = gp - b * n1;
                at = per_point ? (size_t)i * d + k : (shared ? (size_t)k : (size_t)b * d + k);
            }
            double vlo, vhi;
            if (pairs16) {  // one 16-byte load per (lower, upper) pair: a wave's loads use every byte of the lines they touch
                const double2 v = *reinterpret_cast<const double2 *>(S.data + 2 * at);
                vlo = v.x; vhi = v.y;
            } else { vlo = S.data[2 * at]; vhi = S.data[2 * at + 1]; }
            const double rmax = (q1 > 0 ? vhi : vlo) / q1, rmin = (q1 > 0 ? vlo : vhi) / q1;
            float sdmin = -kJvelMaxSd, sdmax = kJvelMaxSd;
            if (q1 > 0 || q1 < 0) {
                sdmax = (float)(rmax <= (double)sdmax ? rmax : (double)sdmax);
                sdmin = (float)(rmin >= (double)sdmin ? rmin : (double)sdmin);
            }
            cmax[pp * dp + k] = sdmax;
            cmin[pp * dp + k] = sdmin;
        }
        __syncthreads();
        if (mine) {
            float sdmin = -kJvelMaxSd, sdmax = kJvelMaxSd;
            for (int k = 0; k < d; ++k) {
                const float hi = cmax[tid * dp + k], lo = cmin[tid * dp + k];
                sdmax = hi <= sdmax ? hi : sdmax;
                sdmin = lo >= sdmin ? lo : sdmin;
            }
            const float up = sdmax * sdmax;
            const double lo = (double)sdmin >= 0.0 ? (double)sdmin : 0.0;
            const double xlo = lo * lo, xhi = (double)up;
            low1 = low1 > xlo ? low1 : xlo;
            high1 = high1 < xhi ? high1 : xhi;
        }
    }
    if (mine) {
        A.low[2 * (size_t)g] = low0; A.low[2 * (size_t)g + 1] = low1;
        A.high[2 * (size_t)g] = high0; A.high[2 * (size_t)g + 1] = high1;
    }
}

}  // namespace tpr

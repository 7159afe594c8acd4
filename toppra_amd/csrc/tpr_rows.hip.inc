// tpr_rows.hip.inc -- the dense rows of seidelWrapper for lists with second-order / torque constraints, built on the GPU.
//
// The reference builds them on the host, one gridpoint at a time: SecondOrderConstraint.compute_constraint_params
// (constraint/linear_second_order.py:142-173) and JointTorqueConstraint.compute_constraint_params (constraint/joint_torque.py)
// evaluate the user's inverse dynamics three times per gridpoint and substitute, canonical_to_interpolate
// (constraint/linear_constraint.py:84-192) turns Collocation parameters into the first-order Interpolation form, and
// seidelWrapper.__init__ (solverwrapper/cy_seidel_solverwrapper.pyx:455-520) flattens F a, F b, F c - g of every constraint
// into a_arr, b_arr, c_arr [N+1][nC] and the variable boxes low_arr, high_arr.  Here the three inverse-dynamics evaluations
// arrive as arrays (a batched model evaluates them in three calls for the whole batch), and one kernel writes the complete
// dense problem of tpr_dense_problem for B trajectories.
//
// Arithmetic (-ffp-contract=off: every operation is rounded on its own), per second-order block of width p:
//   a = wa - w0,  b = wb - w0,  c = w0 + friction * sign(q')                       (linear_second_order.py:154-162)
//   Interpolation: stage i holds [a_i | a_{i+1} + (2 delta_i) b_{i+1}], [b_i | b_{i+1}], [c_i | c_{i+1}] against
//   blkdiag(F_i, F_{i+1}), [g_i | g_{i+1}]; the last stage repeats itself           (linear_constraint.py:160-190)
//   signed identity F = [I; -I], g = [tau_max; -tau_min]: rows [v, -v], c rows c - g_k, -c - g_{p+k}
//   dense F [m][p]: row r = ((F_r0 x_0 + F_r1 x_1) + F_r2 x_2) + ... in index order k = 0 .. p-1, then minus g_r for c.
//   (The reference's F.dot(x) leaves order and fusion to the host's BLAS; rows of F with a single +-1 entry give the same
//   bits in any order.)
// Column layout: rows 0, 1 zero (the x_next pair), the acceleration block [q', -q' (| q'_next + 2 delta q''_next, -...)] as
// tpr_constraint_params_batch writes it, then one block per second-order constraint in list order.
//
// Work layout (that of params_tile_kernel): a block takes up to kRowsTile gridpoints of ONE trajectory.  Phase 1 puts q', q''
// of the tile + one more gridpoint into LDS, phase 2 the a | b | c of every second-order block (coalesced reads of the three
// w arrays), phase 3 writes the rows: a thread owns a column of the stage for good (its block and joint are divided out
// once) and walks the tile's gridpoints, so consecutive threads store consecutive addresses -- 256 / nC whole stages, up to
// 2 KB contiguous, per store instruction.
#pragma once
#include <type_traits>
#include "tpr_device.hpp"
#include "tpr_rows_args.hpp"

namespace tpr {

constexpr int kRowsTile = 32;  // at most; the launcher shrinks it until the LDS record fits

__device__ __forceinline__ Traj rows_traj(const RowsArgs &A, int b) {
    Traj T;
    T.d = A.d; T.nseg = A.nseg; T.N = A.N;
    T.has_vel = A.flags & TPR_HAS_VELOCITY;
    T.has_acc = A.flags & TPR_HAS_ACCELERATION;
    T.interp = A.flags & TPR_ACC_INTERPOLATION;
    T.coef = A.coef + (size_t)b * 4 * A.nseg * A.d;
    T.breaks = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? (size_t)b * (A.nseg + 1) : 0);
    T.grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)b * (A.N + 1) : 0);
    T.vlim = A.vlim ? A.vlim + (size_t)b * 2 * A.d : nullptr;
    T.alim = A.alim ? A.alim + (size_t)b * 2 * A.d : nullptr;
    return T;
}

// np.sign
__device__ __forceinline__ double sign_of(double v) { return v > 0 ? 1.0 : (v < 0 ? -1.0 : (v == 0 ? 0.0 : v)); }

// The body of the row kernels.  Args = RowsArgs: q', q'' from the spline table (second_order_rows_kernel); Args = SampledRowsArgs:
// q', q'' are the caller's samples of any geometric path, which phase 1 copies (sampled_rows_kernel) -- everything after phase 1
// is shared.
template <class Args>
__device__ __forceinline__ void
rows_tile(const Args &A, int tile, int cap, double *a, double *b, double *c, double *low, double *high, double *deltas) {
    // q1 [(cap + 1) d], q2 [(cap + 1) d], delta [cap], alim [2 d], w [(cap + 1) wsum]; cap = the tile the LDS was sized for
    extern __shared__ double rows_lds[];
    const int bt = blockIdx.x, tid = threadIdx.x;
    const Traj T = rows_traj(A, bt);
    const int N = A.N, d = A.d, nC = A.nC, wsum = A.wsum;
    const int i0 = blockIdx.y * tile;
    const int npts = N + 1 - i0 < tile ? N + 1 - i0 : tile;
    double *q1s = rows_lds, *q2s = q1s + (cap + 1) * d, *dl = q2s + (cap + 1) * d, *al = dl + cap, *ws = al + 2 * d;
    constexpr bool kSampled = std::is_same<Args, SampledRowsArgs>::value;
    // phase 1: q', q'' (tpr_device.hpp::cubic_d1_d2, the expressions of params_tile_kernel)
    for (int idx = tid; idx < (npts + 1) * d; idx += blockDim.x) {
        const int pp = idx / d, k = idx - pp * d, i = i0 + pp;
        if constexpr (kSampled) {
            if (i <= N) {
                const size_t at = ((size_t)bt * (N + 1) + i0) * d + idx;
                q1s[idx] = A.qs[at]; q2s[idx] = A.qss[at];
            }
        } else if (i <= N) {
            const double s = T.grid[i];
            const int j = find_segment(T.breaks, T.nseg, s);
            const double t = s - T.breaks[j];
            double q1, q2;
            cubic_d1_d2(T.coef[(size_t)(0 * T.nseg + j) * d + k], T.coef[(size_t)(1 * T.nseg + j) * d + k],
                        T.coef[(size_t)(2 * T.nseg + j) * d + k], t, q1, q2);
            q1s[idx] = q1; q2s[idx] = q2;
        }
    }
    if (tid < npts) dl[tid] = i0 + tid < N ? T.grid[i0 + tid + 1] - T.grid[i0 + tid] : 0.0;
    if (T.has_acc && tid < 2 * d) al[tid] = T.alim[tid];
    __syncthreads();
    const size_t pt0 = (size_t)bt * (N + 1) + i0;  // first gridpoint of the tile in the [B][N+1] arrays
    // phase 2: a | b | c of every second-order block at the tile's gridpoints + one more
    for (int j = 0; j < A.nblocks; ++j) {
        const RowsBlock &K = A.blk[j];
        const int p = K.p;
        const double *fr = K.friction ? K.friction + (size_t)bt * p : nullptr;
        for (int idx = tid; idx < (npts + 1) * p; idx += blockDim.x) {
            const int pp = idx / p, k = idx - pp * p;
            if (i0 + pp <= N) {
                const size_t at = pt0 * p + idx;
                const double w0 = K.w0[at];
                double *rec = ws + pp * wsum + K.lds0;
                rec[k] = K.wa[at] - w0;
                rec[p + k] = K.wb[at] - w0;
                rec[2 * p + k] = fr ? w0 + fr[k] * sign_of(q1s[pp * d + k]) : w0;  // (friction: p == d, checked by the entry)
            }
        }
    }
    __syncthreads();
    // phase 3: rows.  ppp gridpoints per pass, thread = (gridpoint within the pass, column)
    const int ppp = blockDim.x / nC;  // (nC <= 122 < blockDim.x: checked by the entry)
    const int psub = tid / nC, r = tid - psub * nC;
    if (psub < ppp) {
        const int acc_rows = T.has_acc ? (T.interp ? 4 : 2) * d : 0;
        // rows 0, 1 (the x_next pair, filled in per solve: zeros here) travel with the columns next to them, so that a wave
        // whose lanes straddle a stage's first columns still runs ONE loop of stores
        if (acc_rows > 0 && r < 2 + acc_rows) {
            const int m = r - 2, blk = r >= 2 ? m / d : 0, k = r >= 2 ? m - blk * d : 0;
            const bool neg = blk & 1;
            const double cc = r >= 2 ? (neg ? al[2 * k] : -al[2 * k + 1]) : 0.0;
            for (int pp = psub; pp < npts; pp += ppp) {
                double va = 0.0, vb = 0.0;
                if (r >= 2) {
                    const bool nxt = blk >= 2 && i0 + pp < N;
                    const double q1 = q1s[(pp + (nxt ? 1 : 0)) * d + k], q2 = q2s[(pp + (nxt ? 1 : 0)) * d + k];
                    const double ra = nxt ? q1 + (2 * dl[pp]) * q2 : q1;
                    va = neg ? -ra : ra;
                    vb = neg ? -q2 : q2;
                }
                const size_t at = (pt0 + pp) * nC + r;
                a[at] = va; b[at] = vb; c[at] = cc;
            }
        }
        // (the block index is the same for every lane: the descriptors stay in scalar registers)
        for (int j = 0; j < A.nblocks; ++j) {
            const RowsBlock &K = A.blk[j];
            const int p = K.p, m = K.m;
            const bool zero = j == 0 && acc_rows == 0 && r < 2;
            if (!zero && (r < K.col0 || r >= K.col0 + ((K.flags & TPR_SO_INTERPOLATION) ? 2 : 1) * m)) continue;
            const int rr = zero ? 0 : r - K.col0, half = rr >= m ? 1 : 0, row = rr - half * m;
            const double *rec0 = ws + K.lds0;
            const double *g0 = K.g + ((K.flags & TPR_SO_G_PER_TRAJ) ? (size_t)bt * m : 0) + row;
            const bool g_pt = K.flags & TPR_SO_G_PER_POINT;
            if (!(K.flags & (TPR_SO_F_SHARED | TPR_SO_F_PER_TRAJ | TPR_SO_F_PER_POINT))) {  // the signed identity
                const bool neg = row >= p;
                const int k = neg ? row - p : row;
                const double gk = g_pt ? 0.0 : *g0;
                for (int pp = psub; pp < npts; pp += ppp) {
                    const bool nxt = half && i0 + pp < N;  // (the last stage repeats itself)
                    const double *rec = rec0 + (pp + (nxt ? 1 : 0)) * wsum;
                    const double va0 = rec[k], vb0 = rec[p + k], vc0 = rec[2 * p + k];
                    const double ra = nxt ? va0 + (2 * dl[pp]) * vb0 : va0;
                    const double gg = g_pt ? g0[((size_t)bt * (N + 1) + i0 + pp + (nxt ? 1 : 0)) * m] : gk;
                    const size_t at = (pt0 + pp) * nC + r;
                    a[at] = zero ? 0.0 : (neg ? -ra : ra);
                    b[at] = zero ? 0.0 : (neg ? -vb0 : vb0);
                    c[at] = zero ? 0.0 : (neg ? -vc0 : vc0) - gg;
                }
            } else {  // dense F: every row the sum over k in index order
                const double *F0 = K.F + ((K.flags & TPR_SO_F_PER_TRAJ) ? (size_t)bt * m * p : 0) + (size_t)row * p;
                const bool f_pt = K.flags & TPR_SO_F_PER_POINT;
                for (int pp = psub; pp < npts; pp += ppp) {
                    const bool nxt = half && i0 + pp < N;
                    const double *rec = rec0 + (pp + (nxt ? 1 : 0)) * wsum;
                    const double two_delta = 2 * dl[pp];
                    const size_t gpt = (size_t)bt * (N + 1) + i0 + pp + (nxt ? 1 : 0);
                    const double *Fr = f_pt ? F0 + gpt * m * p : F0;
                    double va = 0.0, vb = 0.0, vc = 0.0;
                    for (int k = 0; k < p; ++k) {
                        const double f = Fr[k];
                        const double ra = nxt ? rec[k] + two_delta * rec[p + k] : rec[k];
                        const double ta = f * ra, tb = f * rec[p + k], tc = f * rec[2 * p + k];
                        va = k ? va + ta : ta; vb = k ? vb + tb : tb; vc = k ? vc + tc : tc;
                    }
                    vc = vc - (g_pt ? g0[gpt * m] : *g0);
                    const size_t at = (pt0 + pp) * nC + r;
                    a[at] = zero ? 0.0 : va; b[at] = zero ? 0.0 : vb; c[at] = zero ? 0.0 : vc;
                }
            }
        }
        if (A.nblocks == 0 && acc_rows == 0 && r < 2)
            for (int pp = psub; pp < npts; pp += ppp) { const size_t at = (pt0 + pp) * nC + r; a[at] = 0.0; b[at] = 0.0; c[at] = 0.0; }
    }
    if (tid < npts) {
        double xlo, xhi, low1 = kVarMin, high1 = kVarMax;
        if (T.has_vel) {
            velocity_xbound(T, q1s + tid * d, xlo, xhi);
            low1 = low1 > xlo ? low1 : xlo;
            high1 = high1 < xhi ? high1 : xhi;
        }
        const size_t g = pt0 + tid;
        low[2 * g] = kVarMin; low[2 * g + 1] = low1;
        high[2 * g] = kVarMax; high[2 * g + 1] = high1;
        if constexpr (kSampled) {
            // the constraint's own bound (None without a velocity constraint: the box is written in its place)
            if (A.xbound) { A.xbound[2 * g] = T.has_vel ? xlo : kVarMin; A.xbound[2 * g + 1] = T.has_vel ? xhi : kVarMax; }
        }
        if (deltas && i0 + tid < N) deltas[(size_t)bt * N + i0 + tid] = dl[tid];
    }
}

static __global__ void __launch_bounds__(256)
second_order_rows_kernel(RowsArgs A, int tile, int cap, double *a, double *b, double *c, double *low, double *high, double *deltas) {
    rows_tile(A, tile, cap, a, b, c, low, high, deltas);
}
// ... for a path given as samples at the gridpoints (tpr_sampled_rows_batch)
static __global__ void __launch_bounds__(256)
sampled_rows_kernel(SampledRowsArgs A, int tile, int cap, double *a, double *b, double *c, double *low, double *high, double *deltas) {
    rows_tile(A, tile, cap, a, b, c, low, high, deltas);
}

// SplineInterpolator.__call__(grid, order) for order 0, 1, 2 (interpolator.py:423-430): q in scipy PPoly's evaluation order
// (ppoly_eval_kernel's order-0 expression), q' and q'' from the differentiated coefficient tables (cubic_d1_d2), one thread per
// (gridpoint, joint).
static __global__ void __launch_bounds__(256) path_eval_kernel(PathEvalArgs A) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int d = A.d, nseg = A.nseg, n1 = A.N + 1;
    if (gid >= (long long)A.B * n1 * d) return;
    const long long pt = gid / d;
    const int k = (int)(gid - pt * d), b = (int)(pt / n1), i = (int)(pt - (long long)b * n1);
    const double *coef = A.coef + (size_t)b * 4 * nseg * d;
    const double *breaks = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? (size_t)b * (nseg + 1) : 0);
    const double s = A.grid[((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)b * n1 : 0) + i];
    const int j = find_segment(breaks, nseg, s);
    const double x = s - breaks[j];
    const double c0 = coef[(size_t)(0 * nseg + j) * d + k], c1 = coef[(size_t)(1 * nseg + j) * d + k];
    const double c2 = coef[(size_t)(2 * nseg + j) * d + k], c3 = coef[(size_t)(3 * nseg + j) * d + k];
    double q1, q2;
    cubic_d1_d2(c0, c1, c2, x, q1, q2);
    if (A.q) A.q[gid] = ((c3 + c2 * x) + c1 * (x * x)) + c0 * ((x * x) * x);
    if (A.qs) A.qs[gid] = q1;
    if (A.qss) A.qss[gid] = q2;
}

}  // namespace tpr

// tpr_group.hip.inc -- kernel family 2: constraint rows across lanes (the fast path).
//
// A trajectory is owned by a group of L adjacent lanes (L = 4/8/16, 64/L trajectories per wave).
// The nC = 2+4D constraint rows of a stage LP plus the 4 box rows are dealt round-robin onto
// L x S register slots ("virtual row" vi -> lane vi % L, slot vi / L), so nothing is indexed
// dynamically and nothing lives in scratch.  Seidel's pivot becomes:
//   * violation test of all rows in parallel; the first violated row in the reference's order is
//     an integer min-reduction over (order position, row) keys (DPP butterflies inside the group),
//   * the pivot row is fetched from a small LDS mirror of the stage rows (one broadcast read),
//     every earlier row + the box rows are projected onto the pivot line in parallel (one
//     division per slot, slots no lane needs are skipped wave-uniformly),
//   * min/max DPP reductions solve the 1-D sub-LP; the active-set bookkeeping (ties resolved to the
//     smallest order position, exactly as the reference's strict comparisons do) is done once,
//     after the last pivot.
// Groups in one wave run different pivot counts; control flow is group-uniform, so the wave loops
// until its slowest group is done.  compute_constraint_params is fused: every slot re-evaluates
// the spline derivative it needs from the coefficient table staged in LDS.
//
// Reference map: as tpr_lane.hip.inc (same algorithm, same arithmetic, same results bit for bit).

// Margins of the certificates on row residuals: absolute (the solver's tolerances are 1e-10 and 1e-8)
// and relative (against the rounding of a residual evaluated at a vertex of condition <= 1 / kCertMinCross).
#ifndef TPR_SLACK_ABS
#define TPR_SLACK_ABS 1e-6
#endif
#ifndef TPR_SLACK_REL
#define TPR_SLACK_REL 1e-9
#endif
#ifndef TPR_GROUP_WAVES
#define TPR_GROUP_WAVES 3  // waves per SIMD the rows-across-lanes solve kernel is compiled for
#endif
#ifndef TPR_PREDICT_LOWER
#define TPR_PREDICT_LOWER 1
#endif
#ifndef TPR_PREDICT_UPPER
#define TPR_PREDICT_UPPER 1
#endif

#pragma once
#include <type_traits>
namespace tpr {

#define TPR_WALK_FAIL(code) return false

// ---- cross-lane helpers -------------------------------------------------------------------
constexpr int kDppXor1 = 0xB1;        // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;        // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141; // lane i <-> 7-i within 8
constexpr int kDppMirror = 0x140;     // lane i <-> 15-i within 16

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(dpp_i32<CTRL>(__float_as_int(v)));
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const int lo = dpp_i32<CTRL>(__double2loint(x));
    const int hi = dpp_i32<CTRL>(__double2hiint(x));
    return __hiloint2double(hi, lo);
}

// All-lanes (butterfly) reductions inside a group of L lanes.  OP(a, b) must be commutative.
#define TPR_GROUP_REDUCE(NAME, T, DPP, OP)                                   \
    template <int L>                                                         \
    __device__ __forceinline__ T NAME(T x) {                                 \
        if (L >= 2) { T y = DPP<kDppXor1>(x); x = OP(x, y); }                \
        if (L >= 4) { T y = DPP<kDppXor2>(x); x = OP(x, y); }                \
        if (L >= 8) { T y = DPP<kDppHalfMirror>(x); x = OP(x, y); }          \
        if (L >= 16) { T y = DPP<kDppMirror>(x); x = OP(x, y); }             \
        if (L >= 32) { T y = __shfl_xor(x, 16, 64); x = OP(x, y); }          \
        if (L >= 64) { T y = __shfl_xor(x, 32, 64); x = OP(x, y); }          \
        return x;                                                            \
    }
#define TPR_MIN(a, b) ((b) < (a) ? (b) : (a))
#define TPR_MAX(a, b) ((b) > (a) ? (b) : (a))
#define TPR_OR(a, b) ((a) | (b))
#define TPR_FMIN(a, b) __builtin_fmin(a, b)  // v_min_f64; operands are never NaN here
#define TPR_FMAX(a, b) __builtin_fmax(a, b)
TPR_GROUP_REDUCE(group_min_i32, int, dpp_i32, TPR_MIN)
TPR_GROUP_REDUCE(group_or_i32, int, dpp_i32, TPR_OR)
TPR_GROUP_REDUCE(group_min_f32, float, dpp_f32, TPR_MIN)
TPR_GROUP_REDUCE(group_max_f32, float, dpp_f32, TPR_MAX)
TPR_GROUP_REDUCE(group_min_f64, double, dpp_f64, TPR_FMIN)
TPR_GROUP_REDUCE(group_max_f64, double, dpp_f64, TPR_FMAX)

// ---- one trajectory group ------------------------------------------------------------------
constexpr int kBig = 0x3fffffff;

template <int D, int L>
struct GroupCfg {
    static constexpr int nC = 2 + 4 * D;          // structural rows (velocity is a box bound)
    static constexpr int nV = nC + 4;             // + box rows
    static constexpr int S = (nV + L - 1) / L;    // slots per lane
    static_assert(nV <= 128, "row keys carry the virtual row index in 7 bits");
    // LDS doubles per group: stage rows, then (when it fits) the spline table c0,c1,c2 per segment
    // and dof plus the breakpoints; paths with many segments read the table from global memory
    static constexpr int kRowBuf = 3 * nV;
    __host__ __device__ static constexpr int lds_doubles(int nseg, bool table_in_lds) {
        return kRowBuf + (table_in_lds ? 3 * nseg * D + (nseg + 1) : 0);
    }
};

// ---- host side: launch geometry and dof dispatch, shared by every unit that launches these kernels -----------------
constexpr size_t kMaxDynamicLds = 64 * 1024;

// Block size for B trajectories on L lanes each: `threads`, halved while the batch would leave CUs idle (256 CUs; small
// batches such as BASELINE config 2's 4096 trajectories only make 128 blocks of 256 threads).
static inline int shrink_block_to_batch(int threads, int B, int L) {
    while (threads > 64 && (long long)B * L / threads < 4 * 256) threads /= 2;
    return threads;
}

// Launch geometry of a rows-across-lanes kernel.  The spline table is staged in LDS when a 64-thread block's worth fits
// in 64 KB (always for ordinary waypoint counts); otherwise it stays in global memory.  Block size: the largest of
// 256 / 128 / 64 threads that fits, then shrink_block_to_batch.
struct GroupLaunch {
    int threads;
    unsigned blocks;
    size_t lds;
    bool table_in_lds;
};
template <int D, int L>
static GroupLaunch group_launch_geometry(int B, int nseg) {
    auto lds_bytes = [&](int threads, bool table) {
        return (size_t)(threads / L) * GroupCfg<D, L>::lds_doubles(nseg, table) * sizeof(double);
    };
    GroupLaunch g{64, 0, 0, lds_bytes(64, true) <= kMaxDynamicLds};
    for (int t = 256; t > 64; t /= 2)
        if (lds_bytes(t, g.table_in_lds) <= kMaxDynamicLds) { g.threads = t; break; }
    g.threads = shrink_block_to_batch(g.threads, B, L);
    const int groups = g.threads / L;
    g.blocks = (B + groups - 1) / groups;
    g.lds = lds_bytes(g.threads, g.table_in_lds);
    return g;
}

// Runtime dof -> the compile-time <D, L> of these kernels: 8 lanes per trajectory up to 8 dof, 16 above.  Calls
// f(integral_constant<int, D>, integral_constant<int, L>) and returns its result; `none` for a dof outside LO..HI
// (a unit that holds only part of the range instantiates only that part).
template <int LO = 1, int HI = TPR_MAX_DOF_FAST, class F>
static int for_dof(int d, int none, F &&f) {
    switch (d) {
#define TPR_DOF_CASE(DD)                                                                                              \
    case DD:                                                                                                          \
        if constexpr (DD >= LO && DD <= HI) return f(std::integral_constant<int, DD>{}, std::integral_constant<int, (DD <= 8 ? 8 : 16)>{}); \
        break;
        TPR_DOF_CASE(1) TPR_DOF_CASE(2) TPR_DOF_CASE(3) TPR_DOF_CASE(4) TPR_DOF_CASE(5) TPR_DOF_CASE(6) TPR_DOF_CASE(7) TPR_DOF_CASE(8)
        TPR_DOF_CASE(9) TPR_DOF_CASE(10) TPR_DOF_CASE(11) TPR_DOF_CASE(12) TPR_DOF_CASE(13) TPR_DOF_CASE(14) TPR_DOF_CASE(15) TPR_DOF_CASE(16)
#undef TPR_DOF_CASE
    }
    return none;
}

// Per-lane register state of the LP rows.
template <int D, int L>
struct Slots {
    using C = GroupCfg<D, L>;
    double a[C::S], b[C::S], c[C::S];
};

struct GroupLp {
    bool ok;
    double u, x;
    int ac0, ac1;
};

// Virtual-row bookkeeping (compile-time per slot, runtime per lane).
//   vi 0..3  box rows  low0, high0, low1, high1     (reference ids -1..-4)
//   vi 4,5   rows 0,1  x_next pair
//   vi 6..   rows 2..  acceleration rows, m = vi-6 = blk*D + k
__device__ __forceinline__ int row_id_of(int vi) { return vi < 4 ? -1 - vi : vi - 4; }

// Seidel 2-D LP on the group's slots.  Identical decisions and arithmetic to tpr::lp2d
// (tpr_device.hpp).  `rowbuf` is the group's LDS mirror of the rows: a[nV], b[nV], c[nV].
template <int D, int L>
__device__ inline GroupLp group_lp2d(const Slots<D, L> &R, const double *rowbuf, int gl, double v0, double v1,
                                     double low0, double high0, double low1, double high1, int wac0,
                                     int wac1) {
    using C = GroupCfg<D, L>;
    GroupLp o;
    o.ok = false; o.u = qnan(); o.x = qnan(); o.ac0 = 0; o.ac1 = 0;
    const bool active = !(low0 > high0) && !(low1 > high1);
    double cu, cx;
    if (v0 > kTiny) { cu = high0; o.ac0 = -2; } else { cu = low0; o.ac0 = -1; }
    if (v1 > kTiny) { cx = high1; o.ac1 = -4; } else { cx = low1; o.ac1 = -3; }

    // order positions for this LP's warm start: [wac1, wac0, remaining rows ascending]
    const bool warm = wac0 >= 0 && wac0 < C::nC && wac1 >= 0 && wac1 < C::nC && wac0 != wac1;
    int pos[C::S];
#pragma unroll
    for (int s = 0; s < C::S; ++s) {
        const int vi = s * L + gl;
        const int r = vi - 4;  // structural row index
        int p = r;
        if (warm) p = r == wac1 ? 0 : (r == wac0 ? 1 : 2 + r - (r > wac0 ? 1 : 0) - (r > wac1 ? 1 : 0));
        if (vi < 4) p = -1;          // box rows are projected in every pass, never pivots
        if (vi >= C::nV) p = kBig;   // empty slot
        pos[s] = p;
    }

    int kpos = -1, pivot_vi = -1, want = 0;
    double T = 0;
    double ts[C::S];
    int cls[C::S];  // 0 = not a candidate, 1 = upper bound on t, 2 = lower bound on t
#pragma unroll
    for (int s = 0; s < C::S; ++s) { ts[s] = 0; cls[s] = 0; }
    bool success = false;
    while (active) {
        // first violated structural row after position kpos, in the reference's order
        int key = kBig;
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
            const double val = R.a[s] * cu + R.b[s] * cx + R.c[s];
            const bool viol = (pos[s] > kpos) & (pos[s] < kBig) & !(val < kTiny);
            const int cand = viol ? pos[s] * 128 + (s * L + gl) : kBig;
            key = cand < key ? cand : key;
        }
        key = group_min_i32<L>(key);
        if (key == kBig) { success = true; break; }
        const int k = key >> 7;
        pivot_vi = key & 127;
        const double pa = rowbuf[pivot_vi], pb = rowbuf[C::nV + pivot_vi], pc = rowbuf[2 * C::nV + pivot_vi];
        const double den = pa * pa + pb * pb;
        if (den == 0.0) break;  // the reference raises ZeroDivisionError
        const double zp0 = (-pa * pc) / den;
        const double zp1 = (-pb * pc) / den;
        const double dt0 = -pb, dt1 = pa;
        const double v1d = dt0 * v0 + dt1 * v1;

        // project rows at positions < k and the box rows; per-lane running min / max
        double tmax = kInf1d, tmin = -kInf1d;
        int par_bad = 0;
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
            const bool need = pos[s] < k;  // box rows have pos -1
            cls[s] = 0;
            if (__builtin_amdgcn_ballot_w64(need) == 0) continue;  // wave-uniform skip
            const double denom = dt0 * R.a[s] + dt1 * R.b[s];
            const double num = R.c[s] + zp1 * R.b[s] + zp0 * R.a[s];
            const double t = -num / denom;
            const bool up = need & (denom > kTiny);
            const bool lo = need & (denom < -kTiny);
            ts[s] = t;
            cls[s] = up ? 1 : (lo ? 2 : 0);
            tmax = (up & (t < tmax)) ? t : tmax;
            tmin = (lo & (t > tmin)) ? t : tmin;
            par_bad |= (need & !up & !lo & (num > kSmall)) ? 1 : 0;
        }
        const double gmax = group_min_f64<L>(tmax);
        const double gmin = group_max_f64<L>(tmin);
        par_bad = group_or_i32<L>(par_bad);
        if (par_bad || gmin > gmax) break;
        const bool pick_min = fabs(v1d) < kTiny || v1d < 0;
        T = pick_min ? gmin : gmax;
        want = pick_min ? 2 : 1;
        // the +-1e10 line bounds being active is "infeasible" in the reference (:366-383)
        if (pick_min ? !(T > -kInf1d) : !(T < kInf1d)) break;
        cu = zp0 + T * dt0;
        cx = zp1 + T * dt1;
        kpos = k;
    }
    if (success) {
        o.ok = true; o.u = cu; o.x = cx;
        if (pivot_vi >= 0) {
            // active set of the last pivot: the pivot row, and the row attaining T in its 1-D LP
            // (smallest order index among ties; box rows sort after every structural row)
            int akey = kBig;
#pragma unroll
            for (int s = 0; s < C::S; ++s) {
                const int vi = s * L + gl;
                const int j = vi < 4 ? C::nC + vi : pos[s];
                const int cand = (cls[s] == want && ts[s] == T) ? (j << 8) + (row_id_of(vi) & 0xff) : kBig;
                akey = cand < akey ? cand : akey;
            }
            akey = group_min_i32<L>(akey);
            o.ac0 = pivot_vi - 4;
            o.ac1 = (int)(signed char)(akey & 0xff);
        }
    }
    return o;
}

// Inclusive prefix minimum over the L lanes of a group, in lane order (DPP row shifts inside the row of 16; with 8 lanes
// per group a shift must not reach into the neighbouring group).
template <int L>
__device__ __forceinline__ double group_prefix_min_f64(double x, int gl) {
    static_assert(L == 8 || L == 16, "groups inside one DPP row");
    constexpr double kTop = 3.0e300;
    auto step = [&](double v, double shifted, int d) { return fmin(v, (L == 16 || gl >= d) ? shifted : kTop); };
    auto shr = [&](double v, int lo_, int hi_) { return __hiloint2double(hi_, lo_); };
    (void)shr;
#define TPR_SHR(V, CTRL) __hiloint2double(__builtin_amdgcn_update_dpp(__double2hiint(kTop), __double2hiint(V), CTRL, 0xf, 0xf, false), \
                                          __builtin_amdgcn_update_dpp(__double2loint(kTop), __double2loint(V), CTRL, 0xf, 0xf, false))
    x = step(x, TPR_SHR(x, 0x111), 1);
    x = step(x, TPR_SHR(x, 0x112), 2);
    x = step(x, TPR_SHR(x, 0x114), 4);
    if (L == 16) x = step(x, TPR_SHR(x, 0x118), 8);
    return x;
}
template <int L>
__device__ __forceinline__ double group_shift1_f64(double x, int gl) {  // lane gl reads lane gl - 1 of its group (+3e300 for lane 0)
    constexpr double kTop = 3.0e300;
    const double y = TPR_SHR(x, 0x111);
    return gl >= 1 ? y : kTop;
}
#undef TPR_SHR

// The TRACE of the lower-bound LP's cold run (round 4; see cert_lower_sound in tpr_cert_lane.hip.inc and wave_lower_trace in
// tpr_wave.hip.inc): the prologue (the x_next row the corner (1e8, low1) violates lands on the wall x = low1 at u0) and the
// prefix records of the rows' bounds on u at the wall, each with a clear verdict where it is visited, a clearly signed 1-D
// objective on a record's line and the previous record holding at its vertex with a margin.  The rows sit in (slot, lane)
// = visiting order.  r_vi: the row the certificate names; (w0, w1): the LP's warm start, which must not be a valid pair
// (the reference's order is the identity then).
template <int D, int L>
__device__ inline bool predict_lower_trace(const Slots<D, L> &R, const double *rowbuf, int gl, double low1, double high1,
                                           int r_vi, int w0, int w1, double limit_min) {
    using C = GroupCfg<D, L>;
    if constexpr (L != 8 && L != 16) {
        return false;  // (wide groups are a development experiment)
    } else {
        constexpr double kSlack = TPR_SLACK_ABS, kTraceRel = 1e-12, kTop = 3.0e300;
        const bool cold = !(w0 >= 0 && w0 < C::nC && w1 >= 0 && w1 < C::nC && w0 != w1);
        const double d2 = rowbuf[5], n0 = rowbuf[2 * C::nV + 4], n1 = -rowbuf[2 * C::nV + 5];
        const double nb = 1.0 + d2;  // |a| + |b| of the x_next rows: all the prologue touches
        const double tol_c = kSlack + kTraceRel * (nb * (kVarMax + fabs(low1)) + fabs(n0) + fabs(n1));
        bool ok = cold & (-d2 * kVarMax + (n0 - low1) < -tol_c) & (d2 * kVarMax + (low1 - n1) > tol_c) & (d2 > 1e-6) &
                  (high1 - low1 > 1e-6 * (1.0 + fabs(high1) + fabs(low1)));
        const double u0 = (n1 - low1) * rcp_approx(d2);
        ok &= fabs(u0) < kVarMax * (1.0 - 1e-6);
        const double tol0 = kSlack + kTraceRel * (nb * (fabs(u0) + fabs(low1)) + fabs(n0) + fabs(n1));
        ok &= n0 - n1 < -tol0;
        // a floor of -g = -(b low1 + c) over the rows that can be records (the previous record's slope is (-g_prev) / M): the
        // trajectory's smallest acceleration limit, less |b| low1 where the wall is not at 0 (rare: one reduction then)
        double mg_lo = limit_min;  // (the first record's predecessor is the x_next row: slope 2 delta)
        if (__builtin_amdgcn_ballot_w64(low1 != 0.0) != 0) {
            double bmax = 1.0;
#pragma unroll
            for (int s = 0; s < C::S; ++s) bmax = fmax(bmax, fabs(R.b[s]));
            mg_lo = limit_min - group_max_f64<L>(bmax) * fabs(low1);
        }
        ok &= mg_lo > 0.0;
        double t[C::S], g[C::S];
        bool push[C::S];
        bool bad = false;
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
            const int vi = s * L + gl;
            const bool row = (vi >= 6) & (vi < C::nV);
            g[s] = R.b[s] * low1 + R.c[s];
            push[s] = row & (R.a[s] > 1e-7);
            t[s] = push[s] ? -g[s] * rcp_approx(R.a[s]) : kTop;
            bad |= row & (R.a[s] > 0.0) & !push[s] & !(R.a[s] * u0 + g[s] < -tol0);
        }
        double carry = u0, tmin = kTop, t_r = kTop;
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
            const double inc = group_prefix_min_f64<L>(t[s], gl);
            const double M = fmin(carry, group_shift1_f64<L>(inc, gl));  // the running record when this row is visited
            const double r = R.a[s] * M + g[s];
            const double tol = kSlack + kTraceRel * (fabs(R.a[s] * M) + fabs(R.b[s] * low1) + fabs(R.c[s]));
            const bool viol = r > tol;
            bad |= push[s] & !viol & !(r < -tol);
            const bool prev_ok = M >= u0 ? d2 * (M - t[s]) > 1e-2 * tol : mg_lo * (M - t[s]) > 1e-2 * tol * M;
            bad |= push[s] & viol & !((R.a[s] + 1e-9 * R.b[s] > 1e-6) & prev_ok);
            const double total = group_min_f64<L>(t[s]);
            carry = fmin(carry, total);
            tmin = fmin(tmin, total);
            t_r = (s * L + gl == r_vi) ? t[s] : t_r;
        }
        t_r = group_min_f64<L>(t_r);  // (one lane holds it)
        ok &= (r_vi >= 6) ? (t_r == tmin) & (tmin < u0) : !(tmin < u0);
        return ok && group_or_i32<L>(bad ? 1 : 0) == 0;
    }
}

// Lower-bound LP of a backward stage, answered without running Seidel when the answer is certain.
//
// That LP maximises (1e-9 u - x): its optimum is the vertex z* = (u*, low1) where x sits on its box
// bound and u* is the tightest upper bound the rows allow at x = low1 -- provided z* is feasible
// and the tilt cannot pay for a larger x.  Seidel (in any row order, with its 1e-10 / 1e-8
// tolerances) then necessarily ends with pivot row r* (the row defining u*) limited by the box row
// "x >= low1", and the reference's result is a function of those two rows only:
//     x = zp1 + T dt1,  T = -(low1 - zp1) / (-a_r),  zp = -(a_r, b_r) c_r / (a_r^2 + b_r^2).
// This routine finds r*, verifies with margins several orders above the solver's tolerances that
// z* is the unique, well separated optimum (feasibility of every other row, separation from the
// runner-up bound, dual feasibility of the tilt), and evaluates exactly those formulas.  Anything
// marginal (ties, near-degenerate rows, badly scaled problems) returns false and the caller runs
// the full LP, so the result is bit-identical to the reference either way
// (tests/test_gpu_fullsize.py::test_lower_bound_shortcut_is_exact cross-checks every stage LP).
template <int D, int L>
__device__ inline bool predict_lower_lp(const Slots<D, L> &R, const double *rowbuf, int gl, double low0,
                                        double high0, double low1, double high1, GroupLp &o, int w0 = 0, int w1 = 0, double limit_min = 0.0) {
    using C = GroupCfg<D, L>;
    constexpr double kSlack = TPR_SLACK_ABS;     // absolute margin on row residuals (solver tolerances: 1e-10, 1e-8)
    constexpr double kRelSlack = TPR_SLACK_REL;  // relative margin against rounding of the residuals
    // tightest upper bound on u at x = low1 and its row
    double best = 3.0e300;
    int best_vi = kBig;
#pragma unroll
    for (int s = 0; s < C::S; ++s) {
        const int vi = s * L + gl;
        const bool row = (vi >= 4) & (vi < C::nV);
        const double g = R.b[s] * low1 + R.c[s];
        const double ub = -g * rcp_approx(R.a[s]);  // a search: the winner is verified below, the answer comes from its formulas
        const bool cand = row & (R.a[s] > 0.0) & (ub < best);
        best = cand ? ub : best;
        best_vi = cand ? vi : best_vi;
    }
    const double u1 = group_min_f64<L>(best);
    const int r_vi = group_min_i32<L>(best == u1 ? best_vi : kBig);
    if (r_vi == kBig || !(u1 < high0 - 1.0) || !(u1 > low0 + 1.0) || !(low1 <= high1)) return false;
    const double pa = rowbuf[r_vi], pb = rowbuf[C::nV + r_vi], pc = rowbuf[2 * C::nV + r_vi];
    // every other row must hold at z* = (u1, low1) with a margin; rows bounding u from above must
    // in addition be separated from u1 (so that no vertex within the solver's tolerance of z* exists)
    bool bad = false;
#pragma unroll
    for (int s = 0; s < C::S; ++s) {
        const int vi = s * L + gl;
        const bool row = (vi >= 4) & (vi < C::nV) & (vi != r_vi);
        const double au = R.a[s] * u1, g = R.b[s] * low1 + R.c[s];
        const double val = au + g;
        const double tol = kSlack + kRelSlack * (fabs(au) + fabs(R.b[s] * low1) + fabs(R.c[s]));
        bad |= row & !(val < -tol);
        // Seidel classifies rows by the cross product with the pivot row against an absolute 1e-10;
        // require every row to be either exactly parallel/null (cross == 0: the +- twin, a joint
        // that does not move) or clearly not parallel, so that its tolerance tests cannot deviate
        // from exact arithmetic.  This is what keeps badly scaled problems on the full LP.
#ifndef TPR_TOLERANCE_MODE
        const double cross = pa * R.b[s] - pb * R.a[s];
        bad |= row & (cross != 0.0) & !(fabs(cross) > 1e-7);
#endif
        // ... and every row must be either null or of ordinary magnitude: with all row norms >= 1e-2
        // a cross product between two non-twin rows falls under 1e-10 only if they are parallel to
        // ~1e-6 rad or better, i.e. by coincidence; on down-scaled problems (tiny motions) it happens
        // systematically, the reference's pivots then mis-classify rows as parallel and fail
        // spuriously, and only the full iteration reproduces that.
        const double norm1 = fabs(R.a[s]) + fabs(R.b[s]);
        bad |= row & (norm1 != 0.0) & !(norm1 > 5e-2);
    }
    // the pivot row itself: well conditioned, and the tilt (1e-9) must not make a larger x worthwhile
    bad |= !(pa > 1e-6) | !(pb > -1e8 * pa) | !(fabs(pc) < 1e15);
    if (group_or_i32<L>(bad ? 1 : 0) != 0) return false;
#ifdef TPR_TOLERANCE_MODE
    o.ok = true; o.u = u1; o.x = low1; o.ac0 = r_vi - 4; o.ac1 = -3;
    return true;
#endif
    // round 4: every pivot of the reference's run must be predictable, not only its last
    if (!predict_lower_trace<D, L>(R, rowbuf, gl, low1, high1, r_vi, w0, w1, limit_min)) return false;
    // the reference's arithmetic for (pivot r*, limiter = box row x >= low1)
    const double den = pa * pa + pb * pb;
    const double zp0 = (-pa * pc) / den;
    const double zp1 = (-pb * pc) / den;
    const double dt0 = -pb, dt1 = pa;
    const double denom = dt0 * 0.0 + dt1 * -1.0;
    const double num = low1 + zp1 * -1.0 + zp0 * 0.0;
    const double T = -num / denom;
    o.ok = true;
    o.u = zp0 + T * dt0;
    o.x = zp1 + T * dt1;
    o.ac0 = r_vi - 4;
    o.ac1 = -3;
    return true;
}

// Upper-bound LP of a backward stage (max x - 1e-9 u), answered from a verified optimal vertex.
//
// Seidel's result is a function of its LAST pivot only: the pivot row k and the row l that limits
// the 1-D LP on k's line.  When the LP has a unique, well separated optimal vertex z* on rows
// {r1, r2}, the last pivot is necessarily the one of the two that comes later in the reference's
// row order (box rows never pivot), limited by the other:  after the later row has been visited
// the running optimum is z*, and it must have been violated on that visit because without it the
// optimum sits strictly further out (checked below with a margin far above the solver's 1e-10).
// So: (1) find the optimal vertex by a warm-started simplex walk on the stage rows -- the start is
// the previous stage's active pair, which is still optimal ~92% of the time; a dual pivot (enter the
// most violated row, ratio test on the two multipliers) or, when a multiplier went negative, a
// primal line search along the remaining row, moves it otherwise; (2) certify it: every other row
// holds with a margin, the objective is strictly inside the cone of the two normals, the same
// cross-product / row-norm guards as predict_lower_lp keep the solver's absolute-tolerance
// classifications exact (row norms > 0.05 also keep every intermediate pivot's line optimum inside
// the +-1e10 line bounds: |t| <= 2 sqrt(2) 1e8 / |row|); (3) evaluate the reference's pivot
// formulas for (k, l).  Anything marginal returns false and the caller runs the full iteration.
// The walk itself may use any arithmetic; only step (3) has to match the reference bit for bit.
// sound (TPR_SOUND_CERTIFICATES): the walk is ONE dual pivot at most, from a warm vertex at which exactly one row is
// violated and every other row holds with the certificate's margin, and the row that entered must be the last pivot
// (the kept warm row is then part of its 1-D problem); no primal steps.  See cert_propose2 in tpr_cert.hip.inc for the
// argument: only then is the reference's own run predictable up to its last pivot.
template <int D, int L>
__device__ inline bool predict_upper_lp(const Slots<D, L> &R, const double *rowbuf, int gl, double v0, double v1,
                                        double low1, double high1, int wac0, int wac1, GroupLp &o, bool sound = false) {
    using C = GroupCfg<D, L>;
    const int kMaxIt = sound ? 1 : 6;
    int entered = -1;
    constexpr double kSlack = TPR_SLACK_ABS, kRelSlack = TPR_SLACK_REL;
    if (wac0 == wac1 || !(low1 <= high1)) TPR_WALK_FAIL(0);
    int p = wac0 < 0 ? -1 - wac0 : wac0 + 4;  // reference row id -> virtual row
    int q = wac1 < 0 ? -1 - wac1 : wac1 + 4;
    if (p >= C::nV || q >= C::nV) TPR_WALK_FAIL(1);
    double pa, pb, pc, qa, qb, qc, Dm, maxres, vu = 0, vx = 0;
    for (int it = 0;;) {
        pa = rowbuf[p]; pb = rowbuf[C::nV + p]; pc = rowbuf[2 * C::nV + p];
        qa = rowbuf[q]; qb = rowbuf[C::nV + q]; qc = rowbuf[2 * C::nV + q];
        Dm = pa * qb - qa * pb;
        if (!(fabs(Dm) > 1e-7)) TPR_WALK_FAIL(2);
        const double rD = rcp_approx(Dm);  // the walk's vertices only feed searches and margin tests
        const double u = (pb * qc - qb * pc) * rD;
        const double x = (qa * pc - pa * qc) * rD;
        vu = u; vx = x;  // (the tolerance-mode measurement build returns the vertex itself)
        (void)vu; (void)vx;
        // v = lamp n_p + lamq n_q
        const double lamp = (v0 * qb - v1 * qa) * rD, lamq = (pa * v1 - pb * v0) * rD;
        const bool okp = lamp > 0, okq = lamq > 0;
        if (!(okp & okq)) {
            // primal step: drop the row with the negative multiplier, slide along the other one in
            // the improving direction until the first row blocks
            if (sound | !(okp | okq)) TPR_WALK_FAIL(3);
            if (++it > kMaxIt) TPR_WALK_FAIL(4);
            const int keep = okq ? q : p, drop = okq ? p : q;
            const double ka = okq ? qa : pa, kb = okq ? qb : pb;
            double d0 = -kb, d1 = ka;
            if (d0 * v0 + d1 * v1 < 0) { d0 = -d0; d1 = -d1; }
            double tbest = 3.0e300;
            int tvi = kBig;
#pragma unroll
            for (int s = 0; s < C::S; ++s) {
                const int vi = s * L + gl;
                const bool row = (vi < C::nV) & (vi != keep) & (vi != drop);
                const double res = R.a[s] * u + R.b[s] * x + R.c[s];
                const double nd = R.a[s] * d0 + R.b[s] * d1;
                const double t = -res * rcp_approx(nd);  // a search
                const bool cand = row & (nd > 1e-12) & (t < tbest);
                tbest = cand ? t : tbest;
                tvi = cand ? vi : tvi;
            }
            const double g = group_min_f64<L>(tbest);
            const int r = group_min_i32<L>(tbest == g ? tvi : kBig);
            if (r == kBig) TPR_WALK_FAIL(5);
            p = keep;
            q = r;
            continue;
        }
        // residuals of all other rows at the vertex
        double lmax = -3.0e300, lsc = -3.0e300;
        int lvi = kBig;
        double scs[C::S];
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
            const int vi = s * L + gl;
            const bool row = (vi < C::nV) & (vi != p) & (vi != q);
            const double au = R.a[s] * u, bx = R.b[s] * x;
            const double res = au + bx + R.c[s];
            const double sc = res + (kSlack + kRelSlack * (fabs(au) + fabs(bx) + fabs(R.c[s])));
            scs[s] = row ? sc : -3.0e300;
            lsc = (row & (sc > lsc)) ? sc : lsc;
            const bool bigger = row & (res > lmax);
            lmax = bigger ? res : lmax;
            lvi = bigger ? vi : lvi;
        }
        const double gsc = group_max_f64<L>(lsc);
        maxres = group_max_f64<L>(lmax);
        if (gsc < 0) break;  // primal feasible with margins, dual feasible: optimal
        if (!(maxres > 0)) TPR_WALK_FAIL(6);
        if (++it > kMaxIt) TPR_WALK_FAIL(7);
        // dual pivot: the most violated row enters, the ratio test picks the row that leaves
        const int r = group_min_i32<L>(lmax == maxres ? lvi : kBig);
        if (sound) {  // ... provided it is the ONLY row that does not hold with a margin at the warm vertex
            double l2 = -3.0e300;
#pragma unroll
            for (int s = 0; s < C::S; ++s) l2 = ((s * L + gl != r) & (scs[s] > l2)) ? scs[s] : l2;
            if (!(group_max_f64<L>(l2) < 0)) TPR_WALK_FAIL(14);
            entered = r;
        }
        const double ra = rowbuf[r], rb = rowbuf[C::nV + r];
        const double alp = (ra * qb - qa * rb) * rD, alq = (pa * rb - ra * pb) * rD;
        const bool cp = alp > 0, cq = alq > 0;
        if (!(cp | cq)) TPR_WALK_FAIL(8);
        const bool leave_p = cp & (!cq | (lamp * alq <= lamq * alp));
        if (leave_p) p = r; else q = r;
    }
#ifdef TPR_TOLERANCE_MODE
    o.ok = true; o.u = vu; o.x = vx; o.ac0 = row_id_of(p); o.ac1 = row_id_of(q);
    return true;
#endif
    // roles in the reference's last pivot: the later row in its order is the pivot
    if (p < 4 && q < 4) TPR_WALK_FAIL(9);
    const bool warm = wac0 >= 0 && wac0 < C::nC && wac1 >= 0 && wac1 < C::nC;
    int pp = -1, pq = -1;
    if (p >= 4) { const int r = p - 4; pp = !warm ? r : (r == wac1 ? 0 : (r == wac0 ? 1 : 2 + r - (r > wac0 ? 1 : 0) - (r > wac1 ? 1 : 0))); }
    if (q >= 4) { const int r = q - 4; pq = !warm ? r : (r == wac1 ? 0 : (r == wac0 ? 1 : 2 + r - (r > wac0 ? 1 : 0) - (r > wac1 ? 1 : 0))); }
    const bool p_pivot = pp > pq;
    const int k = p_pivot ? p : q, l = p_pivot ? q : p;
    if (entered >= 4 && k != entered) TPR_WALK_FAIL(15);  // (sound: a structural row that entered is the last pivot)
    const double ka = p_pivot ? pa : qa, kb = p_pivot ? pb : qb, kc = p_pivot ? pc : qc;
    const double la = p_pivot ? qa : pa, lb = p_pivot ? qb : pb, lc = p_pivot ? qc : pc;
    bool bad = false, bad_norm = false;
    double nmax = 0;
#pragma unroll
    for (int s = 0; s < C::S; ++s) {
        const int vi = s * L + gl;
        const bool row = vi < C::nV;
        const double cross = ka * R.b[s] - kb * R.a[s];
        bad |= row & (vi != k) & (cross != 0.0) & !(fabs(cross) > 1e-7);
        const double norm1 = fabs(R.a[s]) + fabs(R.b[s]);
        bad_norm |= row & (norm1 != 0.0) & !(norm1 > 5e-2);
        nmax = (row & (norm1 > nmax)) ? norm1 : nmax;
    }
    nmax = group_max_f64<L>(nmax);
    const double v1d = -kb * v0 + ka * v1;
    const bool bad_v1d = !(fabs(v1d) > 1e-6);
    // violation of the pivot row at the optimum of the rows before it: >= |D| m / (max|n| |n_l|),
    // m = smallest margin of the other rows at z*
    const bool bad_viol = !(fabs(Dm) * (-maxres) > 1e-8 * (nmax * (fabs(la) + fabs(lb))));
    if (group_or_i32<L>((bad | bad_norm | bad_v1d | bad_viol) ? 1 : 0) != 0) return false;
    // the reference's arithmetic for (pivot k, limiter l)
    const double den = ka * ka + kb * kb;
    const double zp0 = (-ka * kc) / den;
    const double zp1 = (-kb * kc) / den;
    const double dt0 = -kb, dt1 = ka;
    const double denom = dt0 * la + dt1 * lb;
    const double num = lc + zp1 * lb + zp0 * la;
    const double T = -num / denom;
    o.ok = true;
    o.u = zp0 + T * dt0;
    o.x = zp1 + T * dt1;
    o.ac0 = row_id_of(k);
    o.ac1 = row_id_of(l);
    return true;
}

// 1-D LP of the forward pass on the structural rows: max v0*u s.t. a u + (b x + c) <= 0,
// low0 <= u <= high0.  Returns false when infeasible.
template <int D, int L>
__device__ inline bool group_lp1d(const Slots<D, L> &R, int gl, double v0, double x, double low0,
                                  double high0, double &u_out) {
    using C = GroupCfg<D, L>;
    double tmax = high0, tmin = low0;
#pragma unroll
    for (int s = 0; s < C::S; ++s) {
        const int vi = s * L + gl;
        const bool need = (vi >= 4) & (vi < C::nV);
        const double bxc = R.b[s] * x + R.c[s];
        const double t = -bxc / R.a[s];
        const bool up = need & (R.a[s] > kTiny);
        const bool lo = need & (R.a[s] < -kTiny);
        tmax = (up & (t < tmax)) ? t : tmax;
        tmin = (lo & (t > tmin)) ? t : tmin;
    }
    const double gmax = group_min_f64<L>(tmax);
    const double gmin = group_max_f64<L>(tmin);
    if (gmin > gmax) return false;
    u_out = (fabs(v0) < kTiny || v0 < 0) ? gmin : gmax;
    return true;
}

// group_lp1d that also returns the reference's solution.active_c[0] (cy_seidel_solverwrapper.pyx:93-144): the first row, in
// index order, that attains the bound it reports -- the comparisons are strict, so a row merely equal to the box end does
// not replace it: -1 (lower end of the box) / -2 (upper end) then.  The wrapper object stores it into its warm-start state
// (:646-649), which is why the dense-row entries carry it.
template <int D, int L>
__device__ inline bool group_lp1d_active(const Slots<D, L> &R, int gl, double v0, double x, double low0, double high0,
                                         double &u_out, int &active) {
    using C = GroupCfg<D, L>;
    double tmax = high0, tmin = low0;
    double ts[C::S];
    int cls[C::S];
#pragma unroll
    for (int s = 0; s < C::S; ++s) {
        const int vi = s * L + gl;
        const bool need = (vi >= 4) & (vi < C::nV);
        const double bxc = R.b[s] * x + R.c[s];
        const double t = -bxc / R.a[s];
        const bool up = need & (R.a[s] > kTiny);
        const bool lo = need & (R.a[s] < -kTiny);
        ts[s] = t; cls[s] = up ? 1 : (lo ? 2 : 0);
        tmax = (up & (t < tmax)) ? t : tmax;
        tmin = (lo & (t > tmin)) ? t : tmin;
    }
    const double gmax = group_min_f64<L>(tmax);
    const double gmin = group_max_f64<L>(tmin);
    if (gmin > gmax) return false;
    const bool pick_min = fabs(v0) < kTiny || v0 < 0;
    u_out = pick_min ? gmin : gmax;
    const bool from_row = pick_min ? gmin > low0 : gmax < high0;
    int key = kBig;
#pragma unroll
    for (int s = 0; s < C::S; ++s) {
        const bool hit = from_row & (cls[s] == (pick_min ? 2 : 1)) & (ts[s] == u_out);
        const int cand = hit ? s * L + gl : kBig;
        key = cand < key ? cand : key;
    }
    key = group_min_i32<L>(key);
    active = key < kBig ? key - 4 : (pick_min ? -1 : -2);
    return true;
}

struct GroupArgs {
    int B, nseg, N, flags;
    const double *coef, *breaks, *grid, *vlim, *alim, *sd_start, *sd_end;
    double *sd2, *sd, *u, *K;
    int32_t *status;
    // compute_controllable_sets(sdmin, sdmax) on its own: K[N] = [sd_end^2, sd_end_hi^2], no forward scan
    const double *sd_end_hi = nullptr;
    int backward_only = 0;
    // TOPPRAsd on family 3 (cert_solve_kernel<..., SDFWD = true>): the fastest / slowest forward profiles
    // x [B][N+1], u [B][N] written after the backward scan of the same launch
    double *sd_xf = nullptr, *sd_uf = nullptr, *sd_xl = nullptr, *sd_ul = nullptr;
    // kernel family 3 above 8 dof (slim blocks): a workspace of cert_tws_doubles(d, nseg) doubles per 64-trajectory block into
    // which every block transposes what it re-reads per stage -- acceleration limits, velocity limits, spline coefficients --
    // as [field][lane] (SURVEY section 7's batch-innermost layout, block by block)
    double *tws = nullptr;
    // TOPPRAsd on family 3: the durations of the fastest / slowest profile, [B][2], summed in the forward scan itself in the
    // reference's order (desired_duration_algorithm.py:11-18) -- sd_finish_kernel then starts from them instead of two passes
    double *sd_dur = nullptr;
};
// From which dof on the certified lane kernels re-read the spline segment's coefficients per stage instead of holding them in
// registers (tpr_cert.hip.inc: kLeanCoef).
#ifndef TPR_LEAN_COEF_FROM
#define TPR_LEAN_COEF_FROM 11
#endif
// fields of the transposed workspace per lane: alim [2 d], vlim [2 d], then -- where the kernel re-reads them -- c0, c1, c2 [nseg][d]
// when the table is short enough
constexpr int kTwsMaxSeg = 16;
__host__ __device__ inline size_t cert_tws_fields(int d, int nseg) {
    return (size_t)4 * d + (d >= TPR_LEAN_COEF_FROM && nseg <= kTwsMaxSeg ? (size_t)3 * nseg * d : 0);
}

// A gridpoint located on the spline: segment index and local parameter.
struct GridPt {
    int j;
    double t;
};

// Per-slot constants of a trajectory + stage row construction.
template <int D, int L>
struct GroupTraj {
    using C = GroupCfg<D, L>;
    int dof[C::S];      // dof of an acceleration row, -1 otherwise
    bool neg[C::S];     // row is the negated half of its +- pair
    bool nextpt[C::S];  // row evaluates at s_{i+1} (interpolation block)
    double climit[C::S];
    double limit_min = 0.0;  // min over the dofs of min(amax, -amin): a floor of -c over the acceleration rows (predict_lower_trace)
    static constexpr int VS = (D + L - 1) / L;
    double vlo[VS], vhi[VS];  // velocity limits of dofs gl, gl+L, ... (has_vel)
    const double *cf;      // LDS: [3][nseg][D] (cubic coefficients c0, c1, c2)
    const double *breaks;  // LDS: [nseg+1]
    double *rowbuf;        // LDS: a[nV], b[nV], c[nV]
    int nseg;
    bool has_vel;
    // acceleration blocks of D rows each that exist: 4 (Interpolation, the reference's default), 2
    // (Collocation: rows at s_i only), 0 (no acceleration constraint).  The slots of the missing blocks
    // hold the disabled row (0, 0, -1), which Seidel never pivots on and never projects (denominator 0,
    // numerator -1), so row indices, visiting order and results are those of the reference's smaller LP.
    int nblk = 4;

    __device__ inline void set_flags(int flags) {
        has_vel = flags & TPR_HAS_VELOCITY;
        nblk = (flags & TPR_HAS_ACCELERATION) ? ((flags & TPR_ACC_INTERPOLATION) ? 4 : 2) : 0;
    }

    __device__ inline void init(int gl, const double *alim, const double *vlim) {
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
            const int vi = s * L + gl;
            const int m = vi - 6;
            const bool acc = m >= 0 && m < nblk * D;
            const int blk = acc ? m / D : 0;
            dof[s] = acc ? m - blk * D : -1;
            neg[s] = blk & 1;
            nextpt[s] = blk >> 1;
            climit[s] = acc ? ((blk & 1) ? alim[2 * dof[s]] : -alim[2 * dof[s] + 1]) : 0.0;
        }
        {
            double lm = 3.0e300;
#pragma unroll
            for (int s = 0; s < C::S; ++s) lm = (dof[s] >= 0 && -climit[s] < lm) ? -climit[s] : lm;
            limit_min = group_min_f64<L>(lm);
        }
#pragma unroll
        for (int v = 0; v < VS; ++v) {
            const int k = gl + v * L;
            vlo[v] = (has_vel && k < D) ? vlim[2 * k] : 0.0;
            vhi[v] = (has_vel && k < D) ? vlim[2 * k + 1] : 0.0;
        }
    }

    __device__ inline GridPt locate(double s) const {
        GridPt g;
        g.j = find_segment(breaks, nseg, s);
        g.t = s - breaks[g.j];
        return g;
    }

    __device__ inline void eval(int k, const GridPt &g, double &q1, double &q2) const {
        cubic_d1_d2(cf[(0 * nseg + g.j) * D + k], cf[(1 * nseg + g.j) * D + k], cf[(2 * nseg + g.j) * D + k],
                    g.t, q1, q2);
    }

    // Rows of stage i (gridpoints s_i = gi, s_{i+1} = gn); x_next pair from (n0, n1); box from
    // the velocity limit at s_i.  Mirrors the rows into LDS when MIRROR (the 2-D LP needs it).
    // last: the stage of the final gridpoint (feasible sets only) -- its interpolation block repeats the
    // stage's own rows and the x_next pair is disabled (linear_constraint.py:172,177).
    template <bool MIRROR>
    __device__ inline void build(Slots<D, L> &R, int gl, const GridPt &gi, const GridPt &gn, double delta,
                                 double n0, double n1, double &low1, double &high1, bool last = false) const {
        low1 = kVarMin; high1 = kVarMax;
        if (has_vel) {
            float sdmin = -kJvelMaxSd, sdmax = kJvelMaxSd;
#pragma unroll
            for (int v = 0; v < VS; ++v) {
                const int k = gl + v * L;
                if (k < D) {
                    double q1, q2;
                    eval(k, gi, q1, q2);
                    // q1 > 0: sdmax <- vhi/q1, sdmin <- vlo/q1 ; q1 < 0: swapped (fp32-rounded, as the reference)
                    const double rmax = (q1 > 0 ? vhi[v] : vlo[v]) / q1, rmin = (q1 > 0 ? vlo[v] : vhi[v]) / q1;
                    if (q1 != 0 && !isnan(q1)) {
                        sdmax = (float)(rmax <= (double)sdmax ? rmax : (double)sdmax);
                        sdmin = (float)(rmin >= (double)sdmin ? rmin : (double)sdmin);
                    }
                }
            }
            sdmax = group_min_f32<L>(sdmax);
            sdmin = group_max_f32<L>(sdmin);
            const float up = sdmax * sdmax;
            const double lo = (double)sdmin >= 0.0 ? (double)sdmin : 0.0;
            const double xlo = lo * lo, xhi = (double)up;
            low1 = low1 > xlo ? low1 : xlo;
            high1 = high1 < xhi ? high1 : xhi;
        }
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
            const int vi = s * L + gl;
            // straight-line on purpose: an if / else-if chain on the row index is lowered to a tree of
            // divergent branches.  Empty slots hold the disabled row (0, 0, -1).
            double a = 0, b = 0, c = -1;
            if (s == 0) {  // the box rows and the x_next pair live in slot 0 (L >= 8)
                const double ta[6] = {-1.0, 1.0, 0.0, 0.0, last ? 0.0 : -2 * delta, last ? 0.0 : 2 * delta};
                const double tb[6] = {0.0, 0.0, -1.0, 1.0, last ? 0.0 : -1.0, last ? 0.0 : 1.0};
                const double tc[6] = {kVarMin, -kVarMax, low1, -high1, last ? -1.0 : n0, last ? -1.0 : -n1};
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const bool hit = vi == j;
                    a = hit ? ta[j] : a;
                    b = hit ? tb[j] : b;
                    c = hit ? tc[j] : c;
                }
            }
            {
                const bool acc = dof[s] >= 0;
                double q1, q2;
                const bool nx = nextpt[s] & !last;
                eval(acc ? dof[s] : 0, nx ? gn : gi, q1, q2);
                const double av = nx ? q1 + (2 * delta) * q2 : q1;
                a = acc ? (neg[s] ? -av : av) : a;
                b = acc ? (neg[s] ? -q2 : q2) : b;
                c = acc ? climit[s] : c;
            }
            R.a[s] = a; R.b[s] = b; R.c[s] = c;
            if (MIRROR && vi < C::nV) {
                rowbuf[vi] = a; rowbuf[C::nV + vi] = b; rowbuf[2 * C::nV + vi] = c;
            }
        }
        if (MIRROR) {  // rows are read back by other lanes of the wave: stores before, loads after, in the memory model too
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
};

template <int D, int L, bool TABLE_IN_LDS>
__global__ void __launch_bounds__(256, TPR_GROUP_WAVES) group_solve_kernel(GroupArgs A) {
    using C = GroupCfg<D, L>;
    const int kGroupsPerBlock = blockDim.x / L;
    extern __shared__ double lds[];
    const int tid = threadIdx.x, gl = tid % L;
    const int gidx = tid / L;
    const int b = blockIdx.x * kGroupsPerBlock + gidx;
    const bool alive0 = b < A.B;
    const int bb = alive0 ? b : A.B - 1;  // idle groups shadow the last trajectory, never store
    const int N = A.N, nseg = A.nseg;

    // stage this group's spline table (c0, c1, c2) and breakpoints in LDS when they fit; the
    // global layout [4][nseg][D] starts with the same three blocks, so the indexing is shared
    double *rowbuf = lds + (size_t)gidx * C::lds_doubles(nseg, TABLE_IN_LDS);
    const double *gcf = A.coef + (size_t)bb * 4 * nseg * D;
    const double *gbrk = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? (size_t)bb * (nseg + 1) : 0);
    const double *cf = gcf, *brk = gbrk;
    if (TABLE_IN_LDS) {  // compile-time: keeps the address space of cf / brk known to the compiler
        double *lcf = rowbuf + C::kRowBuf, *lbrk = lcf + 3 * nseg * D;
        for (int e = gl; e < 3 * nseg * D; e += L) lcf[e] = gcf[e];
        for (int e = gl; e <= nseg; e += L) lbrk[e] = gbrk[e];
        cf = lcf;
        brk = lbrk;
    }
    __syncthreads();

    GroupTraj<D, L> T;
    T.cf = cf;
    T.breaks = brk;
    T.rowbuf = rowbuf;
    T.nseg = nseg;
    T.set_flags(A.flags);
    T.init(gl, T.nblk ? A.alim + (size_t)bb * 2 * D : nullptr, T.has_vel ? A.vlim + (size_t)bb * 2 * D : nullptr);
    const double *grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)bb * (N + 1) : 0);

    Slots<D, L> R;
    double *K = A.K + (size_t)bb * 2 * (N + 1);
    double *xs = A.sd2 ? A.sd2 + (size_t)bb * (N + 1) : nullptr;
    double *sdv = A.sd ? A.sd + (size_t)bb * (N + 1) : nullptr;
    double *us = A.u ? A.u + (size_t)bb * N : nullptr;
    const bool writer = alive0 && gl == 0;
    const double sd_start = A.sd_start ? A.sd_start[bb] : 0.0;
    const double sd_end = A.sd_end ? A.sd_end[bb] : 0.0;

    // ---- backward scan: controllable sets ------------------------------------------------
    int up0 = 0, up1 = 0, dn0 = 0, dn1 = 0;  // warm-start state (active_c_up / active_c_down)
    const bool use_shortcut = TPR_PREDICT_LOWER && !(A.flags & TPR_STRICT_SEIDEL);
    double kn0 = boundary_x(A.flags, sd_end), kn1 = A.sd_end_hi ? boundary_x(A.flags, A.sd_end_hi[bb]) : kn0;
    if (writer) { K[2 * N] = kn0; K[2 * N + 1] = kn1; }
    bool failed = false;
    double s_n = grid[N];
    GridPt gn = T.locate(s_n);
    double s_prefetch = grid[N - 1];
    for (int i = N - 1; i >= 0; --i) {
        const double s_i = s_prefetch;
        if (i > 0) s_prefetch = grid[i - 1];
        const double delta = s_n - s_i;
        const GridPt gi = T.locate(s_i);
        double lo = 0, hi = 0;
        if (!failed) {
            if (isnan(kn0) || isnan(kn1)) { lo = qnan(); hi = qnan(); }
            else {
                double low1, high1;
                T.template build<true>(R, gl, gi, gn, delta, kn0, kn1, low1, high1);
                GroupLp su;
                const bool up_hit = use_shortcut && TPR_PREDICT_UPPER &&
                                    predict_upper_lp<D, L>(R, T.rowbuf, gl, -1e-9, 1.0, low1, high1, dn0, dn1, su,
#ifdef TPR_TOLERANCE_MODE
                                                           false);
#else
                                                           true);  // round 4: the sound mode is the only mode (a moved pair: one predictable pivot, else the iteration)
#endif
                if (!up_hit) su = group_lp2d<D, L>(R, T.rowbuf, gl, -1e-9, 1.0, kVarMin, kVarMax, low1, high1, dn0, dn1);
                if (su.ok) { dn0 = su.ac0; dn1 = su.ac1; }
                hi = su.x;
                {
                    GroupLp sl;
                    if (!(use_shortcut && predict_lower_lp<D, L>(R, T.rowbuf, gl, kVarMin, kVarMax, low1, high1, sl, up0, up1, T.limit_min)))
                        sl = group_lp2d<D, L>(R, T.rowbuf, gl, 1e-9, -1.0, kVarMin, kVarMax, low1, high1, up0, up1);
                    if (sl.ok) { up0 = sl.ac0; up1 = sl.ac1; }
                    lo = sl.x;
                }
            }
            if (lo < 0) lo = 0;
            if (isnan(lo) || isnan(hi)) failed = true;
        }
        if (writer) { K[2 * i] = lo; K[2 * i + 1] = hi; }
        kn0 = lo; kn1 = hi;
        s_n = s_i;
        gn = gi;
    }

    const double x_start = boundary_x(A.flags, sd_start);
    // K[0] is (kn0, kn1) after the loop
    if (A.backward_only) {  // controllable sets on their own (+ the controllability verdict for TOPPRAsd)
        if (writer && A.status)
            A.status[bb] = (failed || x_start + kPySmall < kn0 || kn1 + kPySmall < x_start) ? TPR_STATUS_FAIL_UNCONTROLLABLE
                                                                                             : TPR_STATUS_OK;
        return;
    }
    if (failed || x_start + kPySmall < kn0 || kn1 + kPySmall < x_start) {
        if (writer) {
            for (int i = 0; i <= N; ++i) { if (xs) xs[i] = qnan(); if (sdv) sdv[i] = qnan(); }
            for (int i = 0; i < N; ++i) if (us) us[i] = qnan();
            if (A.status) A.status[bb] = TPR_STATUS_FAIL_UNCONTROLLABLE;
        }
        return;
    }
    __threadfence_block();  // K rows written by lane 0 are re-read by the whole group below

    // ---- forward scan: parameterization ----------------------------------------------------
    double x = x_start;
    double sq = sqrt(x);
    bool any_nan = isnan(sq);
    if (writer) { if (xs) xs[0] = x; if (sdv) sdv[0] = sq; }
    int tries = 0, i = 0;
    bool rows_ready = false;
    double delta = 0, k0 = 0, k1 = 0;
    // gn currently locates grid[0]; software-prefetch the next stage's grid point and K row
    GridPt gi = gn;
    double s_cur = s_n;
    double s_pf = grid[1], k0_pf = K[2], k1_pf = K[3];
    while (i < N) {
        if (!rows_ready) {
            const double s_nx = s_pf;
            k0 = k0_pf; k1 = k1_pf;
            if (i + 2 <= N) { s_pf = grid[i + 2]; k0_pf = K[2 * (i + 2)]; k1_pf = K[2 * (i + 2) + 1]; }
            delta = s_nx - s_cur;
            gn = T.locate(s_nx);
            double low1, high1;
            T.template build<false>(R, gl, gi, gn, delta, k0, k1, low1, high1);
            s_cur = s_nx;
            rows_ready = true;
        }
        double uu = qnan();
        bool ok = false;
        if (!isnan(x)) ok = group_lp1d<D, L>(R, gl, 2 * delta, x, kVarMin, kVarMax, uu);
        if (!ok) {
            if (tries < kMaxTries) {
                const double t1 = x - kPyTiny, t2 = 0.999 * x;
                x = t2 > t1 ? t2 : t1;
                tries += 1;
                if (writer) { if (xs) xs[i] = x; if (sdv) sdv[i] = sqrt(x); }
            } else {
                if (writer) {
                    for (int m = i + 1; m <= N; ++m) { if (xs) xs[m] = qnan(); if (sdv) sdv[m] = qnan(); }
                    for (int m = i; m < N; ++m) if (us) us[m] = 0.0;
                }
                any_nan = true;
                break;
            }
        } else {
            tries = 0;
            double xn = x + (2 * delta) * uu;
            const double t1 = xn - kPyTiny, t2 = 0.9999 * xn;
            xn = t2 > t1 ? t2 : t1;
            const double m1 = xn > k0 ? xn : k0;
            x = m1 < k1 ? m1 : k1;
            sq = sqrt(x);
            if (writer) {
                if (us) us[i] = uu;
                if (xs) xs[i + 1] = x;
                if (sdv) sdv[i + 1] = sq;
            }
            any_nan |= isnan(sq);
            rows_ready = false;
            gi = gn;
            i += 1;
        }
    }
    if (writer && A.status) A.status[bb] = any_nan ? TPR_STATUS_ERR_UNKNOWN : TPR_STATUS_OK;
}

// ---- compute_feasible_sets: reachability_algorithm.py:131-164 -------------------------------------
// Per stage two 2-D LPs (min x, max x) with x and x_next boxed to +-CVXPY_MAXX; the stages are
// independent in exact arithmetic but the reference carries its warm-start state along them, which
// this reproduces (full iteration, as lane_feasible_kernel).
template <int D, int L, bool TABLE_IN_LDS>
__global__ void __launch_bounds__(256, 3) group_feasible_kernel(GroupArgs A, double *X) {
    using C = GroupCfg<D, L>;
    const int kGroupsPerBlock = blockDim.x / L;
    extern __shared__ double lds[];
    const int tid = threadIdx.x, gl = tid % L, gidx = tid / L;
    const int b = blockIdx.x * kGroupsPerBlock + gidx;
    const bool alive0 = b < A.B;
    const int bb = alive0 ? b : A.B - 1;
    const int N = A.N, nseg = A.nseg;
    double *rowbuf = lds + (size_t)gidx * C::lds_doubles(nseg, TABLE_IN_LDS);
    const double *gcf = A.coef + (size_t)bb * 4 * nseg * D;
    const double *gbrk = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? (size_t)bb * (nseg + 1) : 0);
    const double *cf = gcf, *brk = gbrk;
    if (TABLE_IN_LDS) {
        double *lcf = rowbuf + C::kRowBuf, *lbrk = lcf + 3 * nseg * D;
        for (int e = gl; e < 3 * nseg * D; e += L) lcf[e] = gcf[e];
        for (int e = gl; e <= nseg; e += L) lbrk[e] = gbrk[e];
        cf = lcf;
        brk = lbrk;
    }
    __syncthreads();
    GroupTraj<D, L> T;
    T.cf = cf; T.breaks = brk; T.rowbuf = rowbuf; T.nseg = nseg;
    T.set_flags(A.flags);
    T.init(gl, T.nblk ? A.alim + (size_t)bb * 2 * D : nullptr, T.has_vel ? A.vlim + (size_t)bb * 2 * D : nullptr);
    const double *grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)bb * (N + 1) : 0);
    Slots<D, L> R;
    double *Xb = X + (size_t)bb * 2 * (N + 1);
    const bool writer = alive0 && gl == 0;
    int up0 = 0, up1 = 0, dn0 = 0, dn1 = 0;
    double s_i = grid[0];
    GridPt gi = T.locate(s_i);
    for (int i = 0; i <= N; ++i) {
        const bool last = i == N;
        const double s_nx = last ? s_i : grid[i + 1];
        const double delta = s_nx - s_i;
        const GridPt gn = last ? gi : T.locate(s_nx);
        double low1, high1;
        T.template build<true>(R, gl, gi, gn, delta, -kFeasMaxX, kFeasMaxX, low1, high1, last);
        // x_min / x_max of solve_stagewise_optim intersect the box (cy_seidel_solverwrapper.pyx:598-601)
        low1 = low1 > -kFeasMaxX ? low1 : -kFeasMaxX;
        high1 = high1 < kFeasMaxX ? high1 : kFeasMaxX;
#pragma unroll
        for (int s = 0; s < C::S; ++s) {
            const int vi = s * L + gl;
            if (vi == 2) R.c[s] = low1;
            if (vi == 3) R.c[s] = -high1;
        }
        GroupLp sl = group_lp2d<D, L>(R, T.rowbuf, gl, -1e-9, -1.0, kVarMin, kVarMax, low1, high1, up0, up1);
        if (sl.ok) { up0 = sl.ac0; up1 = sl.ac1; }
        GroupLp su = group_lp2d<D, L>(R, T.rowbuf, gl, 1e-9, 1.0, kVarMin, kVarMax, low1, high1, dn0, dn1);
        if (su.ok) { dn0 = su.ac0; dn1 = su.ac1; }
        double lo = sl.x;
        if (lo < 0) lo = 0;
        if (writer) { Xb[2 * i] = lo; Xb[2 * i + 1] = su.x; }
        s_i = s_nx;
        gi = gn;
    }
}

// ---- TOPPRAsd (desired duration): desired_duration_algorithm.py:42-234 ---------------------------
struct SdArgs {
    int B, nseg, N, flags;
    const double *coef, *breaks, *grid, *vlim, *alim, *sd_start;
    const double *K;            // [B][N+1][2] from the backward scan
    const int32_t *status_in;   // [B] status of the time-optimal solve (1 = uncontrollable)
    double *xf, *uf, *xl, *ul;  // fastest / slowest profiles: x [B][N+1], u [B][N]
};

// The two forward scans of TOPPRAsd -- "fastest" (objective [-2 delta, -1]) and "slowest"
// ([2 delta, 1], :219-226) -- share the stage rows, so they run side by side on one row build.
// Unlike TOPPRA's forward scan there is no retry, the shrink is "- SMALL" (1e-5, :117) and a NaN
// stage poisons the rest of the profile.
template <int D, int L, bool TABLE_IN_LDS>
__global__ void __launch_bounds__(256, 3) group_sd_forward_kernel(SdArgs A) {
    using C = GroupCfg<D, L>;
    const int kGroupsPerBlock = blockDim.x / L;
    extern __shared__ double lds[];
    const int tid = threadIdx.x, gl = tid % L;
    const int gidx = tid / L;
    const int b = blockIdx.x * kGroupsPerBlock + gidx;
    const bool alive0 = b < A.B;
    const int bb = alive0 ? b : A.B - 1;
    const int N = A.N, nseg = A.nseg;
    double *rowbuf = lds + (size_t)gidx * C::lds_doubles(nseg, TABLE_IN_LDS);
    const double *gcf = A.coef + (size_t)bb * 4 * nseg * D;
    const double *gbrk = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? (size_t)bb * (nseg + 1) : 0);
    const double *cf = gcf, *brk = gbrk;
    if (TABLE_IN_LDS) {
        double *lcf = rowbuf + C::kRowBuf, *lbrk = lcf + 3 * nseg * D;
        for (int e = gl; e < 3 * nseg * D; e += L) lcf[e] = gcf[e];
        for (int e = gl; e <= nseg; e += L) lbrk[e] = gbrk[e];
        cf = lcf;
        brk = lbrk;
    }
    __syncthreads();
    GroupTraj<D, L> T;
    T.cf = cf; T.breaks = brk; T.rowbuf = rowbuf; T.nseg = nseg;
    T.set_flags(A.flags);
    T.init(gl, T.nblk ? A.alim + (size_t)bb * 2 * D : nullptr, T.has_vel ? A.vlim + (size_t)bb * 2 * D : nullptr);
    const double *grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)bb * (N + 1) : 0);
    const double *K = A.K + (size_t)bb * 2 * (N + 1);
    double *xf = A.xf + (size_t)bb * (N + 1), *xl = A.xl + (size_t)bb * (N + 1);
    double *uf = A.uf + (size_t)bb * N, *ul = A.ul + (size_t)bb * N;
    const bool writer = alive0 && gl == 0;
    Slots<D, L> R;
    const double sd_start = A.sd_start ? A.sd_start[bb] : 0.0;
    double x_fast = boundary_x(A.flags, sd_start), x_slow = x_fast;
    if (A.status_in[bb] == TPR_STATUS_FAIL_UNCONTROLLABLE) { x_fast = qnan(); x_slow = qnan(); }
    if (writer) { xf[0] = x_fast; xl[0] = x_slow; }
    double s_cur = grid[0];
    GridPt gi = T.locate(s_cur);
    for (int i = 0; i < N; ++i) {
        const double s_nx = grid[i + 1];
        const double delta = s_nx - s_cur;
        const double k0 = K[2 * (i + 1)], k1 = K[2 * (i + 1) + 1];
        const GridPt gn = T.locate(s_nx);
        double low1, high1;
        T.template build<false>(R, gl, gi, gn, delta, k0, k1, low1, high1);
        // fastest: max u ; slowest: min u (v0 = -g0 = -2 delta < 0 picks the lower end)
        double u_fast = qnan(), u_slow = qnan();
        bool ok_fast = false, ok_slow = false;
        if (!isnan(x_fast)) ok_fast = group_lp1d<D, L>(R, gl, 2 * delta, x_fast, kVarMin, kVarMax, u_fast);
        if (!isnan(x_slow)) ok_slow = group_lp1d<D, L>(R, gl, -2 * delta, x_slow, kVarMin, kVarMax, u_slow);
        if (ok_fast) {
            const double xn = x_fast + (2 * delta) * u_fast - kPySmall;
            const double m1 = xn > k0 ? xn : k0;
            x_fast = m1 < k1 ? m1 : k1;
        } else { u_fast = qnan(); x_fast = qnan(); }
        if (ok_slow) {
            const double xn = x_slow + (2 * delta) * u_slow - kPySmall;
            const double m1 = xn > k0 ? xn : k0;
            x_slow = m1 < k1 ? m1 : k1;
        } else { u_slow = qnan(); x_slow = qnan(); }
        if (writer) { uf[i] = u_fast; xf[i + 1] = x_fast; ul[i] = u_slow; xl[i + 1] = x_slow; }
        s_cur = s_nx;
        gi = gn;
    }
}

struct SdBlendArgs {
    int B, N, flags;
    double atol;
    const double *grid, *desired;
    const double *xf, *uf, *xl, *ul;
    const int32_t *status_in;
    double *sd2, *sd, *u, *alpha;
    int32_t *status;
    const double *deltas = nullptr;  // [B][N] instead of differences of `grid` (the dense-row entries hold no grid)
    const double *dur = nullptr;     // [B][2]: durations of the fastest / slowest profile when the forward scans summed them (family 3)
};

// step i of a trajectory: from its deltas row when there is one, else the difference of its gridpoints (the same bits:
// the reference computes deltas once, as that difference)
__device__ __forceinline__ double sd_step(const double *deltas, const double *grid, int i) {
    return deltas ? deltas[i] : grid[i + 1] - grid[i];
}

// _compute_duration (:11-18): sequential sum, 1e-9 regularisation.
__device__ inline double sd_duration(const double *xf, const double *xl, double alpha, bool blend,
                                     const double *grid, int N, const double *deltas = nullptr) {
    double t = 0;
    double prev = blend ? alpha * xf[0] + (1 - alpha) * xl[0] : xf[0];
    double sprev = sqrt(prev);
    for (int i = 0; i < N; ++i) {
        const double nx = blend ? alpha * xf[i + 1] + (1 - alpha) * xl[i + 1] : xf[i + 1];
        const double sn = sqrt(nx);
        t += 2 * sd_step(deltas, grid, i) / (sn + sprev + 1e-9);
        sprev = sn;
    }
    return t;
}

// Duration bisection and the final convex combination (:144-191) in three steps, so that lanes of a wave do the same
// work (as ONE kernel -- a thread per trajectory running everything -- the few trajectories that bisect kept their waves
// alive at 12 of 64 lanes active: 2.0 ms at 65536 x 200):
//   sd_decide_kernel  a thread per trajectory: the durations of the fastest and the slowest profile, alpha = 1 / 0 when
//                     the desired duration is out of reach, else an entry in the worklist;
//   sd_bisect_kernel  a thread per worklist entry: the bisection on alpha (every lane iterates ~ log2(range / atol) times);
//   sd_blend_kernel   a wave per trajectory: x = alpha xf + (1 - alpha) xl, sd = sqrt(x), u likewise -- coalesced rows.
// The duration sums are sequential per trajectory, in the reference's order.
static __global__ void __launch_bounds__(64) sd_decide_kernel(SdBlendArgs A, int32_t *worklist, int32_t *count) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= A.B) return;
    if (A.status_in[b] == TPR_STATUS_FAIL_UNCONTROLLABLE) {
        A.alpha[b] = qnan();
        return;
    }
    const int N = A.N;
    const double *grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)b * (N + 1) : 0);
    const double *xf = A.xf + (size_t)b * (N + 1), *xl = A.xl + (size_t)b * (N + 1);
    const double desired = A.desired[b];
    const double *dl = A.deltas ? A.deltas + (size_t)b * N : nullptr;
    const double duration = sd_duration(xf, xl, 1.0, false, grid, N, dl);
    const double duration_slow = sd_duration(xl, xf, 1.0, false, grid, N, dl);
    if (duration > desired) A.alpha[b] = 1.0;
    else if (duration_slow < desired) A.alpha[b] = 0.0;
    else worklist[atomicAdd(count, 1)] = b;
}

static __global__ void __launch_bounds__(64) sd_bisect_kernel(SdBlendArgs A, const int32_t *worklist, const int32_t *count) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= *count) return;
    const int b = worklist[e];
    const int N = A.N;
    const double *grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)b * (N + 1) : 0);
    const double *xf = A.xf + (size_t)b * (N + 1), *xl = A.xl + (size_t)b * (N + 1);
    const double desired = A.desired[b];
    double alpha = 0.0, alpha_low = 1.0, alpha_high = 0.0, diff = 10;
    while (diff > A.atol) {
        alpha = 0.5 * (alpha_low + alpha_high);
        if (alpha == alpha_low || alpha == alpha_high) break;  // interval exhausted (the reference would spin)
        const double da = sd_duration(xf, xl, alpha, true, grid, N, A.deltas ? A.deltas + (size_t)b * N : nullptr);
        if (da < desired) { alpha_low = alpha; diff = desired - da; }
        else { alpha_high = alpha; diff = da - desired; }
    }
    A.alpha[b] = alpha;
}

static __global__ void __launch_bounds__(64) sd_blend_kernel(SdBlendArgs A) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int N = A.N;
    double *xs = A.sd2 ? A.sd2 + (size_t)b * (N + 1) : nullptr;
    double *sdv = A.sd ? A.sd + (size_t)b * (N + 1) : nullptr;
    double *us = A.u ? A.u + (size_t)b * N : nullptr;
    if (A.status_in[b] == TPR_STATUS_FAIL_UNCONTROLLABLE) {
        for (int i = lane; i <= N; i += 64) { if (xs) xs[i] = qnan(); if (sdv) sdv[i] = qnan(); }
        for (int i = lane; i < N; i += 64) if (us) us[i] = qnan();
        if (lane == 0 && A.status) A.status[b] = TPR_STATUS_FAIL_UNCONTROLLABLE;
        return;
    }
    const double *xf = A.xf + (size_t)b * (N + 1), *xl = A.xl + (size_t)b * (N + 1);
    const double *uf = A.uf + (size_t)b * N, *ul = A.ul + (size_t)b * N;
    const double alpha = A.alpha[b];
    bool any_nan = false;
    for (int i = lane; i <= N; i += 64) {
        const double x = alpha * xf[i] + (1 - alpha) * xl[i];
        const double sq = sqrt(x);
        any_nan |= isnan(sq);
        if (xs) xs[i] = x;
        if (sdv) sdv[i] = sq;
    }
    for (int i = lane; i < N; i += 64) if (us) us[i] = alpha * uf[i] + (1 - alpha) * ul[i];
    const bool bad = __builtin_amdgcn_ballot_w64(any_nan) != 0;
    if (lane == 0 && A.status) A.status[b] = bad ? TPR_STATUS_ERR_UNKNOWN : TPR_STATUS_OK;
}

// The same three steps with ONE WAVE PER TRAJECTORY (the default; the kernels above serve N too large for the LDS
// rows): the profiles are read once, coalesced, into LDS; the square roots and the quotients of a duration are
// computed lane-parallel over the gridpoints and then summed by a sequential loop in the reference's order
// (_compute_duration, :11-18); every decision is wave-uniform, so a trajectory that bisects costs its own wave ~19
// passes and nobody else anything (thread-per-trajectory: 0.8 ms for the 5 % that bisect, at 500 cycles per gridpoint
// of strided loads).  LDS: 5 (N + 1) doubles.
static __global__ void __launch_bounds__(64) sd_finish_kernel(SdBlendArgs A) {
    extern __shared__ double sdl[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int N = A.N;
    double *xs = A.sd2 ? A.sd2 + (size_t)b * (N + 1) : nullptr;
    double *sdv = A.sd ? A.sd + (size_t)b * (N + 1) : nullptr;
    double *us = A.u ? A.u + (size_t)b * N : nullptr;
    if (A.status_in[b] == TPR_STATUS_FAIL_UNCONTROLLABLE) {  // (wave-uniform)
        for (int i = lane; i <= N; i += 64) { if (xs) xs[i] = qnan(); if (sdv) sdv[i] = qnan(); }
        for (int i = lane; i < N; i += 64) if (us) us[i] = qnan();
        if (lane == 0) { if (A.alpha) A.alpha[b] = qnan(); if (A.status) A.status[b] = TPR_STATUS_FAIL_UNCONTROLLABLE; }
        return;
    }
    double *Lf = sdl, *Ll = Lf + (N + 1), *Ln = Ll + (N + 1), *Ls = Ln + (N + 1), *Lt = Ls + (N + 1);
    const double *grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)b * (N + 1) : 0);
    const double *xf = A.xf + (size_t)b * (N + 1), *xl = A.xl + (size_t)b * (N + 1);
    // The profiles go to LDS only for a wave that needs duration passes: with the two durations handed in (A.dur: family 3 sums
    // them in its forward scans) that is the ~5 % of the trajectories that bisect; everybody else blends straight from global
    // memory (wave-uniform throughout).
    bool staged = false;
    auto stage = [&]() {
        for (int i = lane; i <= N; i += 64) { Lf[i] = xf[i]; Ll[i] = xl[i]; }
        for (int i = lane; i < N; i += 64) Ln[i] = 2 * sd_step(A.deltas ? A.deltas + (size_t)b * N : nullptr, grid, i);
        __syncthreads();
        staged = true;
    };
    // mode 0: the fastest profile, 1: the slowest, 2: the blend alpha xf + (1 - alpha) xl
    auto duration = [&](int mode, double alpha) {
        for (int i = lane; i <= N; i += 64) {
            const double x = mode == 2 ? alpha * Lf[i] + (1 - alpha) * Ll[i] : (mode == 1 ? Ll[i] : Lf[i]);
            Ls[i] = sqrt(x);
        }
        __syncthreads();
        for (int i = lane; i < N; i += 64) Lt[i] = Ln[i] / (Ls[i + 1] + Ls[i] + 1e-9);
        __syncthreads();
        double t = 0;
#pragma unroll 8
        for (int i = 0; i < N; ++i) t += Lt[i];
        __syncthreads();  // (the next pass overwrites Ls / Lt)
        return t;
    };
    auto uni = [](bool c) { return __builtin_amdgcn_ballot_w64(c) != 0; };  // every lane holds the same value
    const double desired = A.desired[b];
    double dur, dur_slow;
    if (A.dur) { dur = A.dur[2 * (size_t)b]; dur_slow = A.dur[2 * (size_t)b + 1]; }
    else { stage(); dur = duration(0, 1.0); dur_slow = duration(1, 1.0); }
    double alpha = 0.0;
    if (uni(dur > desired)) alpha = 1.0;
    else if (uni(dur_slow < desired)) alpha = 0.0;
    else {
        if (!staged) stage();
        double alpha_low = 1.0, alpha_high = 0.0, diff = 10;
        while (uni(diff > A.atol)) {
            alpha = 0.5 * (alpha_low + alpha_high);
            if (uni(alpha == alpha_low || alpha == alpha_high)) break;  // interval exhausted (the reference would spin)
            const double da = duration(2, alpha);
            if (uni(da < desired)) { alpha_low = alpha; diff = desired - da; }
            else { alpha_high = alpha; diff = da - desired; }
        }
    }
    bool any_nan = false;
    for (int i = lane; i <= N; i += 64) {
        const double x = staged ? alpha * Lf[i] + (1 - alpha) * Ll[i] : alpha * xf[i] + (1 - alpha) * xl[i];
        const double sq = sqrt(x);
        any_nan |= isnan(sq);
        if (xs) xs[i] = x;
        if (sdv) sdv[i] = sq;
    }
    if (us) {
        const double *uf = A.uf + (size_t)b * N, *ul = A.ul + (size_t)b * N;
        for (int i = lane; i < N; i += 64) us[i] = alpha * uf[i] + (1 - alpha) * ul[i];
    }
    const bool bad = uni(any_nan);
    if (lane == 0) { if (A.alpha) A.alpha[b] = alpha; if (A.status) A.status[b] = bad ? TPR_STATUS_ERR_UNKNOWN : TPR_STATUS_OK; }
}

}  // namespace tpr

// tpr_spline.hip.inc -- batched cubic-spline fit: waypoints -> PPoly coefficient tables.
//
// Replaces SplineInterpolator.__init__ -> scipy.interpolate.CubicSpline (interpolator.py:419) for a
// batch of paths: one thread per (path, dof).  The arithmetic follows scipy's construction step by
// step -- slopes, the tridiagonal system for the knot derivatives with its boundary rows
// (scipy/interpolate/_cubic.py, CubicSpline.__init__), LAPACK dgtsv's elimination with partial
// pivoting (the not-a-knot rows are not diagonally dominant, so rows do get swapped), and
// CubicHermiteSpline's coefficient formulas -- so the tables agree with scipy's to the last bit on
// FMA-free LAPACK builds (checked in tests/test_gpu_spline.py; the stated bound is 1e-12 relative).
// Boundary conditions: not-a-knot, first derivative (clamped), second derivative (natural).  Splines of up to
// kSplineMaxPts points keep their working arrays in registers / scratch, longer ones (ParametrizeSpline fits
// N+1 points) in a coalesced global workspace.
// Included by tpr_kernels.hip.

namespace tpr {

constexpr int kSplineMaxPts = 64;

enum { kBcNotAKnot = 0, kBcFirst = 1, kBcSecond = 2 };

struct SplineArgs {
    int B, m, d;           // m waypoints
    int knots_per_path;    // knots [m] shared or [B][m]
    int bc0, bc1;          // boundary condition kinds
    const double *knots;
    const double *way;     // [B][m][d]
    const double *bcv0;    // [B][d] boundary values (kBcFirst / kBcSecond) or nullptr (= 0)
    const double *bcv1;
    double *coef;          // [B][4][m-1][d]
};

// Working arrays of one (path, dof) fit: registers / scratch for short splines, a global workspace laid
// out [array][point][thread] (coalesced across the threads of a wave) for long ones.
// kMax: compile-time bound on the number of points (0: none).  With a small bound every loop of the fit is unrolled and
// the arrays live in registers (round 3: the five-waypoint fit of the benchmark paths ran with 3 KB of scratch per lane).
template <int MAXP>
struct LocalArrays {
    static constexpr int kMax = MAXP;
    double a[6][MAXP];
    __device__ __forceinline__ double &at(int arr, int i) { return a[arr][i]; }
};
struct GlobalArrays {
    static constexpr int kMax = 0;
    double *base;      // + thread index
    size_t stride_i;   // threads
    size_t stride_arr; // points * threads
    __device__ __forceinline__ double &at(int arr, int i) { return base[(size_t)arr * stride_arr + (size_t)i * stride_i]; }
};
// loop "for (i = LO; i < HI; ++i)" whose trip count is bounded by W::kMax when that is a (small) compile-time constant
#define TPR_FIT_FOR(i, LO, HI) _Pragma("unroll") for (int i = (LO); i < ((W::kMax > 0 && W::kMax <= 16) ? W::kMax : (HI)); ++i) if (i < (HI))

// One cubic-spline fit (scipy CubicSpline + LAPACK dgtsv arithmetic, see the file header).
//   x: knots (stride 1), y: values (stride ys), n points, out: coefficient column (power block stride cs, segment stride os)
template <class W>
__device__ inline void spline_fit_one(W &w, const double *x, const double *y, size_t ys, int n, int bc0, int bc1, double v0,
                                      double v1, double *out, size_t cs, size_t os) {
    enum { DX = 0, SLOPE = 1, DL = 2, DG = 3, DU = 4, S = 5 };
    TPR_FIT_FOR(i, 0, n - 1) {
        w.at(DX, i) = x[i + 1] - x[i];
        w.at(SLOPE, i) = (y[(size_t)(i + 1) * ys] - y[(size_t)i * ys]) / w.at(DX, i);
    }
    if (n == 2) {  // scipy: not-a-knot on two points means "slope at both ends"
        if (bc0 == kBcNotAKnot) { bc0 = kBcFirst; v0 = w.at(SLOPE, 0); }
        if (bc1 == kBcNotAKnot) { bc1 = kBcFirst; v1 = w.at(SLOPE, 0); }
    }
    if (n == 3 && bc0 == kBcNotAKnot && bc1 == kBcNotAKnot) {
        // parabola through three points (scipy solves this 3x3 system with a dense LU)
        // [1 1 0; dx1 2(dx0+dx1) dx0; 0 1 1] s = [2 slope0; 3(dx0 slope1 + dx1 slope0); 2 slope1]
        const double dx0 = w.at(DX, 0), dx1 = w.at(DX, 1), sl0 = w.at(SLOPE, 0), sl1 = w.at(SLOPE, 1);
        const double b0 = 2 * sl0, b1 = 3 * (dx0 * sl1 + dx1 * sl0), b2 = 2 * sl1;
        const double a10 = dx1, a11 = 2 * (dx0 + dx1), a12 = dx0;
        // eliminate with s0 = b0 - s1, s2 = b2 - s1
        const double s1 = (b1 - a10 * b0 - a12 * b2) / (a11 - a10 - a12);
        w.at(S, 0) = b0 - s1; w.at(S, 1) = s1; w.at(S, 2) = b2 - s1;
    } else {
        // tridiagonal system for the knot derivatives: dl (sub), dg (diagonal), du (super), rhs s
        TPR_FIT_FOR(i, 1, n - 1) {
            w.at(DG, i) = 2 * (w.at(DX, i - 1) + w.at(DX, i));
            w.at(DU, i) = w.at(DX, i - 1);
            w.at(DL, i - 1) = w.at(DX, i);
            w.at(S, i) = 3 * (w.at(DX, i) * w.at(SLOPE, i - 1) + w.at(DX, i - 1) * w.at(SLOPE, i));
        }
        if (bc0 == kBcNotAKnot) {
            const double dd = x[2] - x[0], dx0 = w.at(DX, 0), dx1 = w.at(DX, 1);
            w.at(DG, 0) = dx1; w.at(DU, 0) = dd;
            w.at(S, 0) = ((dx0 + 2 * dd) * dx1 * w.at(SLOPE, 0) + dx0 * dx0 * w.at(SLOPE, 1)) / dd;
        } else if (bc0 == kBcFirst) {
            w.at(DG, 0) = 1; w.at(DU, 0) = 0; w.at(S, 0) = v0;
        } else {
            const double dx0 = w.at(DX, 0);
            w.at(DG, 0) = 2 * dx0; w.at(DU, 0) = dx0;
            w.at(S, 0) = -0.5 * v0 * (dx0 * dx0) + 3 * (y[ys] - y[0]);
        }
        if (bc1 == kBcNotAKnot) {
            const double dd = x[n - 1] - x[n - 3], dxa = w.at(DX, n - 2), dxb = w.at(DX, n - 3);
            w.at(DG, n - 1) = dxb; w.at(DL, n - 2) = dd;
            w.at(S, n - 1) = (dxa * dxa * w.at(SLOPE, n - 3) + (2 * dd + dxa) * dxb * w.at(SLOPE, n - 2)) / dd;
        } else if (bc1 == kBcFirst) {
            w.at(DG, n - 1) = 1; w.at(DL, n - 2) = 0; w.at(S, n - 1) = v1;
        } else {
            const double dxa = w.at(DX, n - 2);
            w.at(DG, n - 1) = 2 * dxa; w.at(DL, n - 2) = dxa;
            w.at(S, n - 1) = 0.5 * v1 * (dxa * dxa) + 3 * (y[(size_t)(n - 1) * ys] - y[(size_t)(n - 2) * ys]);
        }
        // LAPACK dgtsv: Gaussian elimination with partial pivoting, then back substitution
        TPR_FIT_FOR(i, 0, n - 1) {
            const bool last = i == n - 2;
            if (fabs(w.at(DG, i)) >= fabs(w.at(DL, i))) {
                if (w.at(DG, i) != 0.0) {
                    const double fact = w.at(DL, i) / w.at(DG, i);
                    w.at(DG, i + 1) = w.at(DG, i + 1) - fact * w.at(DU, i);
                    w.at(S, i + 1) = w.at(S, i + 1) - fact * w.at(S, i);
                }
                if (!last) w.at(DL, i) = 0.0;
            } else {
                const double fact = w.at(DG, i) / w.at(DL, i);
                w.at(DG, i) = w.at(DL, i);
                double temp = w.at(DG, i + 1);
                w.at(DG, i + 1) = w.at(DU, i) - fact * temp;
                if (!last) {
                    w.at(DL, i) = w.at(DU, i + 1);
                    w.at(DU, i + 1) = -fact * w.at(DL, i);
                }
                w.at(DU, i) = temp;
                temp = w.at(S, i);
                w.at(S, i) = w.at(S, i + 1);
                w.at(S, i + 1) = temp - fact * w.at(S, i + 1);
            }
        }
        w.at(S, n - 1) = w.at(S, n - 1) / w.at(DG, n - 1);
        if (n > 1) w.at(S, n - 2) = (w.at(S, n - 2) - w.at(DU, n - 2) * w.at(S, n - 1)) / w.at(DG, n - 2);
        if (W::kMax > 0 && W::kMax <= 16) {
#pragma unroll
            for (int i = W::kMax - 3; i >= 0; --i)
                if (i <= n - 3) w.at(S, i) = (w.at(S, i) - w.at(DU, i) * w.at(S, i + 1) - w.at(DL, i) * w.at(S, i + 2)) / w.at(DG, i);
        } else {
            for (int i = n - 3; i >= 0; --i)
                w.at(S, i) = (w.at(S, i) - w.at(DU, i) * w.at(S, i + 1) - w.at(DL, i) * w.at(S, i + 2)) / w.at(DG, i);
        }
    }
    // CubicHermiteSpline: t = (s_i + s_{i+1} - 2 slope)/dx; c0 = t/dx; c1 = (slope - s_i)/dx - t
    TPR_FIT_FOR(i, 0, n - 1) {
        const double dxi = w.at(DX, i), sl = w.at(SLOPE, i), si = w.at(S, i);
        const double t = (si + w.at(S, i + 1) - 2 * sl) / dxi;
        out[0 * cs + (size_t)i * os] = t / dxi;
        out[1 * cs + (size_t)i * os] = (sl - si) / dxi - t;
        out[2 * cs + (size_t)i * os] = si;
        out[3 * cs + (size_t)i * os] = y[(size_t)i * ys];
    }
}

// counts (optional, [B]): points of each path actually used (ragged batches: ParametrizeSpline drops
// gridpoints it reaches in no time); segments beyond a path's last one are filled with its last value
// (a constant extension) so that the tables stay rectangular.
// STORE: 0 = working arrays in a coalesced global workspace (any number of points), 8 / 64 = in registers / scratch for
// up to that many points
template <int STORE>
__global__ void __launch_bounds__(128) spline_fit_kernel(SplineArgs A, const int32_t *counts, double *workspace) {
    constexpr bool BIG = STORE == 0;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)A.B * A.d;
    if (gid >= total) return;
    const int b = (int)(gid / A.d), k = (int)(gid % A.d);
    const int nmax = A.m;
    const int n = counts ? counts[b] : nmax;
    const double *x = A.knots + (A.knots_per_path ? (size_t)b * nmax : 0);
    const double *y = A.way + (size_t)b * nmax * A.d + k;  // stride d
    double *out = A.coef + (size_t)b * 4 * (nmax - 1) * A.d + k;
    const size_t cs = (size_t)(nmax - 1) * A.d;  // stride between power blocks
    const double v0 = A.bcv0 ? A.bcv0[(size_t)b * A.d + k] : 0.0, v1 = A.bcv1 ? A.bcv1[(size_t)b * A.d + k] : 0.0;
    if (n >= 2) {
        if (BIG) {
            GlobalArrays w{workspace + gid, (size_t)total, (size_t)nmax * (size_t)total};
            spline_fit_one(w, x, y, (size_t)A.d, n, A.bc0, A.bc1, v0, v1, out, cs, (size_t)A.d);
        } else {
            LocalArrays<BIG ? 1 : STORE> w;
            spline_fit_one(w, x, y, (size_t)A.d, n, A.bc0, A.bc1, v0, v1, out, cs, (size_t)A.d);
        }
    }
    for (int i = (n >= 2 ? n - 1 : 0); i < nmax - 1; ++i) {
        out[0 * cs + (size_t)i * A.d] = 0.0; out[1 * cs + (size_t)i * A.d] = 0.0; out[2 * cs + (size_t)i * A.d] = 0.0;
        out[3 * cs + (size_t)i * A.d] = y[(size_t)(n >= 1 ? n - 1 : 0) * A.d];
    }
}

// ---- ParametrizeSpline (toppra/parametrizer.py:161-196) for B trajectories ---------------------------
struct ParamSplineArgs {
    int B, N, d, nseg, flags;
    const double *coef, *breaks, *grid, *sd;
    double *tk;        // [B][N+1] knot times, compacted, padded with the last time + 1, + 2, ...
    double *way;       // [B][N+1][d] q(s) at the kept gridpoints, padded with the last point
    double *bcv0, *bcv1;  // [B][d] q'(s_0) sd_0, q'(s_N) sd_N
    int32_t *counts;   // [B] kept gridpoints
};

// The same for a path given as samples at the gridpoints (tpr_param_spline_samples_batch): coef / breaks stay null.
struct ParamSamplesArgs : ParamSplineArgs {
    const double *q, *qs;  // [B][N+1][d]: path(grid), path(grid, 1)
};

// q(s) in scipy's power-basis order (PPoly.__call__)
__device__ __forceinline__ double cubic_d0(double c0, double c1, double c2, double c3, double x) {
    return ((c3 + c2 * x) + c1 * (x * x)) + c0 * ((x * x) * x);
}

// One thread per trajectory: the time stamps of :176-186 (a sequential sum; a gridpoint reached in less
// than TINY seconds is dropped), then the waypoints and the clamped-end derivatives.
// Args = ParamSamplesArgs: the kept samples are copied where the cubic is evaluated, the end derivatives are the samples'.
template <class Args>
__global__ void __launch_bounds__(64) param_spline_knots_kernel(Args A) {
    constexpr bool kSampled = std::is_same<Args, ParamSamplesArgs>::value;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= A.B) return;
    const int N = A.N, d = A.d, nseg = A.nseg;
    const double *ss = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)b * (N + 1) : 0);
    const double *v = A.sd + (size_t)b * (N + 1);
    const double *breaks = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? (size_t)b * (nseg + 1) : 0);
    const double *cf = A.coef + (size_t)b * 4 * nseg * d;
    double *tk = A.tk + (size_t)b * (N + 1);
    double *way = A.way + (size_t)b * (N + 1) * d;
    auto put = [&](int slot, int i) {
        if constexpr (kSampled) {
            for (int k = 0; k < d; ++k) way[(size_t)slot * d + k] = A.q[((size_t)b * (N + 1) + i) * d + k];
            return;
        }
        const double s = ss[i];
        const int j = find_segment(breaks, nseg, s);
        const double x = s - breaks[j];
        for (int k = 0; k < d; ++k)
            way[(size_t)slot * d + k] = cubic_d0(cf[(0 * nseg + j) * d + k], cf[(1 * nseg + j) * d + k],
                                                 cf[(2 * nseg + j) * d + k], cf[(3 * nseg + j) * d + k], x);
    };
    int cnt = 1;
    double t = 0.0;
    tk[0] = 0.0;
    put(0, 0);
    for (int i = 1; i <= N; ++i) {
        const double sd_avg = (v[i - 1] + v[i]) / 2;
        // (a trajectory that could not be parameterized has NaN velocities: its time stamps -- and with them its
        // duration -- are NaN from there on, instead of the "standing stretch" 5 s the comparison would fall into)
        const double delta_t = isnan(sd_avg) ? qnan() : (sd_avg > kPyTiny ? (ss[i] - ss[i - 1]) / sd_avg : 5.0);
        t = t + delta_t;
        if (delta_t < kPyTiny) continue;  // np.delete(t_grid, skip): the running time keeps the skipped step
        tk[cnt] = t;
        put(cnt, i);
        cnt += 1;
    }
    for (int i = cnt; i <= N; ++i) {  // rectangular padding (never evaluated: counts says so)
        tk[i] = tk[i - 1] + 1.0;
        for (int k = 0; k < d; ++k) way[(size_t)i * d + k] = way[(size_t)(cnt - 1) * d + k];
    }
    A.counts[b] = cnt;
    // clamped ends: path(path_interval[0/1], 1) * velocities[0/-1]; the path interval is the spline's own
    if constexpr (kSampled) {  // (the gridpoints span the path interval)
        for (int k = 0; k < d; ++k) {
            A.bcv0[(size_t)b * d + k] = A.qs[(size_t)b * (N + 1) * d + k] * v[0];
            A.bcv1[(size_t)b * d + k] = A.qs[((size_t)b * (N + 1) + N) * d + k] * v[N];
        }
        return;
    }
    const double s0 = breaks[0], s1 = breaks[nseg];
    for (int e = 0; e < 2; ++e) {
        const double s = e ? s1 : s0;
        const int j = find_segment(breaks, nseg, s);
        const double x = s - breaks[j];
        double *dst = (e ? A.bcv1 : A.bcv0) + (size_t)b * d;
        for (int k = 0; k < d; ++k) {
            double q1, q2;
            cubic_d1_d2(cf[(0 * nseg + j) * d + k], cf[(1 * nseg + j) * d + k], cf[(2 * nseg + j) * d + k], x, q1, q2);
            dst[k] = q1 * (e ? v[N] : v[0]);
        }
    }
}

// ---- ParametrizeSpline in ONE kernel (d <= 64) ---------------------------------------------------------
// The two kernels above cost 10.4 ms at 65536 x 7 x 200 (profiles/r03_secondary_before_*: 12 GB + 19 GB of HBM traffic
// against 3.2 GB of algorithmic bytes -- one thread per trajectory writing waypoints with stride d, then six working
// arrays per fit through a global workspace).  What the computation needs is much less:
//   * the d fits of a trajectory share their knots, hence their tridiagonal MATRIX: dgtsv's pivoting decisions and
//     multipliers depend on the knot times only.  Every lane eliminates the matrix in registers alongside its own
//     right-hand side (SIMD: the redundancy is free) -- row i+1 is built from knots i .. i+2 as the elimination
//     reaches it, so DX, SLOPE, the sub-diagonal and the initial right-hand side are never stored;
//   * back substitution needs the eliminated rows in reverse: three doubles per knot per TRAJECTORY and the eliminated
//     right-hand side, one double per knot per (trajectory, dof), stored [task][knot][lane] -- 512 contiguous bytes
//     per wave store.  Both are read back within a millisecond of being written: they come from the caches;
//   * the coefficient rows of a tile of T segments are computed lane-parallel from the tile's knot slopes (LDS) with
//     consecutive lanes on consecutive table entries: every store of the 2.9 GB output is 512 contiguous bytes.
// A wave owns min(16, floor(64/d)) whole trajectories (lane = tl * d + k); a block is one wave.
//
// The three sequential passes (time stamps, elimination, back substitution) are software-pipelined by hand so that no
// step of a pass waits for memory.  gfx950 counts loads and stores in ONE in-order counter, so a wait for a
// prefetched value is a wait for every store issued before it: each pass therefore moves whole tiles -- the stores
// of tile t-1 and the loads of tile t+1 are issued together at the top of tile t's arithmetic, and the single wait
// at its end finds them done.  Per-trajectory values travel through LDS (loaded once, read by the trajectory's d
// lanes); the path segment under the running knot is tracked in registers (reloaded when the knot crosses a breakpoint).
// Arithmetic: the same expressions, in the same order, as param_spline_knots_kernel + spline_fit_one with clamped
// ends (tests/test_gpu_param.py compares the two bit for bit, ragged knot counts and row exchanges included).
constexpr int kPsTile = 8;
constexpr int kPsMaxTpw = 16;   // bounds the per-lane share of a tile's per-trajectory loads
#ifndef TPR_PS_WAVES
#define TPR_PS_WAVES 2   // waves per SIMD the register allocation aims at (3 spills: slower)
#endif

struct ParamFusedArgs {
    ParamSplineArgs K;
    double *coef_t;     // [B][4][N][d]
    double *rhs;        // [tasks][N+1][64] eliminated right-hand sides
    double *rows;       // [tasks][N+1][3][tpw] eliminated matrix rows: diagonal, first and second super-diagonal
    double *sk;         // [B][N+1] path position of each knot
    int tpw;            // trajectories per wave
};

// The path segment holding s (find_segment's answer) with its coefficients of dof k in registers.  Gridpoints ascend
// (the algorithm's precondition; reachability_algorithm.py refuses anything else) and so do breakpoints, hence a pass
// that walks the knots UP only ever leaves a segment through its upper end, one that walks DOWN through its lower
// end: one comparison per knot against a bound that is +-inf on the end segments.
struct SegTrack {
    int g;
    double lo, up, dn, c0, c1, c2, c3;   // x = s - lo; leave upward when s >= up, downward when !(s >= dn)
    __device__ __forceinline__ void load(const double *breaks, int nseg, const double *cf, int d, int g_) {
        g = g_; lo = breaks[g];
        up = g < nseg - 1 ? breaks[g + 1] : __longlong_as_double(0x7ff0000000000000LL);
        dn = g > 0 ? lo : -__longlong_as_double(0x7ff0000000000000LL);
        c0 = cf[(0 * nseg + g) * d]; c1 = cf[(1 * nseg + g) * d]; c2 = cf[(2 * nseg + g) * d]; c3 = cf[(3 * nseg + g) * d];
    }
    template <bool UP>
    __device__ __forceinline__ double at(const double *breaks, int nseg, const double *cf, int d, double s) {
        if (UP ? (s >= up) : (s < dn)) {
            int g2 = g;
            if (UP) { g2 = g + 1; while (g2 < nseg - 1 && s >= breaks[g2 + 1]) ++g2; }
            else { g2 = g - 1; while (g2 > 0 && !(s >= breaks[g2])) --g2; }
            load(breaks, nseg, cf, d, g2);
        }
        return cubic_d0(c0, c1, c2, c3, s - lo);
    }
};

// floor(x / p) for x < 2^32 / p from inv = recip_u32(p): one multiply
__device__ __forceinline__ unsigned recip_u32(unsigned p) { return p == 1 ? 0u : (unsigned)(0x100000000ULL / p) + 1u; }
__device__ __forceinline__ int div_u32(int x, unsigned inv) { return inv ? (int)__umulhi((unsigned)x, inv) : x; }
// every outstanding load has landed, every outstanding store has left (vmcnt = 0; the other counters untouched)
__device__ __forceinline__ void wait_vmem() { __builtin_amdgcn_s_waitcnt(0x0F70); }
// Lanes of ONE wave exchanging values through LDS: the wave's LDS instructions execute in program order, so all it
// takes is that the earlier ones have completed (lgkmcnt = 0) and that the compiler keeps the order.  __syncthreads()
// would also drain the vector-memory counter -- every store and prefetch in flight -- which is exactly what the tile
// pipelines below are built to avoid; it is used only between the passes, where lanes do exchange data through global
// memory.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (no instruction at this scope: the order of the LDS accesses, stated)
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int T>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(TPR_PS_WAVES))) param_spline_fused_kernel(ParamFusedArgs A) {
    constexpr int kCoop = ((T + 1) * 3 * kPsMaxTpw + 63) / 64;  // doubles per lane of a tile's cooperative loads: rows,
    constexpr int kCoopK = ((T + 1) * kPsMaxTpw + 63) / 64;     // knots,
    constexpr int kCoop1 = T + 1;                               // pass 1's steps: tpw * TS <= (T + 1) * 64
    extern __shared__ double ps_lds[];
    const int lane = threadIdx.x;
    const int N = A.K.N, d = A.K.d, nseg = A.K.nseg, tpw = A.tpw;
    double *sS = ps_lds;                   // [T+1][64] knot slopes of the tile          (pass 1: step durations)
    double *sY = sS + (T + 1) * 64;        // [T+1][64] waypoints of the tile            (pass 1: gridpoints)
    double *sYl = sY + (T + 1) * 64;       // [64] last waypoint (constant extension)
    double *sX = sYl + 64;                 // [T+1][tpw] knot times of the tile being written out
    double *sK = sX + (T + 1) * tpw;       // [T+1][tpw] path positions of the tile's knots
    double *sM = sK + (T + 1) * tpw;       // [T+1][3][tpw] eliminated rows of the tile (global layout)
    int *sN = reinterpret_cast<int *>(sM + (T + 1) * 3 * tpw);  // [tpw] knots per trajectory
    const int tl = lane / d, k = lane - tl * d;
    const long long b0 = (long long)blockIdx.x * tpw;
    const long long b = b0 + tl;
    const int ntraj = A.K.B - b0 < tpw ? (int)(A.K.B - b0) : tpw;   // trajectories of this wave
    const bool act = tl < ntraj;
    const size_t bb = act ? (size_t)b : (size_t)b0;
    const bool lead = act & (k == 0);
    const bool per_grid = (A.K.flags & TPR_GRID_PER_TRAJ) != 0;
    const double *__restrict__ ss = A.K.grid + (per_grid ? bb * (N + 1) : 0);
    const double *__restrict__ v = A.K.sd + bb * (N + 1);
    const double *__restrict__ breaks = A.K.breaks + ((A.K.flags & TPR_BREAKS_PER_TRAJ) ? bb * (nseg + 1) : 0);
    const double *__restrict__ cf = A.K.coef + bb * 4 * nseg * d + (act ? k : 0);
    double *__restrict__ tk = A.K.tk + bb * (N + 1);
    double *__restrict__ sk = A.sk + bb * (N + 1);
    const size_t rstride = (size_t)3 * tpw;
    double *__restrict__ rows0 = A.rows + (size_t)blockIdx.x * (N + 1) * rstride;  // this task's rows
    double *__restrict__ rows = rows0 + (act ? tl : 0);
    double *__restrict__ rhs = A.rhs + (size_t)blockIdx.x * (N + 1) * 64 + lane;
    const size_t cs = (size_t)N * d;  // stride between power blocks
    const unsigned inv_d = recip_u32(d), inv_tpw = recip_u32(tpw);

    // (1) time stamps (parametrizer.py:176-186).  The step durations of TS gridpoints x all trajectories are computed
    // lane-parallel (coalesced reads of the velocity rows); the running sum -- sequential by definition -- is left to
    // one lane per trajectory, from LDS.
    int n = 1;
    {
        const int TS = (T + 1) * 64 / tpw < 64 ? (T + 1) * 64 / tpw : 64;
        double *dT = sS, *gS = sY;  // [tpw][TS]
        double t = 0.0, t_kept = 0.0;
        if (lead) { tk[0] = 0.0; sk[0] = ss[0]; }
        for (int i0 = 0; i0 < N; i0 += TS) {  // steps i0+1 .. i0+cnt
            const int cnt = N - i0 < TS ? N - i0 : TS;
            const unsigned inv_cnt = recip_u32(cnt);
            double va[kCoop1], vb[kCoop1], ga[kCoop1], gb[kCoop1];  // all of the tile's loads first, then its divisions
#pragma unroll
            for (int r = 0; r < kCoop1; ++r) {
                const int idx = r * 64 + lane;
                if (idx < ntraj * cnt) {
                    const int t2 = div_u32(idx, inv_cnt), i = i0 + idx - t2 * cnt + 1;
                    const double *v2 = A.K.sd + (size_t)(b0 + t2) * (N + 1), *g2 = A.K.grid + (per_grid ? (size_t)(b0 + t2) * (N + 1) : 0);
                    va[r] = v2[i - 1]; vb[r] = v2[i]; ga[r] = g2[i - 1]; gb[r] = g2[i];
                }
            }
#pragma unroll
            for (int r = 0; r < kCoop1; ++r) {
                const int idx = r * 64 + lane;
                if (idx < ntraj * cnt) {
                    const int t2 = div_u32(idx, inv_cnt), u = idx - t2 * cnt;
                    const double sd_avg = (va[r] + vb[r]) / 2;
                    dT[t2 * TS + u] = isnan(sd_avg) ? qnan() : (sd_avg > kPyTiny ? (gb[r] - ga[r]) / sd_avg : 5.0);
                    gS[t2 * TS + u] = gb[r];
                }
            }
            wave_lds_sync();
            if (lead) {
                for (int u = 0; u < cnt; ++u) {
                    const double delta_t = dT[tl * TS + u];
                    t = t + delta_t;
                    if (delta_t < kPyTiny) continue;  // np.delete(t_grid, skip): the running time keeps the skipped step
                    tk[n] = t; sk[n] = gS[tl * TS + u];
                    t_kept = t;
                    n += 1;
                }
            }
            wave_lds_sync();
        }
        if (lead) {
            const double s_last = ss[N];
            for (int i = n; i <= N; ++i) { t_kept = t_kept + 1.0; tk[i] = t_kept; sk[i] = s_last; }  // rectangular padding
            A.K.counts[b] = n;
            sN[tl] = n;
        }
    }
    __syncthreads();
    int nmax = 1;
    for (int t2 = 0; t2 < ntraj; ++t2) nmax = sN[t2] > nmax ? sN[t2] : nmax;
    if (act) n = sN[tl];
    SegTrack seg;
    seg.load(breaks, nseg, cf, d, find_segment(breaks, nseg, A.sk[bb * (N + 1)]));

    // (2) rows of the clamped system, built as LAPACK dgtsv's elimination reaches them (spline_fit_one above).
    // Tile = T elimination steps i0 .. i0+T-1, which need the knots i0+2 .. i0+T+1 (sX / sK here: [T][tpw]).
    {
        double bc[2] = {0.0, 0.0};
        double xb = 0.0, yb = 0.0, dx_i = 0.0, sl_i = 0.0, dg = 1.0, du = 0.0, s = 0.0;
        const bool run = act & (n >= 2);
        if (run) {
            for (int e = 0; e < 2; ++e) {  // q'(path end) * velocity: parametrizer.py:189-194
                const double se = e ? breaks[nseg] : breaks[0];
                const int g = find_segment(breaks, nseg, se);
                double q1, q2;
                cubic_d1_d2(cf[(0 * nseg + g) * d], cf[(1 * nseg + g) * d], cf[(2 * nseg + g) * d], se - breaks[g], q1, q2);
                bc[e] = q1 * (e ? v[N] : v[0]);
            }
            const double y_first = seg.at<true>(breaks, nseg, cf, d, sk[0]);
            xb = tk[1]; yb = seg.at<true>(breaks, nseg, cf, d, sk[1]);
            dx_i = xb - tk[0];             // DX(i), SLOPE(i)
            sl_i = (yb - y_first) / dx_i;
            s = bc[0];                     // (dg, du, s): row i as eliminated so far
        }
        double nx[kCoopK], ns[kCoopK];    // a tile's knots in flight: lane's share of [tpw][T]
        auto fetch_knots = [&](int i0) {
#pragma unroll
            for (int r = 0; r < kCoopK; ++r) {
                const int idx = r * 64 + lane;
                if (idx < ntraj * T) {
                    const int t2 = idx / T, u = idx - t2 * T;
                    const int j = i0 + u + 2 < N ? i0 + u + 2 : N;
                    nx[r] = A.K.tk[(size_t)(b0 + t2) * (N + 1) + j]; ns[r] = A.sk[(size_t)(b0 + t2) * (N + 1) + j];
                }
            }
        };
        auto land_knots = [&]() {
#pragma unroll
            for (int r = 0; r < kCoopK; ++r) {
                const int idx = r * 64 + lane;
                if (idx < ntraj * T) {
                    const int t2 = idx / T, u = idx - t2 * T;
                    sX[u * tpw + t2] = nx[r]; sK[u * tpw + t2] = ns[r];
                }
            }
        };
        fetch_knots(0);
        wait_vmem();
        land_knots();
        wave_lds_sync();
        double outr[T];   // the tile's eliminated right-hand sides, stored at the top of the next tile
        int prev_i0 = -1;
        auto flush = [&](int p0) {  // global stores of tile p0: right-hand sides from registers, rows from LDS
#pragma unroll
            for (int u = 0; u < T; ++u) {
                const int i = p0 + u;
                if (run & (i <= n - 2)) {
                    rhs[(size_t)i * 64] = outr[u];
                    if (lead) {
                        rows[i * rstride] = sM[(u * 3 + 0) * tpw + tl];
                        rows[i * rstride + tpw] = sM[(u * 3 + 1) * tpw + tl];
                        rows[i * rstride + 2 * tpw] = sM[(u * 3 + 2) * tpw + tl];
                    }
                }
            }
        };
        for (int i0 = 0; i0 <= nmax - 2; i0 += T) {
            if (prev_i0 >= 0) flush(prev_i0);
            const bool more = i0 + T <= nmax - 2;
            if (more) fetch_knots(i0 + T);
#pragma unroll
            for (int u = 0; u < T; ++u) {
                const int i = i0 + u;
                if (run & (i <= n - 2)) {
                    const bool last = i == n - 2;
                    double dx_n = 0.0, sl_n = 0.0, xc = xb, yc = yb;
                    double dg1 = 1.0, du1 = 0.0, dl = 0.0, s1 = bc[1];  // row i+1 and the sub-diagonal entry under row i
                    if (!last) {
                        xc = sX[u * tpw + tl]; yc = seg.at<true>(breaks, nseg, cf, d, sK[u * tpw + tl]);
                        dx_n = xc - xb; sl_n = (yc - yb) / dx_n;
                        dg1 = 2 * (dx_i + dx_n); du1 = dx_i; dl = dx_n;
                        s1 = 3 * (dx_n * sl_i + dx_i * sl_n);
                    }
                    double dl2 = 0.0;  // second super-diagonal of row i (a row exchange fills it)
                    if (fabs(dg) >= fabs(dl)) {
                        if (dg != 0.0) {
                            const double fact = dl / dg;
                            dg1 = dg1 - fact * du;
                            s1 = s1 - fact * s;
                        }
                    } else {
                        const double fact = dg / dl;
                        dg = dl;
                        const double temp = dg1;
                        dg1 = du - fact * temp;
                        if (!last) { dl2 = du1; du1 = -fact * dl2; }
                        du = temp;
                        const double s_old = s, s1_old = s1;
                        s = s1_old;
                        s1 = s_old - fact * s1_old;
                    }
                    if (lead) { sM[(u * 3 + 0) * tpw + tl] = dg; sM[(u * 3 + 1) * tpw + tl] = du; sM[(u * 3 + 2) * tpw + tl] = dl2; }
                    outr[u] = s;
                    dg = dg1; du = du1; s = s1; dx_i = dx_n; sl_i = sl_n; xb = xc; yb = yc;
                }
            }
            wait_vmem();
            wave_lds_sync();
            if (more) land_knots();
            wave_lds_sync();
            prev_i0 = i0;
        }
        if (prev_i0 >= 0) flush(prev_i0);
        if (run) {
            if (lead) { rows[(n - 1) * rstride] = dg; rows[(n - 1) * rstride + tpw] = 0.0; rows[(n - 1) * rstride + 2 * tpw] = 0.0; }
            rhs[(size_t)(n - 1) * 64] = s;
        }
    }
    __syncthreads();

    // (3) back substitution, a tile of T segments at a time from the top; the tile's coefficient rows
    // (CubicHermiteSpline's formulas) are computed lane-parallel over (trajectory, segment, dof) in the table's own
    // order, ONE TILE BEHIND: the stores of tile t+1 and the loads of tile t-1 surround the arithmetic of tile t.
    double s1 = 0.0, s2 = 0.0, y1 = 0.0;
    if (act) {
        seg.load(breaks, nseg, cf, d, find_segment(breaks, nseg, sk[n - 1]));
        y1 = seg.at<false>(breaks, nseg, cf, d, sk[n - 1]);
        sYl[lane] = y1;
        if (n >= 2) s1 = rhs[(size_t)(n - 1) * 64] / rows[(n - 1) * rstride];
    }
    double rq[T], rqn[T], cm[kCoop], cx[kCoopK], ck[kCoopK];
    const int row_cnt = (T + 1) * 3 * tpw, kn_cnt = (T + 1) * ntraj;
    const unsigned inv_rs = recip_u32(3 * tpw), inv_full = recip_u32(T * d);
    auto fetch_tile = [&](int i0) {   // tile i0: rows + path positions of knots i0 .. i0+T, right-hand sides i0 .. i0+T-1
#pragma unroll
        for (int u = 0; u < T; ++u) rqn[u] = rhs[(size_t)(i0 + u < N ? i0 + u : N) * 64];
#pragma unroll
        for (int r = 0; r < kCoop; ++r) {
            const int idx = r * 64 + lane;
            if (idx < row_cnt) {
                const int u = div_u32(idx, inv_rs);
                cm[r] = rows0[(size_t)(i0 + u <= N ? idx + (size_t)i0 * rstride : idx - u * rstride + N * rstride)];
            }
        }
#pragma unroll
        for (int r = 0; r < kCoopK; ++r) {
            const int idx = r * 64 + lane;
            if (idx < kn_cnt) {
                const int t2 = idx / (T + 1), u = idx - t2 * (T + 1);
                ck[r] = A.sk[(size_t)(b0 + t2) * (N + 1) + (i0 + u < N ? i0 + u : N)];
            }
        }
    };
    auto fetch_times = [&](int i0) {  // knot times i0 .. i0+T
#pragma unroll
        for (int r = 0; r < kCoopK; ++r) {
            const int idx = r * 64 + lane;
            if (idx < kn_cnt) {
                const int t2 = idx / (T + 1), u = idx - t2 * (T + 1);
                cx[r] = A.K.tk[(size_t)(b0 + t2) * (N + 1) + (i0 + u < N ? i0 + u : N)];
            }
        }
    };
    auto land_tile = [&]() {
#pragma unroll
        for (int u = 0; u < T; ++u) rq[u] = rqn[u];
#pragma unroll
        for (int r = 0; r < kCoop; ++r) {
            const int idx = r * 64 + lane;
            if (idx < row_cnt) sM[idx] = cm[r];
        }
#pragma unroll
        for (int r = 0; r < kCoopK; ++r) {
            const int idx = r * 64 + lane;
            if (idx < kn_cnt) { const int t2 = idx / (T + 1), u = idx - t2 * (T + 1); sK[u * tpw + t2] = ck[r]; }
        }
    };
    auto land_times = [&]() {
#pragma unroll
        for (int r = 0; r < kCoopK; ++r) {
            const int idx = r * 64 + lane;
            if (idx < kn_cnt) { const int t2 = idx / (T + 1), u = idx - t2 * (T + 1); sX[u * tpw + t2] = cx[r]; }
        }
    };
    auto write_out = [&](int i0) {   // coefficient rows of tile i0 from sS / sY / sX
        const int segs = N - i0 < T ? N - i0 : T;     // segments of this tile inside the table
        const int per_traj = segs * d, total = per_traj * ntraj;
        const unsigned inv_pt = segs == T ? inv_full : recip_u32(per_traj);
        for (int idx = lane; idx < total; idx += 64) {
            const int t2 = div_u32(idx, inv_pt);
            const int item = idx - t2 * per_traj;
            const int jj = div_u32(item, inv_d), k2 = item - jj * d;
            const int i = i0 + jj, l2 = t2 * d + k2, n2 = sN[t2];
            double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = sYl[l2];
            if (i <= n2 - 2) {
                const double dxi = sX[(jj + 1) * tpw + t2] - sX[jj * tpw + t2];
                const double si = sS[jj * 64 + l2], sn = sS[(jj + 1) * 64 + l2];
                const double y0 = sY[jj * 64 + l2], sl = (sY[(jj + 1) * 64 + l2] - y0) / dxi;
                const double t = (si + sn - 2 * sl) / dxi;
                c0 = t / dxi; c1 = (sl - si) / dxi - t; c2 = si; c3 = y0;
            }
            double *o = A.coef_t + (size_t)(b0 + t2) * 4 * cs + (size_t)i0 * d + item;
            o[0] = c0; o[cs] = c1; o[2 * cs] = c2; o[3 * cs] = c3;
        }
    };
    const int top = ((N - 1) / T) * T;
    fetch_tile(top);
    wait_vmem();
    land_tile();
    wave_lds_sync();
    for (int i0 = top; i0 >= 0; i0 -= T) {
        if (i0 >= T) fetch_tile(i0 - T);
        fetch_times(i0);
        if (i0 < top) write_out(i0 + T);
        wave_lds_sync();
#pragma unroll
        for (int u = T - 1; u >= 0; --u) {
            const int i = i0 + u;
            if (act & (i <= n - 2)) {
                if ((u == T - 1) | (i == n - 2)) { sS[(u + 1) * 64 + lane] = s1; sY[(u + 1) * 64 + lane] = y1; }
                double num = rq[u] - sM[(u * 3 + 1) * tpw + tl] * s1;
                if (i < n - 2) num = num - sM[(u * 3 + 2) * tpw + tl] * s2;
                const double si = num / sM[(u * 3 + 0) * tpw + tl];
                const double y0 = seg.at<false>(breaks, nseg, cf, d, sK[u * tpw + tl]);
                sS[u * 64 + lane] = si; sY[u * 64 + lane] = y0;
                s2 = s1; s1 = si; y1 = y0;
            }
        }
        wait_vmem();
        wave_lds_sync();
        if (i0 >= T) land_tile();
        land_times();
        wave_lds_sync();
    }
    write_out(0);
}

// ---- ParametrizeSpline, parallel in the knots (d <= 16, N + 1 knots in LDS: the default where it fits) ------------------
// The fused kernel above reproduces LAPACK's elimination order, and with it LAPACK's 3 x N dependent steps per fit: at the
// headline shape 0.8 of its 1.9 ms are the two sequential passes, and the eliminated right-hand sides wait in HBM for the
// back substitution (profiles/r03: 5.2 GB moved for 3.2 GB of results).  The system is strictly diagonally dominant by
// rows -- 2 (dx_{i-1} + dx_i) on the diagonal against dx_i and dx_{i-1} beside it, the clamped ends are identity rows --
// so it needs no pivoting and parallel cyclic reduction solves it stably in ceil(log2 n) steps: at step s every row i
// eliminates its couplings to i - s and i + s with rows i - s and i + s, after the last step each row reads b_i m_i = r_i.
// One block per trajectory, one thread per knot (KPT knots per thread beyond 256), the d right-hand sides of a knot in the
// thread's registers, neighbours' rows through LDS; the matrix part of a step is shared by the d fits.  Nothing but the
// results goes to HBM: knot times, counts and the [4][N][d] table (consecutive lanes on consecutive table entries).
// Bit-identical to the other variants: knot times (the reference's sequential sum, parametrizer.py:176-186 -- one thread
// adds, from LDS; which gridpoints survive is a parallel count), counts, waypoints.  Equal to rounding: the knot derivatives
// (another elimination order; divisions by a step or a pivot are products with a reciprocal refined to the last bit or
// two) and with them the table: tests/test_gpu_param.py bounds the evaluated q, dq/dt, d2q/dt2 against the LAPACK-order
// kernel (variant 2) and checks the reference's own samples with that row's tolerance (1e-10).
__device__ __forceinline__ double rcp_refined(double x) {  // 1 / x to ~1 ulp: v_rcp_f64 + two Newton steps
    double r = __builtin_amdgcn_rcp(x);
    r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
    return __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
}

// wave_lds_sync() that also keeps the COMPILER from moving LDS accesses across it (a wavefront-scope fence emits nothing)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    wave_lds_sync();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// SAMPLE: instead of the [4][N][d] table, q / dq/dt / d2q/dt2 at T times per trajectory (ParamSampleArgs) -- what a caller of
// compute_trajectory() does next (traj(ts), traj(ts, 1), traj(ts, 2): examples/plot_kinematics.py:52-57) -- straight from
// the knot derivatives in LDS: the 2.9 GB table of the headline batch is neither written nor read back.  The coefficients of
// a sample's segment and the evaluation are the expressions of the table pass and of ppoly_eval_kernel: the same bits as
// table + evaluation.
struct ParamSampleArgs {
    int T, fractions;        // times are fractions of the trajectory's duration (linspace(0, 1, T) * duration) or absolute
    const double *times;     // [B][T], or [T] shared (fractions only)
    int times_per_traj;
    double *q[3];            // [B][T][d] per order, nullptr = not wanted
    double *duration;        // [B] or nullptr
};

template <int D, int KPT, bool SAMPLE = false>
__global__ void __launch_bounds__(256) param_spline_pcr_kernel(ParamSplineArgs A, double *__restrict__ coef_t,
                                                               ParamSampleArgs Q = ParamSampleArgs{}) {
    extern __shared__ double pcr_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = A.N, nseg = A.nseg, NS = N + 1;
    const int NP = NS | 1;             // odd stride of the [dof][knot] arrays: consecutive dofs of a knot on different banks
    const size_t b = blockIdx.x;
    // 1 + D + max(D - 1, 2) columns of NP doubles: 22.5 KB at 7 dof and 200 gridpoints, seven blocks per CU
    constexpr int XC = SAMPLE ? (D > 2 ? D : 2) : (D - 1 > 2 ? D - 1 : 2);  // (SAMPLE keeps the knot times: one column more)
    double *tkS = pcr_lds;             // [NP] knot times (kept knots first, padding behind them) | the last dof's waypoints
    double *R = tkS + NP;              // [D][NP]  waypoints | right-hand sides -> knot derivatives
    double *X = R + (size_t)D * NP;    // [XC][NP] step durations, raw times | a, c of the rows | the other dofs' waypoints
    __shared__ int cnt_s[KPT * 4];
    __shared__ double bc_s[2][D];
    const bool per_grid = (A.flags & TPR_GRID_PER_TRAJ) != 0;
    const double *__restrict__ ss = A.grid + (per_grid ? b * NS : 0);
    const double *__restrict__ v = A.sd + b * NS;
    const double *__restrict__ breaks = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? b * (nseg + 1) : 0);
    const double *__restrict__ cf = A.coef + b * 4 * nseg * D;
    auto waypoint = [&](double s, double (&out)[D]) {
        const int g = find_segment(breaks, nseg, s);
        const double x = s - breaks[g];
#pragma unroll
        for (int k = 0; k < D; ++k)
            out[k] = cubic_d0(cf[(0 * nseg + g) * D + k], cf[(1 * nseg + g) * D + k], cf[(2 * nseg + g) * D + k], cf[(3 * nseg + g) * D + k], x);
    };

    // (1) time stamps.  Step durations in parallel; the running sum by ONE thread (parametrizer.py:176-186 adds in
    // gridpoint order), while everybody else evaluates the waypoint of its gridpoint -- which gridpoints survive
    // (np.delete(t_grid, skip): a step that takes no time is dropped, the running time keeps it) is a parallel count, and
    // the survivors move to their knot's slot with their waypoints.
    int n;
    double y[KPT][D];
    {
        double *dT = X, *traw = X + NP;
        bool keep[KPT];
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const int u = tid + 256 * j;
            keep[j] = false;
            double g_next = 0.0;
            if (u < N) {
                const double sd_avg = (v[u] + v[u + 1]) / 2;
                g_next = ss[u + 1];
                const double delta_t = isnan(sd_avg) ? qnan() : (sd_avg > kPyTiny ? (g_next - ss[u]) / sd_avg : 5.0);
                dT[u] = delta_t;
                keep[j] = !(delta_t < kPyTiny);
            }
            const unsigned long long m = __ballot(keep[j]);
            if (lane == 0) cnt_s[j * 4 + wv] = __popcll(m);
            if (u < N) waypoint(g_next, y[j]);
        }
        if (tid == 255) {  // gridpoint 0 = knot 0
            double y0[D];
            waypoint(ss[0], y0);
#pragma unroll
            for (int k = 0; k < D; ++k) R[(size_t)k * NP] = y0[k];
            tkS[0] = 0.0;
        }
        if (tid == 254 || tid == 253) {  // clamped ends: q'(path end) * velocity, parametrizer.py:189-194
            const int e = tid == 253;
            const double se = e ? breaks[nseg] : breaks[0];
            const int g = find_segment(breaks, nseg, se);
            const double vel = e ? v[N] : v[0];
#pragma unroll
            for (int k = 0; k < D; ++k) {
                double q1, q2;
                cubic_d1_d2(cf[(0 * nseg + g) * D + k], cf[(1 * nseg + g) * D + k], cf[(2 * nseg + g) * D + k], se - breaks[g], q1, q2);
                bc_s[e][k] = q1 * vel;
            }
        }
        __syncthreads();
        if (tid == 0) {  // the dependent chain: one addition per step, eight steps' durations read ahead
            double t = 0.0, cur[8], nxt[8];
            int u0 = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) cur[e] = dT[e < N ? e : 0];
            for (; u0 + 8 <= N; u0 += 8) {
#pragma unroll
                for (int e = 0; e < 8; ++e) nxt[e] = dT[u0 + 8 + e < N ? u0 + 8 + e : 0];  // in flight during the additions
#pragma unroll
                for (int e = 0; e < 8; ++e) { t = t + cur[e]; traw[u0 + e] = t; }
#pragma unroll
                for (int e = 0; e < 8; ++e) cur[e] = nxt[e];
            }
            for (; u0 < N; ++u0) { t = t + dT[u0]; traw[u0] = t; }
        }
        __syncthreads();
        int base = 1;  // knot 0 is always kept
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const unsigned long long m = __ballot(keep[j]);
            int slot = base + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                slot += w < wv ? cnt_s[j * 4 + w] : 0;
                base += cnt_s[j * 4 + w];
            }
            if (keep[j]) {
                tkS[slot] = traw[tid + 256 * j];
#pragma unroll
                for (int k = 0; k < D; ++k) R[(size_t)k * NP + slot] = y[j][k];
            }
        }
        n = base;
        __syncthreads();
        if (n <= N) {  // rectangular padding: last kept time + 1, + 2, ... (a running sum, as in the other kernels); n is uniform
            if (tid == 0) {
                double t_kept = tkS[n - 1];
                for (int i = n; i <= N; ++i) { t_kept = t_kept + 1.0; tkS[i] = t_kept; }
            }
            __syncthreads();
        }
        if (tid == 0 && A.counts) A.counts[b] = n;
    }
    if (!SAMPLE || A.tk) for (int i = tid; i <= N; i += 256) A.tk[b * NS + i] = tkS[i];

    // (2) the rows of the clamped system, normalised to a unit diagonal: (a, c, r_1..r_d) of knot i.  Chord slopes are formed
    // by both of their knots' threads (the same operands: the same bits) rather than exchanged.
    double *La = X, *Lc = X + NP;
    {
        double ra[KPT], rc[KPT], rr[KPT][D];
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const int i = tid + 256 * j;
            ra[j] = 0.0; rc[j] = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) rr[j][k] = 0.0;
            if (i < n) {
#pragma unroll
                for (int k = 0; k < D; ++k) y[j][k] = R[(size_t)k * NP + i];
                if (i == 0 || i == n - 1) {
#pragma unroll
                    for (int k = 0; k < D; ++k) rr[j][k] = n >= 2 ? bc_s[i != 0][k] : 0.0;
                } else {
                    const double dxm = tkS[i] - tkS[i - 1], dxp = tkS[i + 1] - tkS[i];
                    const double rdm = rcp_refined(dxm), rdp = rcp_refined(dxp);
                    const double rb = rcp_refined(2 * (dxm + dxp));
                    ra[j] = dxp * rb; rc[j] = dxm * rb;
                    const double wm = 3 * ra[j], wp = 3 * rc[j];
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        const double slm = (y[j][k] - R[(size_t)k * NP + i - 1]) * rdm;
                        const double slp = (R[(size_t)k * NP + i + 1] - y[j][k]) * rdp;
                        rr[j][k] = wm * slm + wp * slp;
                    }
                }
            }
        }
        __syncthreads();  // (the waypoints in LDS are dead)
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const int i = tid + 256 * j;
            if (i < n) {
                La[i] = ra[j]; Lc[i] = rc[j];
#pragma unroll
                for (int k = 0; k < D; ++k) R[(size_t)k * NP + i] = rr[j][k];
            }
        }
        __syncthreads();
    }

    // (3) the solve.  row i <- row i combined with rows i - s and i + s so that it couples i - 2s and i + 2s instead:
    auto reduce_row = [&](int i, int s, double &a2, double &c2, double (&r2)[D]) {
        const int im = i - s, ip = i + s;
        const bool hm = im >= 0, hp = ip < n;
        const int jm = hm ? im : i, jp = hp ? ip : i;
        const double ai = hm ? La[i] : 0.0, ci = hp ? Lc[i] : 0.0;
        const double rbb = rcp_refined(__builtin_fma(-ai, Lc[jm], __builtin_fma(-ci, La[jp], 1.0)));
        a2 = -ai * La[jm] * rbb; c2 = -ci * Lc[jp] * rbb;
#pragma unroll
        for (int k = 0; k < D; ++k)
            r2[k] = __builtin_fma(-ai, R[(size_t)k * NP + jm], __builtin_fma(-ci, R[(size_t)k * NP + jp], R[(size_t)k * NP + i])) * rbb;
    };
    // cyclic reduction down to at most 64 rows (every second row drops out per level, updated in place: the rows a
    // level reads are not the rows it writes), parallel cyclic reduction of those by one wave, back substitution
    int L = 0;
    while (((n - 1) >> L) >= 64) ++L;
    for (int l = 0; l < L; ++l) {
        const int s = 1 << l;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const int i = 2 * s * (tid + 256 * j) + 2 * s - 1;
            if (i < n) {
                double a2, c2, r2[D];
                reduce_row(i, s, a2, c2, r2);
                La[i] = a2; Lc[i] = c2;
#pragma unroll
                for (int k = 0; k < D; ++k) R[(size_t)k * NP + i] = r2[k];
            }
        }
        __syncthreads();
    }
    if (wv == 0) {
        const int S = 1 << L, i = S * lane + S - 1;
        for (int p = S; p < n; p <<= 1) {
            double a2 = 0.0, c2 = 0.0, r2[D];
            if (i < n) reduce_row(i, p, a2, c2, r2);
            wave_lds_fence();
            if (i < n) {
                La[i] = a2; Lc[i] = c2;
#pragma unroll
                for (int k = 0; k < D; ++k) R[(size_t)k * NP + i] = r2[k];
            }
            wave_lds_fence();
        }
    }
    __syncthreads();
    for (int l = L - 1; l >= 0; --l) {
        const int s = 1 << l;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const int i = 2 * s * (tid + 256 * j) + s - 1;
            if (i < n) {
                const int im = i - s, ip = i + s;
                const bool hm = im >= 0, hp = ip < n;
                const int jm = hm ? im : i, jp = hp ? ip : i;
                const double ai = hm ? La[i] : 0.0, ci = hp ? Lc[i] : 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k)
                    R[(size_t)k * NP + i] = __builtin_fma(-ai, R[(size_t)k * NP + jm], __builtin_fma(-ci, R[(size_t)k * NP + jp], R[(size_t)k * NP + i]));
            }
        }
        __syncthreads();
    }

    // (4) coefficient rows (CubicHermiteSpline's formulas) lane-parallel over (segment, dof), in the table's own order.
    // The waypoints return to LDS (the rows' a, c and the knot times are dead: the steps come from the knot times this block
    // stored above -- L2).
    auto ycol = [&](int k) { return k < XC ? X + (size_t)k * NP : tkS; };
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const int i = tid + 256 * j;
        if (i < n) {
#pragma unroll
            for (int k = 0; k < D; ++k) ycol(k)[i] = y[j][k];
        }
    }
    __syncthreads();
    if (SAMPLE) {
        const double dur = tkS[n - 1];
        if (tid == 0 && Q.duration) Q.duration[b] = dur;
        const double *tq = Q.times + (Q.times_per_traj ? b * Q.T : 0);
        const int live = n - 1 < 1 ? 1 : n - 1;  // segments in use (ppoly_eval_kernel's `live`)
        for (int idx = tid; idx < Q.T * D; idx += 256) {
            const int s = idx / D, k = idx - s * D;
            const double tt = Q.fractions ? tq[s] * dur : tq[s];
            // interval = clip(searchsorted(knot_times, t, 'right') - 1, 0, live - 1), as ppoly_eval_kernel
            int lo = 0, hi = live + 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tkS[mid] <= tt) lo = mid + 1; else hi = mid;
            }
            int jj = lo - 1;
            if (jj > live - 1) jj = live - 1;
            if (jj < 0) jj = 0;
            const double *Mk = R + (size_t)k * NP, *Yk = ycol(k);
            double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = Yk[n - 1];
            if (jj <= n - 2) {
                const double rd = rcp_refined(tkS[jj + 1] - tkS[jj]);
                const double si = Mk[jj], sn = Mk[jj + 1];
                const double y0 = Yk[jj], sl = (Yk[jj + 1] - y0) * rd;
                const double t = (si + sn - 2 * sl) * rd;
                c0 = t * rd; c1 = (sl - si) * rd - t; c2 = si; c3 = y0;
            }
            const double x = tt - tkS[jj];
            double q1, q2;
            cubic_d1_d2(c0, c1, c2, x, q1, q2);
            const size_t at = (b * Q.T + s) * D + k;
            if (Q.q[0]) Q.q[0][at] = cubic_d0(c0, c1, c2, c3, x);
            if (Q.q[1]) Q.q[1][at] = q1;
            if (Q.q[2]) Q.q[2][at] = q2;
        }
        return;
    }
    const size_t cs = (size_t)N * D;
    double *__restrict__ o = coef_t + b * 4 * cs;
    const double *tkg = A.tk + b * NS;
    for (int idx = tid; idx < N * D; idx += 256) {
        const int jj = idx / D, k = idx - jj * D;
        const double *Mk = R + (size_t)k * NP, *Yk = ycol(k);
        double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = Yk[n - 1];
        if (jj <= n - 2) {
            const double rd = rcp_refined(tkg[jj + 1] - tkg[jj]);
            const double si = Mk[jj], sn = Mk[jj + 1];
            const double y0 = Yk[jj], sl = (Yk[jj + 1] - y0) * rd;
            const double t = (si + sn - 2 * sl) * rd;
            c0 = t * rd; c1 = (sl - si) * rd - t; c2 = si; c3 = y0;
        }
        o[idx] = c0; o[cs + idx] = c1; o[2 * cs + idx] = c2; o[3 * cs + idx] = c3;
    }
}

// Piecewise-cubic evaluation (scipy PPoly of a CubicSpline and its derivatives) for B paths with their own
// breakpoints: times [B][T] -> out [B][T][d], order 0 / 1 / 2.  counts (optional): valid breakpoints per path.
struct PpolyArgs {
    int B, nseg, d, T, order;
    const double *coef;    // [B][4][nseg][d]
    const double *breaks;  // [B][nseg+1]
    const int32_t *counts; // [B] or nullptr
    const double *times;   // [B][T]
    double *out;           // [B][T][d]
};

// One thread per (sample, dof): the d lanes of a sample read its four coefficient rows as four contiguous d-double pieces
// (a load instruction of the wave touches 64/d samples' pieces instead of 64 scattered doubles of 64 samples: the
// thread-per-sample form of round 2 spent 2.0 ms at 65536 x 64 samples x 7 dof waiting for its 28 scattered loads per
// lane), search the breakpoints together (same addresses: broadcast loads) and store consecutive doubles.
__global__ void __launch_bounds__(256) ppoly_eval_kernel(PpolyArgs A) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int nseg = A.nseg, d = A.d;
    if (gid >= (long long)A.B * A.T * d) return;
    const long long sample = gid / d;
    const int k = (int)(gid - sample * d);
    const int b = (int)(sample / A.T);
    const double *__restrict__ brk = A.breaks + (size_t)b * (nseg + 1);
    const double *__restrict__ cf = A.coef + (size_t)b * 4 * nseg * d;
    int live = A.counts ? A.counts[b] - 1 : nseg;  // segments in use ...
    live = live < 1 ? 1 : (live > nseg ? nseg : live);  // ... never outside the tables, whatever counts holds
    const double t = A.times[sample];
    // interval = clip(searchsorted(breaks, t, 'right') - 1, 0, live - 1)  (extrapolation from the end segments)
    int lo = 0, hi = live + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (brk[mid] <= t) lo = mid + 1; else hi = mid;
    }
    int j = lo - 1;
    if (j > live - 1) j = live - 1;
    if (j < 0) j = 0;
    const double x = t - brk[j];
    const double c0 = cf[(0 * nseg + j) * d + k], c1 = cf[(1 * nseg + j) * d + k], c2 = cf[(2 * nseg + j) * d + k];
    double q1, q2;
    cubic_d1_d2(c0, c1, c2, x, q1, q2);
    A.out[gid] = A.order == 0 ? cubic_d0(c0, c1, c2, cf[(3 * nseg + j) * d + k], x) : (A.order == 1 ? q1 : q2);
}

}  // namespace tpr

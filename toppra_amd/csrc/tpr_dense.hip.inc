// tpr_dense.hip.inc -- the seidel path on DENSE constraint rows: any canonical-linear constraint set.
//
// The fused kernels regenerate the rows of JointVelocityConstraint + JointAccelerationConstraint from the path's spline
// table.  The reference's wrapper is more general: seidelWrapper.__init__ (cy_seidel_solverwrapper.pyx:425-531) flattens
// ANY list of canonical-linear constraints -- SecondOrderConstraint / JointTorqueConstraint with a user's inverse
// dynamics, varying velocity limits, hand-written (a, b, c, F, g) -- into a_arr, b_arr, c_arr [N+1][nC] (rows 0, 1
// reserved for the x_next pair), low_arr, high_arr [N+1][2] and deltas [N], and everything after that
// (solve_stagewise_optim :549-697, compute_controllable_sets / compute_parameterization / compute_feasible_sets,
// reachability_algorithm.py:131-376) reads nothing else.  These kernels take exactly those arrays for B trajectories.
// Rows across lanes as in family 2 (tpr_group.hip.inc: 8 lanes per trajectory up to 34 rows, 16 up to 66, 32 up to 122), every stage LP
// through the reference's full Seidel iteration (group_lp2d / group_lp1d: its decisions and arithmetic, warm-start state
// carried along as the wrapper object carries it) -- no certificates: they lean on the structure of the generated rows.
// Missing rows of the last slots hold the disabled row (0, 0, -1), which Seidel never pivots on and never projects.
// Row traffic: 24 (nC + 2) bytes per stage and pass, 8 consecutive rows per group load; it hides behind the iteration's
// instruction count, which is what bounds these kernels (DESIGN.md section 3.5).
// Included by tpr_dense_tu.hip, tpr_sampled_tu.hip and tpr_boxed_tu.hip (after tpr_dense_args.hpp).

namespace tpr {

// Rows of stage i of one trajectory onto the group's slots (the counterpart of GroupTraj::build).
template <int D, int L>
struct DenseStage {
    using C = GroupCfg<D, L>;
    using Args = DenseArgs;
    const double *a, *b, *c, *low, *high, *deltas;
    int nC;
    double *rowbuf;
    // trajectory bb of the batch; rb: the group's LDS row mirror
    __device__ inline void init(const DenseArgs &A, int bb, int gl, double *rb) {
        const int N = A.N;
        nC = A.nC;
        a = A.a + (size_t)bb * (N + 1) * nC; b = A.b + (size_t)bb * (N + 1) * nC; c = A.c + (size_t)bb * (N + 1) * nC;
        low = A.low + (size_t)bb * 2 * (N + 1); high = A.high + (size_t)bb * 2 * (N + 1);
        deltas = A.deltas + (size_t)bb * N;
        rowbuf = rb;
    }
    __device__ inline double delta(int i) const { return deltas[i]; }
    template <bool MIRROR>
    __device__ inline void build(Slots<D, L> &R, int gl, int i, double delta, double n0, double n1, double &low0,
                                 double &high0, double &low1, double &high1, bool last, double xcap) const {
        low0 = low[2 * i]; high0 = high[2 * i];
        low1 = low[2 * i + 1]; high1 = high[2 * i + 1];
        // (feasible sets: x_min / x_max of solve_stagewise_optim intersect the box, cy_seidel_solverwrapper.pyx:598-601)
        low1 = low1 > -xcap ? low1 : -xcap;
        high1 = high1 < xcap ? high1 : xcap;
        const double *ai = a + (size_t)i * nC, *bi = b + (size_t)i * nC, *ci = c + (size_t)i * nC;
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
            const int r = vi - 4;  // the wrapper's row index
            if (r >= 2 && r < nC) { ra = ai[r]; rb = bi[r]; rc = ci[r]; }
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

// The same contract with the stage's rows GENERATED from path samples (tpr_sampled_problem): the velocity + acceleration
// rows of any geometric path, given as q', q'' [N+1][d] at the gridpoints.  The slots hold what second_order_rows_kernel
// (nblocks = 0) writes into the dense arrays, expression for expression -- [q'_i, -q'_i (| q'_{i+1} + (2 delta) q''_{i+1},
// -...)], [q'', ...], c = -amax / amin, the +-1e8 box with velocity_xbound's fp32 running bounds, the last stage
// repeating itself -- so every pass returns the bits of the dense pass on those rows.  Here D is the slot layout
// (2 + 4 D >= nC) and d the path's dof: under Collocation 2 d rows take the place of 4 D.
// Loads: a slot reads its q', q'' straight from global memory, consecutive lanes consecutive dofs -- per stage the group
// touches the 4 d doubles of gridpoints i and i + 1, two short runs of 8 d bytes in each of the two arrays.  No LDS
// staging: the run of gridpoint i + 1 is the run of gridpoint i one stage later (and the whole trajectory is read again
// by the forward scan), so three of the four runs of a stage are cache hits either way, and staging would put a second
// wave barrier and 4 d more LDS doubles per group (q', q'' of both gridpoints) in front of every stage for a load that is already one instruction per
// slot (DESIGN.md section 3.5).
template <int D, int L>
struct SampledStage {
    using C = GroupCfg<D, L>;
    using Args = SampledArgs;
    int dof[C::S];      // dof of an acceleration row, -1 otherwise
    bool neg[C::S];     // row is the negated half of its +- pair
    bool nextpt[C::S];  // row is evaluated at s_{i+1} (the Interpolation block)
    double climit[C::S];
    const double *qs, *qss, *grid, *vlim;
    int d;
    double *rowbuf;
    __device__ inline void init(const SampledArgs &A, int bb, int gl, double *rb) {
        d = A.d;
        const int N = A.N;
        qs = A.qs + (size_t)bb * (N + 1) * d; qss = A.qss + (size_t)bb * (N + 1) * d;
        grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)bb * (N + 1) : 0);
        vlim = (A.flags & TPR_HAS_VELOCITY) ? A.vlim + (size_t)bb * 2 * d : nullptr;
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
        low0 = kVarMin; high0 = kVarMax;
        low1 = kVarMin; high1 = kVarMax;
        if (vlim) {  // velocity_xbound with the dofs across the group's lanes: min / max of fp32-rounded quotients in any order
            float sdmin = -kJvelMaxSd, sdmax = kJvelMaxSd;
            for (int k = gl; k < d; k += L) {
                const double q1 = q1i[k], vlo = vlim[2 * k], vhi = vlim[2 * k + 1];
                const double rmax = (q1 > 0 ? vhi : vlo) / q1, rmin = (q1 > 0 ? vlo : vhi) / q1;
                if (q1 != 0) {
                    sdmax = (float)(rmax <= (double)sdmax ? rmax : (double)sdmax);
                    sdmin = (float)(rmin >= (double)sdmin ? rmin : (double)sdmin);
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

constexpr double kDenseNoCap = 1e300;  // "no x box beyond the wrapper's own"

// compute_controllable_sets + compute_parameterization (backward_only: the first alone) -- group_solve_kernel's scans
// with every LP through the full iteration.
template <int D, int L, class Stage = DenseStage<D, L>>
__global__ void __launch_bounds__(256) dense_solve_kernel(typename Stage::Args A) {
    using C = GroupCfg<D, L>;
    const int kGroupsPerBlock = blockDim.x / L;
    extern __shared__ double lds[];
    const int tid = threadIdx.x, gl = tid % L, gidx = tid / L;
    const int b = blockIdx.x * kGroupsPerBlock + gidx;
    const bool alive0 = b < A.B;
    const int bb = alive0 ? b : A.B - 1;  // idle groups shadow the last trajectory, never store
    const int N = A.N;
    Stage T;
    T.init(A, bb, gl, lds + (size_t)gidx * C::kRowBuf);

    Slots<D, L> R;
    double *K = A.K + (size_t)bb * 2 * (N + 1);
    double *xs = A.sd2 ? A.sd2 + (size_t)bb * (N + 1) : nullptr;
    double *sdv = A.sd ? A.sd + (size_t)bb * (N + 1) : nullptr;
    double *us = A.u ? A.u + (size_t)bb * N : nullptr;
    const bool writer = alive0 && gl == 0;
    const double sd_start = A.sd_start ? A.sd_start[bb] : 0.0;
    const double sd_end = A.sd_end ? A.sd_end[bb] : 0.0;

    // ---- backward scan: controllable sets (reachability_algorithm.py:166-238) -----------------------------
    // warm-start state (active_c_up / active_c_down, reference row ids): a fresh object's zeros, or what an earlier pass on
    // the same wrapper object left behind (tpr_dense_problem.active)
    int up0 = 0, up1 = 0, dn0 = 0, dn1 = 0;
    if (A.active) { const int32_t *st = A.active + (size_t)bb * 4; up0 = st[0]; up1 = st[1]; dn0 = st[2]; dn1 = st[3]; }
    auto put_state = [&]() {
        if (A.active && writer) { int32_t *st = A.active + (size_t)bb * 4; st[0] = up0; st[1] = up1; st[2] = dn0; st[3] = dn1; }
    };
    double kn0 = boundary_x(A.flags, sd_end), kn1 = A.sd_end_hi ? boundary_x(A.flags, A.sd_end_hi[bb]) : kn0;
    if (writer) { K[2 * N] = kn0; K[2 * N + 1] = kn1; }
    bool failed = false;
    for (int i = N - 1; i >= 0; --i) {
        const double delta = T.delta(i);
        double lo = 0, hi = 0;
        if (!failed) {
            if (isnan(kn0) || isnan(kn1)) { lo = qnan(); hi = qnan(); }
            else {
                double low0, high0, low1, high1;
                T.template build<true>(R, gl, i, delta, kn0, kn1, low0, high0, low1, high1, false, kDenseNoCap);
                const GroupLp su = group_lp2d<D, L>(R, T.rowbuf, gl, -1e-9, 1.0, low0, high0, low1, high1, dn0, dn1);
                if (su.ok) { dn0 = su.ac0; dn1 = su.ac1; }
                hi = su.x;
                const GroupLp sl = group_lp2d<D, L>(R, T.rowbuf, gl, 1e-9, -1.0, low0, high0, low1, high1, up0, up1);
                if (sl.ok) { up0 = sl.ac0; up1 = sl.ac1; }
                lo = sl.x;
            }
            if (lo < 0) lo = 0;
            if (isnan(lo) || isnan(hi)) failed = true;
        }
        if (writer) { K[2 * i] = lo; K[2 * i + 1] = hi; }
        kn0 = lo; kn1 = hi;
    }
    const double x_start = boundary_x(A.flags, sd_start);
    const bool uncontrollable = failed || x_start + kPySmall < kn0 || kn1 + kPySmall < x_start;
    if (A.backward_only) {
        if (writer && A.status) A.status[bb] = uncontrollable ? TPR_STATUS_FAIL_UNCONTROLLABLE : TPR_STATUS_OK;
        put_state();
        return;
    }
    if (uncontrollable) {
        put_state();
        if (writer) {
            for (int i = 0; i <= N; ++i) { if (xs) xs[i] = qnan(); if (sdv) sdv[i] = qnan(); }
            for (int i = 0; i < N; ++i) if (us) us[i] = qnan();
            if (A.status) A.status[bb] = TPR_STATUS_FAIL_UNCONTROLLABLE;
        }
        return;
    }
    __threadfence_block();  // K rows written by lane 0 are re-read by the whole group below

    // ---- forward scan: parameterization (reachability_algorithm.py:240-376, time_optimal_algorithm.py:55-92) ------
    double x = x_start;
    double sq = sqrt(x);
    bool any_nan = isnan(sq);
    if (writer) { if (xs) xs[0] = x; if (sdv) sdv[0] = sq; }
    int tries = 0, i = 0;
    bool rows_ready = false;
    double delta = 0, k0 = 0, k1 = 0, low0 = 0, high0 = 0;
    while (i < N) {
        if (!rows_ready) {
            k0 = K[2 * (i + 1)]; k1 = K[2 * (i + 1) + 1];
            delta = T.delta(i);
            double low1, high1;
            T.template build<false>(R, gl, i, delta, k0, k1, low0, high0, low1, high1, false, kDenseNoCap);
            rows_ready = true;
        }
        double uu = qnan();
        bool ok = false;
        int act1d = 0;
        if (!isnan(x)) ok = group_lp1d_active<D, L>(R, gl, 2 * delta, x, low0, high0, uu, act1d);
        if (ok) dn0 = act1d;  // the 1-variable path's write into active_c_down (cy_seidel_solverwrapper.pyx:646-649)
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
            i += 1;
        }
    }
    if (writer && A.status) A.status[bb] = any_nan ? TPR_STATUS_ERR_UNKNOWN : TPR_STATUS_OK;
    put_state();
}

// compute_feasible_sets (reachability_algorithm.py:131-164): group_feasible_kernel on dense rows.
template <int D, int L, class Stage = DenseStage<D, L>>
__global__ void __launch_bounds__(256) dense_feasible_kernel(typename Stage::Args A) {
    using C = GroupCfg<D, L>;
    const int kGroupsPerBlock = blockDim.x / L;
    extern __shared__ double lds[];
    const int tid = threadIdx.x, gl = tid % L, gidx = tid / L;
    const int b = blockIdx.x * kGroupsPerBlock + gidx;
    const bool alive0 = b < A.B;
    const int bb = alive0 ? b : A.B - 1;
    const int N = A.N;
    Stage T;
    T.init(A, bb, gl, lds + (size_t)gidx * C::kRowBuf);
    Slots<D, L> R;
    double *Xb = A.X + (size_t)bb * 2 * (N + 1);
    const bool writer = alive0 && gl == 0;
    int up0 = 0, up1 = 0, dn0 = 0, dn1 = 0;
    if (A.active) { const int32_t *st = A.active + (size_t)bb * 4; up0 = st[0]; up1 = st[1]; dn0 = st[2]; dn1 = st[3]; }
    for (int i = 0; i <= N; ++i) {
        const bool last = i == N;
        const double delta = last ? 0.0 : T.delta(i);
        double low0, high0, low1, high1;
        T.template build<true>(R, gl, i, delta, -kFeasMaxX, kFeasMaxX, low0, high0, low1, high1, last, kFeasMaxX);
        GroupLp sl = group_lp2d<D, L>(R, T.rowbuf, gl, -1e-9, -1.0, low0, high0, low1, high1, up0, up1);
        if (sl.ok) { up0 = sl.ac0; up1 = sl.ac1; }
        GroupLp su = group_lp2d<D, L>(R, T.rowbuf, gl, 1e-9, 1.0, low0, high0, low1, high1, dn0, dn1);
        if (su.ok) { dn0 = su.ac0; dn1 = su.ac1; }
        double lo = sl.x;
        if (lo < 0) lo = 0;
        if (writer) { Xb[2 * i] = lo; Xb[2 * i + 1] = su.x; }
    }
    if (A.active && writer) { int32_t *st = A.active + (size_t)bb * 4; st[0] = up0; st[1] = up1; st[2] = dn0; st[3] = dn1; }
}

// The two forward scans of TOPPRAsd (desired_duration_algorithm.py:93-142,219-226) on dense rows: group_sd_forward_kernel
// with the stage rows loaded.  Reads K and the controllability verdict (status) of the backward scan.
template <int D, int L, class Stage = DenseStage<D, L>>
__global__ void __launch_bounds__(256) dense_sd_forward_kernel(typename Stage::Args A) {
    using C = GroupCfg<D, L>;
    const int kGroupsPerBlock = blockDim.x / L;
    extern __shared__ double lds[];
    const int tid = threadIdx.x, gl = tid % L, gidx = tid / L;
    const int b = blockIdx.x * kGroupsPerBlock + gidx;
    const bool alive0 = b < A.B;
    const int bb = alive0 ? b : A.B - 1;
    const int N = A.N;
    Stage T;
    T.init(A, bb, gl, lds + (size_t)gidx * C::kRowBuf);
    const double *K = A.K + (size_t)bb * 2 * (N + 1);
    double *xf = A.sd_xf + (size_t)bb * (N + 1), *xl = A.sd_xl + (size_t)bb * (N + 1);
    double *uf = A.sd_uf + (size_t)bb * N, *ul = A.sd_ul + (size_t)bb * N;
    const bool writer = alive0 && gl == 0;
    Slots<D, L> R;
    const double sd_start = A.sd_start ? A.sd_start[bb] : 0.0;
    double x_fast = boundary_x(A.flags, sd_start), x_slow = x_fast;
    if (A.status[bb] == TPR_STATUS_FAIL_UNCONTROLLABLE) { x_fast = qnan(); x_slow = qnan(); }
    if (writer) { xf[0] = x_fast; xl[0] = x_slow; }
    int st_up0 = 0, st_dn0 = 0;  // (the backward scan of the same call left the state in A.active)
    if (A.active) { st_up0 = A.active[(size_t)bb * 4]; st_dn0 = A.active[(size_t)bb * 4 + 2]; }
    for (int i = 0; i < N; ++i) {
        const double delta = T.delta(i);
        const double k0 = K[2 * (i + 1)], k1 = K[2 * (i + 1) + 1];
        double low0, high0, low1, high1;
        T.template build<false>(R, gl, i, delta, k0, k1, low0, high0, low1, high1, false, kDenseNoCap);
        // fastest: max u ; slowest: min u (v0 = -g0 = -2 delta < 0 picks the lower end)
        double u_fast = qnan(), u_slow = qnan();
        bool ok_fast = false, ok_slow = false;
        int act_fast = 0, act_slow = 0;
        if (!isnan(x_fast)) ok_fast = group_lp1d_active<D, L>(R, gl, 2 * delta, x_fast, low0, high0, u_fast, act_fast);
        if (!isnan(x_slow)) ok_slow = group_lp1d_active<D, L>(R, gl, -2 * delta, x_slow, low0, high0, u_slow, act_slow);
        // the 1-variable path's writes (cy_seidel_solverwrapper.pyx:646-649): g = [-2 delta, -1] -> active_c_down, [2 delta, 1] -> active_c_up
        if (ok_fast) st_dn0 = act_fast;
        if (ok_slow) st_up0 = act_slow;
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
    }
    if (A.active && writer) { A.active[(size_t)bb * 4] = st_up0; A.active[(size_t)bb * 4 + 2] = st_dn0; }
}

// Host side: launch geometry of one pass, shared by the units that instantiate these kernels.
template <int D, int L, class Stage = DenseStage<D, L>>
static int dense_launch(const typename Stage::Args &A, int feasible /* 0 solve, 1 feasible sets, 2 TOPPRAsd forward scans */, hipStream_t stream) {
    using C = GroupCfg<D, L>;
    const int threads = shrink_block_to_batch(256, A.B, L);  // small batches: more, smaller blocks
    const int groups = threads / L;
    const size_t lds = (size_t)groups * C::kRowBuf * sizeof(double);
    const dim3 grid((A.B + groups - 1) / groups), block(threads);
    if (feasible == 1) hipLaunchKernelGGL((dense_feasible_kernel<D, L, Stage>), grid, block, lds, stream, A);
    else if (feasible == 2) hipLaunchKernelGGL((dense_sd_forward_kernel<D, L, Stage>), grid, block, lds, stream, A);
    else hipLaunchKernelGGL((dense_solve_kernel<D, L, Stage>), grid, block, lds, stream, A);
    return 0;
}

// ... and the layout of a call, the one table of the three units: nC rows per stage (incl. the two x_next rows; 2 + (4 | 2 | 0) d
// by the flags when they are generated) -> the smallest row-slot layout that holds them, 2 + 4 D >= nC, on 8 / 16 / 32 lanes.
// 0 = launched, -1 = more rows than the layouts hold (122: the row keys carry the virtual row index in 7 bits).
template <template <int, int> class Stage>
static int dense_dispatch(const typename Stage<1, 8>::Args &A, int feasible, hipStream_t stream) {
    const int D = A.nC <= 6 ? 1 : (A.nC - 2 + 3) / 4;
    switch (D) {
#define TPR_DENSE_CASE(DD, LL) case DD: return dense_launch<DD, LL, Stage<DD, LL>>(A, feasible, stream)
        TPR_DENSE_CASE(1, 8); TPR_DENSE_CASE(2, 8); TPR_DENSE_CASE(3, 8); TPR_DENSE_CASE(4, 8);
        TPR_DENSE_CASE(5, 8); TPR_DENSE_CASE(6, 8); TPR_DENSE_CASE(7, 8); TPR_DENSE_CASE(8, 8);
        TPR_DENSE_CASE(9, 16); TPR_DENSE_CASE(10, 16); TPR_DENSE_CASE(11, 16); TPR_DENSE_CASE(12, 16);
        TPR_DENSE_CASE(13, 16); TPR_DENSE_CASE(14, 16); TPR_DENSE_CASE(15, 16); TPR_DENSE_CASE(16, 16);
        TPR_DENSE_CASE(17, 32); TPR_DENSE_CASE(18, 32); TPR_DENSE_CASE(19, 32); TPR_DENSE_CASE(20, 32);
        TPR_DENSE_CASE(21, 32); TPR_DENSE_CASE(22, 32); TPR_DENSE_CASE(23, 32); TPR_DENSE_CASE(24, 32);
        TPR_DENSE_CASE(25, 32); TPR_DENSE_CASE(26, 32); TPR_DENSE_CASE(27, 32); TPR_DENSE_CASE(28, 32);
        TPR_DENSE_CASE(29, 32); TPR_DENSE_CASE(30, 32);
#undef TPR_DENSE_CASE
    }
    return -1;
}

}  // namespace tpr

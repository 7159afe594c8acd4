// tpr_robust.hip.inc -- robust (conic) TOPP-RA: stage problems of RobustLinearConstraint.
//
// PARITY UNPINNED against ECOS (the reference's solver: absent here, and the reference holds no golden vectors for it);
// cross-checked at 1e-7 against an independent exact solver (tests/test_gpu_robust.py).
// The reference hands these stage problems to ECOS (an interior-point SOCP
// solver, toppra/solverwrapper/ecos_solverwrapper.py:90-207) which is not available; this solves the
// same *problem* -- rows a u + b x + c + ||(ru u, rx x, rc)|| <= 0 (conic_constraint.py:19-26), the
// velocity box capped at ECOS_MAXX, absent bounds replaced by +-ECOS_INFTY, x_next bounds -- exactly,
// by an elementary method: for fixed x every row is a closed-form interval in u, so the feasible x
// form an interval whose ends are found by bisection on "the u-interval is non-empty".  The scans
// around it are the reference's (reachability_algorithm.py:166-376).  One trajectory per lane
// (generic dof and discretisation); checked bit for bit against the CPU restatement of the same
// method and, for a zero ellipsoid, against the seidel LP path.  Included by tpr_kernels.hip.

#pragma once
#include "tpr_robust_args.hpp"
namespace tpr {

constexpr double kEcosInfty = 1000.0;  // toppra/constants.py:47
constexpr double kEcosMaxX = 10000.0;  // toppra/constants.py:46
constexpr int kRobIters = 64;
constexpr int kRobSecant = 24;

// The end of the feasible x interval between a feasible point `good` and an infeasible one `bad`: the width
// g(x) = h - l of the u-interval is concave in x, so its zero is bracketed and found by the Illinois variant of
// regula falsi (secant steps; the value of an end kept twice is halved), with plain bisection when g is not
// finite at an end (unbounded interval / a row that admits no u) and after kRobSecant steps, so that the bracket
// always closes to rounding level within kRobIters evaluations.  Returns the last FEASIBLE point: the bound is
// never overstated.  interval(x, l, h): the u-interval at x.
// ga_known / gb_known: the merit at `good` / `bad` when the caller has evaluated that point already (the ends of the x box
// are probed before any search: round 3 -- two of a stage's ~12 interval evaluations were repeats), NaN otherwise.
template <class Interval>
__device__ inline double rob_edge(Interval &&interval, double good, double bad, double guess, double ga_known, double gb_known) {
    double l, h, g;  // g: the interval's edge merit (finite on both sides of the boundary, never flat on the feasible side)
    auto g_of = [&]() { return g; };
    double ga = ga_known, gb = gb_known;
    if (isnan(ga_known)) { interval(good, l, h, g); ga = g_of(); }
    if (isnan(gb_known)) { interval(bad, l, h, g); gb = g_of(); }
    // the neighbouring stage's bound is a good first guess: probe it and a point 2 % beyond it
    for (int probe = 0; probe < 2; ++probe) {
        const double lo = good < bad ? good : bad, hi = good < bad ? bad : good;
        if (!(guess > lo && guess < hi)) break;
        interval(guess, l, h, g);
        const double step = 0.02 * (fabs(guess) + 1e-3) * (bad > good ? 1.0 : -1.0);
        if (l <= h) { good = guess; ga = g_of(); guess = guess + step; }
        else { bad = guess; gb = g_of(); guess = guess - step; }
    }
    int last = 0;
    for (int it = 0; it < kRobIters; ++it) {
        const double width = bad - good;
        if (!(fabs(width) > 4.5e-16 * fmax(fabs(good), fabs(bad)))) break;
        const bool sec = it < kRobSecant && isfinite(ga) && isfinite(gb) && ga - gb > 0;
        double f = sec ? ga / (ga - gb) : 0.5;

        double mid = good + width * f;
        // a secant step shorter than ~2 ulp is replaced by a 2 ulp step: it jumps ACROSS the root, which is what
        // closes the bracket when the iterates approach from one side (Brent's minimum step)
        const double minstep = 4.5e-16 * fmax(fabs(good), fabs(bad)) * (width > 0 ? 1.0 : -1.0);
        if (fabs(mid - good) < fabs(minstep)) mid = good + minstep;
        if (fabs(bad - mid) < fabs(minstep)) mid = bad - minstep;
        if (mid == good || mid == bad) mid = 0.5 * (good + bad);
        if (mid == good || mid == bad) break;
        interval(mid, l, h, g);
        const double gm = g_of();
        if (l <= h) { good = mid; ga = gm; if (last > 0) gb *= 0.5; last = 1; }
        else { bad = mid; gb = gm; if (last < 0) ga *= 0.5; last = -1; }
    }
    return good;
}

__device__ __forceinline__ double pinf() { return __longlong_as_double(0x7ff0000000000000LL); }

// u-interval of one row at fixed x.  viol = -inf when the row admits some u, otherwise the row's smallest
// attainable residual min_u (a u + m + ||.||) > 0: a convex function of x that tells the search for a
// feasible x which way to go (rows with |a| < ru exclude whole ranges of x).
__device__ inline void rob_row_interval(double a, double b, double c, double ru, double rx, double rc, double x,
                                        double &lo, double &hi, double &viol) {
    const double kap = (rx * x) * (rx * x) + rc * rc, m = b * x + c, A = a * a - ru * ru;
    lo = -pinf(); hi = pinf(); viol = -pinf();
    if (A > 0) {
        // one quotient for both signs of a (the +- twin rows of a joint sit in neighbouring lanes: as two branches half of
        // the lanes idled through each division); x - s == x + (-s) exactly
        // limits written as 1e300: m * m overflows, the root would be +inf and a row that is slack by 1e300 would bound u
        // at -+inf.  There |m| > 1.3e154 and the root is |m| ru (kap A, at most ~1e8 a^2, is far below an ulp of ru^2 m^2)
        const double mm = m * m, root = sqrt(kap * A + (ru * ru) * mm);
        const double s = mm == pinf() ? fabs(m) * ru : root;
        const bool up = a > 0;
        const double val = (-a * m + (up ? -s : s)) / A;
        hi = up ? val : hi; lo = up ? lo : val;
    } else if (A < 0) {
        const double disc = kap * A + (ru * ru) * (m * m);
        if (disc < 0 || m > 0) { lo = pinf(); hi = -pinf(); viol = m + sqrt(kap * -A) / ru; return; }
        const double s = sqrt(disc), r1 = (-a * m - s) / A, r2 = (-a * m + s) / A;
        lo = r1 < r2 ? r1 : r2; hi = r1 < r2 ? r2 : r1;
    } else {
        if (m >= 0) { lo = pinf(); hi = -pinf(); viol = m; return; }
        if (a > 0) hi = (kap - m * m) / (2 * a * m);
        else if (a < 0) lo = (kap - m * m) / (2 * a * m);
        else if (m * m < kap) { lo = pinf(); hi = -pinf(); viol = m + sqrt(kap); }
    }
}

// Merit of x in the search for a feasible point, two levels compared lexicographically:
//   ok = false: some row admits no u at this x; val = -(largest such violation)   (concave in x)
//   ok = true:  every row admits some u;        val = width of the intersection   (concave in x; >= 0: feasible)
struct RobMerit {
    bool ok;
    double val;
    __device__ bool feasible() const { return ok && val >= 0; }
    __device__ bool better_than(const RobMerit &q) const { return ok != q.ok ? ok : val > q.val; }
};
__device__ inline RobMerit rob_merit_of(double l, double h, double v) {
    RobMerit m;
    m.ok = !(v > -pinf());
    m.val = m.ok ? h - l : -v;
    return m;
}

struct RobStage {
    const StageRows *R;
    double ru, rx, rc, n0, n1, d2;
    bool has_next;
};

// gedge: merit for the edge search -- minus the row violation where a row admits no u, else the width h - l of the
// interval; when the x_next rows form an equality (they pin u, the width is 0 on the whole feasible side) the slack
// of that u against the rows' own interval instead.
__device__ inline void rob_u_interval(const RobStage &S, double x, double &lo, double &hi, double &vmax, double *gedge = nullptr) {
    double l = -pinf(), h = pinf(), v = -pinf();
    for (int j = 2; j < S.R->nC; ++j) {
        double rl, rh, rv;
        rob_row_interval(S.R->a[j], S.R->b[j], S.R->c[j], S.ru, S.rx, S.rc, x, rl, rh, rv);
        l = rl > l ? rl : l; h = rh < h ? rh : h; v = rv > v ? rv : v;
    }
    double g = 0;
    bool eq = false;
    if (S.has_next) {
        const double rl = (S.n0 - x) / S.d2, rh = (S.n1 - x) / S.d2;
        eq = S.n0 == S.n1;
        if (eq) { const double g1 = rl - l, g2 = h - rh; g = g1 < g2 ? g1 : g2; }
        l = rl > l ? rl : l; h = rh < h ? rh : h;
    }
    lo = l; hi = h; vmax = v;
    if (gedge) *gedge = v > -pinf() ? -v : (eq ? g : h - l);
}

__device__ inline bool rob_feasible(const RobStage &S, double x) { double l, h, v; rob_u_interval(S, x, l, h, v); return l <= h; }
__device__ inline RobMerit rob_merit(const RobStage &S, double x) { double l, h, v; rob_u_interval(S, x, l, h, v); return rob_merit_of(l, h, v); }

__device__ inline bool rob_x_interval(const RobStage &S, double xl, double xh, double &x_lower, double &x_upper) {
    if (!(xl <= xh)) return false;
    double el, eh, ev, g_xl, g_xh;  // the box ends: feasibility and the edge merit (reused by the edge searches)
    rob_u_interval(S, xl, el, eh, ev, &g_xl);
    const bool fl = el <= eh;
    rob_u_interval(S, xh, el, eh, ev, &g_xh);
    const bool fh = el <= eh;
    double xf, g_xf = qnan();
    if (fl) { xf = xl; g_xf = g_xl; } else if (fh) { xf = xh; g_xf = g_xh; } else {
        const double gr = 0.6180339887498949;
        double a = xl, b = xh, c1 = b - gr * (b - a), c2 = a + gr * (b - a);
        RobMerit m1 = rob_merit(S, c1), m2 = rob_merit(S, c2);
        bool found = false;
        xf = 0;
        for (int it = 0; it < kRobIters && !found; ++it) {
            if (m1.feasible()) { xf = c1; found = true; break; }
            if (m2.feasible()) { xf = c2; found = true; break; }
            if (m1.better_than(m2)) { b = c2; c2 = c1; m2 = m1; c1 = b - gr * (b - a); m1 = rob_merit(S, c1); }
            else { a = c1; c1 = c2; m1 = m2; c2 = a + gr * (b - a); m2 = rob_merit(S, c2); }
        }
        if (!found) return false;
    }
    auto interval = [&](double xx, double &l, double &h, double &g) { double v; rob_u_interval(S, xx, l, h, v, &g); };
    x_upper = fh ? xh : rob_edge(interval, xf, xh, S.has_next ? S.n1 : xh, g_xf, g_xh);
    x_lower = fl ? xl : rob_edge(interval, xf, xl, S.has_next ? S.n0 : xl, g_xf, g_xl);
    return true;
}

__device__ inline void rob_box(const StageRows &R, bool has_vel, double bound, double &xl, double &xh) {
    xl = -bound; xh = bound;
    if (has_vel) {
        const double hcap = R.high1 < kEcosMaxX ? R.high1 : kEcosMaxX;
        xl = R.low1 > xl ? R.low1 : xl;
        xh = hcap < xh ? hcap : xh;
    }
}


static __global__ void __launch_bounds__(64) robust_solve_kernel(RobustArgs P) {
    const BatchArgs &A = P.A;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= A.B) return;
    const Traj T = make_traj(A, b);
    const int N = A.N, d = A.d;
    StageRows R;
    RobStage S;
    S.R = &R; S.ru = P.ru; S.rx = P.rx; S.rc = P.rc;
    double q1c[TPR_MAX_DOF], q2c[TPR_MAX_DOF], q1n[TPR_MAX_DOF], q2n[TPR_MAX_DOF];
    double *K = A.K + (size_t)b * 2 * (N + 1);
    double *xs = A.sd2 ? A.sd2 + (size_t)b * (N + 1) : nullptr;
    double *sdv = A.sd ? A.sd + (size_t)b * (N + 1) : nullptr;
    double *us = A.u ? A.u + (size_t)b * N : nullptr;
    const double sd_start = A.sd_start ? A.sd_start[b] : 0.0;
    const double sd_end = A.sd_end ? A.sd_end[b] : 0.0;

    if (P.X) {  // compute_feasible_sets: +-1e4 bounds on x and x_next (reachability_algorithm.py:151-156)
        double *X = P.X + (size_t)b * 2 * (N + 1);
        path_eval(T, T.grid[0], q1c, q2c);
        for (int i = 0; i <= N; ++i) {
            const bool last = i == N;
            double delta = 0;
            if (!last) { delta = T.grid[i + 1] - T.grid[i]; path_eval(T, T.grid[i + 1], q1n, q2n); }
            build_rows(T, R, q1c, q2c, q1n, q2n, delta, last);
            double xl, xh, lo, hi;
            rob_box(R, T.has_vel, kFeasMaxX, xl, xh);
            S.has_next = !last; S.n0 = -kFeasMaxX; S.n1 = kFeasMaxX; S.d2 = 2 * delta;
            if (rob_x_interval(S, xl, xh, lo, hi)) { X[2 * i] = lo < 0 ? 0 : lo; X[2 * i + 1] = hi; }
            else { X[2 * i] = qnan(); X[2 * i + 1] = qnan(); }
            for (int k = 0; k < d; ++k) { q1c[k] = q1n[k]; q2c[k] = q2n[k]; }
        }
    }

    // backward scan
    double kn0 = sd_end * sd_end, kn1 = kn0;
    K[2 * N] = kn0; K[2 * N + 1] = kn1;
    bool failed = false;
    path_eval(T, T.grid[N], q1n, q2n);
    double s_next = T.grid[N];
    for (int i = N - 1; i >= 0; --i) {
        if (failed) { K[2 * i] = 0; K[2 * i + 1] = 0; continue; }
        const double s_i = T.grid[i], delta = s_next - s_i;
        path_eval(T, s_i, q1c, q2c);
        build_rows(T, R, q1c, q2c, q1n, q2n, delta, false);
        double xl, xh, lo, hi;
        rob_box(R, T.has_vel, kEcosInfty, xl, xh);
        S.has_next = true; S.n0 = kn0; S.n1 = kn1; S.d2 = 2 * delta;
        if (isnan(kn0) || isnan(kn1) || !rob_x_interval(S, xl, xh, lo, hi)) {
            K[2 * i] = qnan(); K[2 * i + 1] = qnan();
            failed = true;
        } else {
            lo = lo < 0 ? 0 : lo;
            K[2 * i] = lo; K[2 * i + 1] = hi;
            kn0 = lo; kn1 = hi;
        }
        for (int k = 0; k < d; ++k) { q1n[k] = q1c[k]; q2n[k] = q2c[k]; }
        s_next = s_i;
    }
    const double x_start = sd_start * sd_start;
    if (failed || x_start + kPySmall < K[0] || K[1] + kPySmall < x_start) {
        for (int i = 0; i <= N; ++i) { if (xs) xs[i] = qnan(); if (sdv) sdv[i] = qnan(); }
        for (int i = 0; i < N; ++i) if (us) us[i] = qnan();
        if (A.status) A.status[b] = TPR_STATUS_FAIL_UNCONTROLLABLE;
        return;
    }

    // forward scan
    path_eval(T, T.grid[0], q1c, q2c);
    double x = x_start;
    double sq = sqrt(x);
    bool any_nan = isnan(sq);
    if (xs) xs[0] = x;
    if (sdv) sdv[0] = sq;
    int tries = 0, i = 0;
    bool rows_ready = false;
    double delta = 0;
    while (i < N) {
        const double k0 = K[2 * (i + 1)], k1 = K[2 * (i + 1) + 1];
        if (!rows_ready) {
            delta = T.grid[i + 1] - T.grid[i];
            path_eval(T, T.grid[i + 1], q1n, q2n);
            build_rows(T, R, q1c, q2c, q1n, q2n, delta, false);
            rows_ready = true;
        }
        double uu = qnan();
        if (!isnan(x)) {
            double xl, xh, l, h;
            rob_box(R, T.has_vel, kEcosInfty, xl, xh);
            S.has_next = true; S.n0 = k0; S.n1 = k1; S.d2 = 2 * delta;
            if (xl <= x && x <= xh) {
                double vv;
                rob_u_interval(S, x, l, h, vv);
                if (l <= h) uu = h;
            }
        }
        if (isnan(uu)) {
            if (tries < kMaxTries) {
                const double t1 = x - kPyTiny, t2 = 0.999 * x;
                x = t2 > t1 ? t2 : t1;
                tries += 1;
                if (xs) xs[i] = x;
                if (sdv) sdv[i] = sqrt(x);
            } else {
                for (int m = i + 1; m <= N; ++m) { if (xs) xs[m] = qnan(); if (sdv) sdv[m] = qnan(); }
                for (int m = i; m < N; ++m) if (us) us[m] = 0.0;
                any_nan = true;
                break;
            }
        } else {
            tries = 0;
            if (us) us[i] = uu;
            double xn = x + (2 * delta) * uu;
            const double t1 = xn - kPyTiny, t2 = 0.9999 * xn;
            xn = t2 > t1 ? t2 : t1;
            const double m1 = xn > k0 ? xn : k0;
            x = m1 < k1 ? m1 : k1;
            sq = sqrt(x);
            if (xs) xs[i + 1] = x;
            if (sdv) sdv[i + 1] = sq;
            any_nan |= isnan(sq);
            for (int k = 0; k < d; ++k) { q1c[k] = q1n[k]; q2c[k] = q2n[k]; }
            rows_ready = false;
            i += 1;
        }
    }
    if (A.status) A.status[b] = any_nan ? TPR_STATUS_ERR_UNKNOWN : TPR_STATUS_OK;
}


// ---- rows across lanes (as kernel family 2): the same method, the rows of a stage dealt onto the
// L x S register slots of a group of L lanes, the row intervals intersected with DPP min/max
// reductions.  Serves acceleration + Interpolation (what GroupTraj::build generates); feasible sets
// and Collocation stay with the lane kernel above.  min / max are order independent, so the results
// are the lane kernel's bit for bit.
template <int D, int L>
struct GroupRobStage {
    const Slots<D, L> *R;
    double ru, rx, rc, n0, n1, d2;
    int gl;
    int nrow;       // virtual rows 6 .. nrow - 1 are the constraint's rows (Collocation: two blocks; the slots of the
                    // missing interpolation blocks hold disabled rows, which are NOT rows of the robust problem)
    bool has_next;  // false at the last gridpoint of compute_feasible_sets: no x_next rows
    // Slot 0 holds constraint rows in lanes 6 .. L-1 only (rows 0..5 are the box and x_next rows, which the interval
    // evaluation treats apart) and the last occupied slot s_end in lanes 0 .. cnt-1: when cnt <= 6 the two are evaluated
    // as ONE slot (7 dof on 8 lanes: four row evaluations per lane instead of five; min / max do not care about order)
    int s_end;
    bool merge;
    __device__ void set_rows(int nrow_) {
        nrow = nrow_;
        s_end = (nrow_ - 1) / L;
        merge = s_end >= 1 && nrow_ - s_end * L <= 6;
    }
};

template <int D, int L>
__device__ inline void group_rob_u_interval(const GroupRobStage<D, L> &S, double x, double &lo, double &hi, double &vmax,
                                            double *gedge = nullptr) {
    using C = GroupCfg<D, L>;
    double l = -pinf(), h = pinf(), v = -pinf();
#pragma unroll
    for (int s = 0; s < C::S; ++s) {
        if (s == 0 && S.merge) continue;  // (group- and wave-uniform: slot 0 rides with slot s_end below)
        const int vi = s * L + S.gl;
        if (__builtin_amdgcn_ballot_w64(vi >= 6 && vi < S.nrow) == 0) continue;  // no lane of the wave has a row here
        double ra = S.R->a[s], rb = S.R->b[s], rc = S.R->c[s];
        bool row = vi >= 6 && vi < S.nrow;
        if (s > 0 && S.merge && s == S.s_end) {  // lanes 6 .. L-1 are free in this slot: they take slot 0's rows
            const bool from0 = S.gl >= 6;
            ra = from0 ? S.R->a[0] : ra; rb = from0 ? S.R->b[0] : rb; rc = from0 ? S.R->c[0] : rc;
            row = from0 ? S.gl < S.nrow : row;
        }
        double rl, rh, rv;
        rob_row_interval(ra, rb, rc, S.ru, S.rx, S.rc, x, rl, rh, rv);
        l = (row & (rl > l)) ? rl : l;
        h = (row & (rh < h)) ? rh : h;
        v = (row & (rv > v)) ? rv : v;
    }
    l = group_max_f64<L>(l);
    h = group_min_f64<L>(h);
    // (a row that admits no u at this x is rare: the third reduction runs only when some lane of the wave has one)
    if (__builtin_amdgcn_ballot_w64(v > -pinf()) != 0) v = group_max_f64<L>(v);
    double g = 0;
    bool eq = false;
    if (S.has_next) {  // (group-uniform)
        const double rl = (S.n0 - x) / S.d2, rh = (S.n1 - x) / S.d2;
        eq = S.n0 == S.n1;
        const double g1 = rl - l, g2 = h - rh;
        g = g1 < g2 ? g1 : g2;
        l = rl > l ? rl : l; h = rh < h ? rh : h;
    }
    lo = l; hi = h; vmax = v;
    if (gedge) *gedge = v > -pinf() ? -v : (eq ? g : h - l);
}

template <int D, int L>
__device__ inline bool group_rob_x_interval(const GroupRobStage<D, L> &S, double xl, double xh, double &x_lower,
                                            double &x_upper) {
    auto merit = [&](double x) { double l, h, v; group_rob_u_interval<D, L>(S, x, l, h, v); return rob_merit_of(l, h, v); };
    if (!(xl <= xh)) return false;
    double el, eh, ev, g_xl, g_xh;  // the box ends: feasibility and the edge merit (reused by the edge searches)
    group_rob_u_interval<D, L>(S, xl, el, eh, ev, &g_xl);
    const bool fl = el <= eh;
    group_rob_u_interval<D, L>(S, xh, el, eh, ev, &g_xh);
    const bool fh = el <= eh;
    double xf, g_xf = qnan();
    if (fl) { xf = xl; g_xf = g_xl; } else if (fh) { xf = xh; g_xf = g_xh; } else {
        const double gr = 0.6180339887498949;
        double a = xl, b = xh, c1 = b - gr * (b - a), c2 = a + gr * (b - a);
        RobMerit m1 = merit(c1), m2 = merit(c2);
        bool found = false;
        xf = 0;
        for (int it = 0; it < kRobIters && !found; ++it) {
            if (m1.feasible()) { xf = c1; found = true; break; }
            if (m2.feasible()) { xf = c2; found = true; break; }
            if (m1.better_than(m2)) { b = c2; c2 = c1; m2 = m1; c1 = b - gr * (b - a); m1 = merit(c1); }
            else { a = c1; c1 = c2; m1 = m2; c2 = a + gr * (b - a); m2 = merit(c2); }
        }
        if (!found) return false;
    }
    // (group-uniform control flow: every lane of the group sees the same l, h after the reductions)
    auto interval = [&](double xx, double &l, double &h, double &g) { double v; group_rob_u_interval<D, L>(S, xx, l, h, v, &g); };
    x_upper = fh ? xh : rob_edge(interval, xf, xh, S.has_next ? S.n1 : xh, g_xf, g_xh);
    x_lower = fl ? xl : rob_edge(interval, xf, xl, S.has_next ? S.n0 : xl, g_xf, g_xl);
    return true;
}

template <int D, int L>
__global__ void __launch_bounds__(256) group_robust_kernel(RobustArgs P) {
    using C = GroupCfg<D, L>;
    const BatchArgs &A = P.A;
    extern __shared__ double lds[];
    const int kGroupsPerBlock = blockDim.x / L;
    const int tid = threadIdx.x, gl = tid % L, gidx = tid / L;
    const int b = blockIdx.x * kGroupsPerBlock + gidx;
    const bool alive0 = b < A.B;
    const int bb = alive0 ? b : A.B - 1;
    const int N = A.N, nseg = A.nseg;
    // the group's spline table (c0, c1, c2) and breakpoints in LDS, as in group_solve_kernel
    double *rowbuf = lds + (size_t)gidx * C::lds_doubles(nseg, true);
    const double *gcf = A.coef + (size_t)bb * 4 * nseg * D;
    const double *gbrk = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? (size_t)bb * (nseg + 1) : 0);
    double *lcf = rowbuf + C::kRowBuf, *lbrk = lcf + 3 * nseg * D;
    for (int e = gl; e < 3 * nseg * D; e += L) lcf[e] = gcf[e];
    for (int e = gl; e <= nseg; e += L) lbrk[e] = gbrk[e];
    __syncthreads();
    GroupTraj<D, L> T;
    T.cf = lcf; T.breaks = lbrk; T.rowbuf = rowbuf; T.nseg = nseg;
    T.set_flags(A.flags);  // acceleration with Interpolation (four blocks of rows) or Collocation (two)
    T.init(gl, A.alim + (size_t)bb * 2 * D, T.has_vel ? A.vlim + (size_t)bb * 2 * D : nullptr);
    const double *grid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)bb * (N + 1) : 0);
    Slots<D, L> R;
    GroupRobStage<D, L> S;
    S.R = &R; S.ru = P.ru; S.rx = P.rx; S.rc = P.rc; S.gl = gl;
    S.set_rows(6 + T.nblk * D); S.has_next = true;
    double *K = A.K + (size_t)bb * 2 * (N + 1);
    double *xs = A.sd2 ? A.sd2 + (size_t)bb * (N + 1) : nullptr;
    double *sdv = A.sd ? A.sd + (size_t)bb * (N + 1) : nullptr;
    double *us = A.u ? A.u + (size_t)bb * N : nullptr;
    const bool writer = alive0 && gl == 0;
    const double sd_start = A.sd_start ? A.sd_start[bb] : 0.0;
    const double sd_end = A.sd_end ? A.sd_end[bb] : 0.0;
    auto box = [&](double low1, double high1, double &xl, double &xh) {  // rob_box with bound = ECOS_INFTY
        xl = -kEcosInfty; xh = kEcosInfty;
        if (T.has_vel) {
            const double hcap = high1 < kEcosMaxX ? high1 : kEcosMaxX;
            xl = low1 > xl ? low1 : xl;
            xh = hcap < xh ? hcap : xh;
        }
    };

    if (P.X) {  // compute_feasible_sets: +-1e4 bounds on x and x_next (reachability_algorithm.py:151-156), as the lane kernel
        double *X = P.X + (size_t)bb * 2 * (N + 1);
        double s_i = grid[0];
        GridPt gi = T.locate(s_i);
        for (int i = 0; i <= N; ++i) {
            const bool last = i == N;
            const double s_nx = last ? s_i : grid[i + 1];
            const double delta = s_nx - s_i;
            const GridPt gnx = last ? gi : T.locate(s_nx);
            double low1, high1, xl, xh, lo, hi;
            T.template build<true>(R, gl, gi, gnx, delta, -kFeasMaxX, kFeasMaxX, low1, high1, last);
            xl = -kFeasMaxX; xh = kFeasMaxX;  // rob_box with bound = CVXPY_MAXX
            if (T.has_vel) {
                const double hcap = high1 < kEcosMaxX ? high1 : kEcosMaxX;
                xl = low1 > xl ? low1 : xl;
                xh = hcap < xh ? hcap : xh;
            }
            S.has_next = !last; S.n0 = -kFeasMaxX; S.n1 = kFeasMaxX; S.d2 = 2 * delta;
            const bool got = group_rob_x_interval<D, L>(S, xl, xh, lo, hi);
            if (writer) { X[2 * i] = got ? (lo < 0 ? 0 : lo) : qnan(); X[2 * i + 1] = got ? hi : qnan(); }
            s_i = s_nx;
            gi = gnx;
        }
        S.has_next = true;
    }

    // backward scan
    double kn0 = sd_end * sd_end, kn1 = kn0;
    if (writer) { K[2 * N] = kn0; K[2 * N + 1] = kn1; }
    bool failed = false;
    double s_n = grid[N];
    GridPt gn = T.locate(s_n);
    for (int i = N - 1; i >= 0; --i) {
        const double s_i = grid[i], delta = s_n - s_i;
        const GridPt gi = T.locate(s_i);
        double lo = 0, hi = 0;
        if (!failed) {
            double low1, high1, xl, xh;
            T.template build<false>(R, gl, gi, gn, delta, kn0, kn1, low1, high1);
            box(low1, high1, xl, xh);
            S.n0 = kn0; S.n1 = kn1; S.d2 = 2 * delta;
            if (isnan(kn0) || isnan(kn1) || !group_rob_x_interval<D, L>(S, xl, xh, lo, hi)) {
                lo = qnan(); hi = qnan();
                failed = true;
            } else {
                lo = lo < 0 ? 0 : lo;
                kn0 = lo; kn1 = hi;
            }
        }
        if (writer) { K[2 * i] = lo; K[2 * i + 1] = hi; }
        s_n = s_i;
        gn = gi;
    }
    const double x_start = sd_start * sd_start;
    if (failed || x_start + kPySmall < kn0 || kn1 + kPySmall < x_start) {
        if (writer) {
            for (int i = 0; i <= N; ++i) { if (xs) xs[i] = qnan(); if (sdv) sdv[i] = qnan(); }
            for (int i = 0; i < N; ++i) if (us) us[i] = qnan();
            if (A.status) A.status[bb] = TPR_STATUS_FAIL_UNCONTROLLABLE;
        }
        return;
    }
    __threadfence_block();

    // forward scan
    double x = x_start;
    double sq = sqrt(x);
    bool any_nan = isnan(sq);
    if (writer) { if (xs) xs[0] = x; if (sdv) sdv[0] = sq; }
    int tries = 0, i = 0;
    bool rows_ready = false;
    double delta = 0, k0 = 0, k1 = 0, low1 = 0, high1 = 0;
    GridPt gi = gn;
    double s_cur = s_n;
    while (i < N) {
        if (!rows_ready) {
            const double s_nx = grid[i + 1];
            k0 = K[2 * (i + 1)]; k1 = K[2 * (i + 1) + 1];
            delta = s_nx - s_cur;
            gn = T.locate(s_nx);
            T.template build<false>(R, gl, gi, gn, delta, k0, k1, low1, high1);
            s_cur = s_nx;
            rows_ready = true;
        }
        double uu = qnan();
        if (!isnan(x)) {
            double xl, xh, l, h;
            box(low1, high1, xl, xh);
            S.n0 = k0; S.n1 = k1; S.d2 = 2 * delta;
            if (xl <= x && x <= xh) {
                double vv;
                group_rob_u_interval<D, L>(S, x, l, h, vv);
                if (l <= h) uu = h;
            }
        }
        if (isnan(uu)) {
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
            if (writer) { if (us) us[i] = uu; if (xs) xs[i + 1] = x; if (sdv) sdv[i + 1] = sq; }
            any_nan |= isnan(sq);
            rows_ready = false;
            gi = gn;
            i += 1;
        }
    }
    if (writer && A.status) A.status[bb] = any_nan ? TPR_STATUS_ERR_UNKNOWN : TPR_STATUS_OK;
}

}  // namespace tpr

// tpr_wave.hip.inc -- kernel family 4: one trajectory per WAVE (the latency kernel).
//
// Families 2 and 3 are throughput designs: they need thousands of trajectories to fill the chip and a
// trajectory's 3N stage LPs crawl along on 1/8 (family 2) or 1/64 (family 3) of a wave.  A single
// trajectory (BASELINE config 1) or a few thousand (config 2) are bound by the LATENCY of that chain.
// Here the whole wave works on one trajectory:
//
//   * one constraint row per lane (vi = family 2's virtual row numbering: 0..3 box rows, 4,5 the x_next
//     pair, 6.. the acceleration rows; 4d + 6 <= 64 rows up to 14 dof, two / three register slots per
//     lane above -- the dof is a RUNTIME value, one instantiation per slot count serves every dof);
//   * per-trajectory scalars (the running vertex, K[i+1], warm-start pairs) are wave-uniform, rows are
//     fetched with v_readlane, and every "for all rows" test of the certificates is ONE compare per lane
//     plus a ballot -- no reductions on the common path;
//   * the chain-independent work (velocity box of every gridpoint with its 7 divisions, the norm bound
//     of the certificates) is done stage-parallel in a prologue, one gridpoint per lane, into LDS;
//   * K lives in LDS between the two scans and goes to HBM only if the caller asked for it; sd^2, u, sd
//     are staged in LDS and written with coalesced stores at the end.
//
// The certificates are those of family 2 (predict_lower_lp / predict_upper_lp in tpr_group.hip.inc: same
// conditions, same margins) applied to the WARM pair only -- the case in which the reference's own run is
// predictable end to end; a moved active pair, like anything else that does not certify, runs the
// reference's full Seidel iteration (wave_lp2d below == tpr::lp2d / group_lp2d decision for decision).
// Results are bit-identical to the reference either way.
//
// Reference map: reachability_algorithm.py:166-238 (backward), :240-376 (forward),
// time_optimal_algorithm.py:55-92, cy_seidel_solverwrapper.pyx:425-531 (rows), :549-697 (stage LP),
// :149-390 (solve_lp2d), :93-144 (solve_lp1d).

namespace tpr {

constexpr int kWaveBig = 0x3fffffff;

// A condition every lane agrees on, as a scalar branch condition (the compiler cannot see that a value
// computed identically in all lanes is uniform; cross-lane operations below need full-wave control flow).
__device__ __forceinline__ bool wave_any(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0; }

__device__ __forceinline__ int wave_uni(int x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ double wave_bcast(double x, int src_lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), src_lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src_lane);
    return __hiloint2double(hi, lo);
}

// ---- all-lanes reductions over the 64 lanes: 4 DPP steps inside a row of 16, then the two cross-row
// exchanges of gfx950 (v_permlane16_swap / v_permlane32_swap: VALU, no LDS round trip)
#define TPR_WAVE_REDUCE(NAME, T, TO_I, FROM_I, OP)                                                      \
    __device__ __forceinline__ T NAME(T x) {                                                            \
        { T y = FROM_I(dpp_i32<kDppXor1>(TO_I(x))); x = OP(x, y); }                                     \
        { T y = FROM_I(dpp_i32<kDppXor2>(TO_I(x))); x = OP(x, y); }                                     \
        { T y = FROM_I(dpp_i32<kDppHalfMirror>(TO_I(x))); x = OP(x, y); }                               \
        { T y = FROM_I(dpp_i32<kDppMirror>(TO_I(x))); x = OP(x, y); }                                   \
        { auto r = __builtin_amdgcn_permlane16_swap(TO_I(x), TO_I(x), false, false);                    \
          x = OP(FROM_I((int)r[0]), FROM_I((int)r[1])); }                                               \
        { auto r = __builtin_amdgcn_permlane32_swap(TO_I(x), TO_I(x), false, false);                    \
          x = OP(FROM_I((int)r[0]), FROM_I((int)r[1])); }                                               \
        return x;                                                                                       \
    }
#define TPR_ID(x) (x)
TPR_WAVE_REDUCE(wave_min_i32, int, TPR_ID, TPR_ID, TPR_MIN)
TPR_WAVE_REDUCE(wave_min_f32, float, __float_as_int, __int_as_float, TPR_MIN)
TPR_WAVE_REDUCE(wave_max_f32, float, __float_as_int, __int_as_float, TPR_MAX)
#undef TPR_ID

// exact fp64 minimum / maximum (operands are never NaN: callers select them from compared values)
#define TPR_WAVE_REDUCE64(NAME, OP)                                                                     \
    __device__ __forceinline__ double NAME(double x) {                                                  \
        { double y = dpp_f64<kDppXor1>(x); x = OP(x, y); }                                              \
        { double y = dpp_f64<kDppXor2>(x); x = OP(x, y); }                                              \
        { double y = dpp_f64<kDppHalfMirror>(x); x = OP(x, y); }                                        \
        { double y = dpp_f64<kDppMirror>(x); x = OP(x, y); }                                            \
        { auto a = __builtin_amdgcn_permlane16_swap(__double2loint(x), __double2loint(x), false, false);\
          auto b = __builtin_amdgcn_permlane16_swap(__double2hiint(x), __double2hiint(x), false, false);\
          x = OP(__hiloint2double((int)b[0], (int)a[0]), __hiloint2double((int)b[1], (int)a[1])); }     \
        { auto a = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(x), false, false);\
          auto b = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(x), false, false);\
          x = OP(__hiloint2double((int)b[0], (int)a[0]), __hiloint2double((int)b[1], (int)a[1])); }     \
        return x;                                                                                       \
    }
#define TPR_SELMIN(a, b) ((b) < (a) ? (b) : (a))
#define TPR_SELMAX(a, b) ((b) > (a) ? (b) : (a))
TPR_WAVE_REDUCE64(wave_min_f64, TPR_SELMIN)
TPR_WAVE_REDUCE64(wave_max_f64, TPR_SELMAX)

// ---- rows of a stage LP: S register slots per lane, virtual row vi = 64 s + lane
template <int S>
struct WaveRows {
    double a[S], b[S], c[S];
};

struct WaveLp {
    bool ok;
    double u, x;
    int ac0, ac1;  // reference row ids (box rows -1..-4)
};

// Row vi (wave-uniform index) as wave-uniform values.
template <int S>
__device__ __forceinline__ void wave_fetch(const WaveRows<S> &R, int vi, double &a, double &b, double &c) {
    const int src = vi & 63, slot = vi >> 6;
    double ra = R.a[0], rb = R.b[0], rc = R.c[0];
#pragma unroll
    for (int s = 1; s < S; ++s) {
        const bool hit = slot == s;  // uniform
        ra = hit ? R.a[s] : ra; rb = hit ? R.b[s] : rb; rc = hit ? R.c[s] : rc;
    }
    a = wave_bcast(ra, src); b = wave_bcast(rb, src); c = wave_bcast(rc, src);
}

// First virtual row whose predicate holds (-1: none).  pred[s] is per lane.
template <int S>
__device__ __forceinline__ int wave_first(const bool (&pred)[S]) {
    int vi = -1;
#pragma unroll
    for (int s = S - 1; s >= 0; --s) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(pred[s]);
        if (m != 0) vi = 64 * s + (int)__builtin_ctzll(m);
    }
    return vi;
}

template <int S>
__device__ __forceinline__ bool wave_any_slot(const bool (&pred)[S]) {
    bool any = false;
#pragma unroll
    for (int s = 0; s < S; ++s) any |= pred[s];
    return __builtin_amdgcn_ballot_w64(any) != 0;
}

// Row with the smallest key (+inf = not a candidate); -1 when there is none.  fp32 keys: this is only
// ever used to SEARCH (the winner is certified afterwards or the LP goes to the full iteration).
template <int S>
__device__ __forceinline__ int wave_argmin(const float (&key)[S]) {
    float best = key[0];
    int bs = 0;
#pragma unroll
    for (int s = 1; s < S; ++s) { const bool lt = key[s] < best; best = lt ? key[s] : best; bs = lt ? s : bs; }
    const float m = wave_min_f32(best);
    const unsigned long long hit = __builtin_amdgcn_ballot_w64((best == m) & (best < 3.0e38f));
    if (hit == 0) return -1;
    const int src = (int)__builtin_ctzll(hit);
    return 64 * __builtin_amdgcn_readlane(bs, src) + src;
}

// Position of structural row r (reference id) in the reference's visiting order for warm start (w0, w1):
// [w1, w0, the rest ascending] when both are structural rows and distinct, else the identity
// (cy_seidel_solverwrapper.pyx:253-264).
__device__ __forceinline__ int wave_order_pos(int r, int w0, int w1, bool warm) {
    return !warm ? r : (r == w1 ? 0 : (r == w0 ? 1 : 2 + r - (r > w0 ? 1 : 0) - (r > w1 ? 1 : 0)));
}

// The reference's full Seidel iteration on the wave's rows: decision for decision tpr::lp2d (tpr_device.hpp) /
// group_lp2d (tpr_group.hip.inc).  Rows vi 0..3 hold the box (-1,0,low0) (1,0,-high0) (0,-1,low1) (0,1,-high1);
// nC = structural rows (vi 4 .. nC+3); slots past nC + 4 hold anything (they are masked).
template <int S>
__device__ inline WaveLp wave_lp2d(const WaveRows<S> &R, int nC, int lane, double v0, double v1, double low0,
                                   double high0, double low1, double high1, int wac0, int wac1) {
    WaveLp o;
    o.ok = false; o.u = qnan(); o.x = qnan(); o.ac0 = 0; o.ac1 = 0;
    const int nV = nC + 4;
    const bool active = !(low0 > high0) && !(low1 > high1);
    double cu, cx;
    if (v0 > kTiny) { cu = high0; o.ac0 = -2; } else { cu = low0; o.ac0 = -1; }
    if (v1 > kTiny) { cx = high1; o.ac1 = -4; } else { cx = low1; o.ac1 = -3; }
    const bool warm = wac0 >= 0 && wac0 < nC && wac1 >= 0 && wac1 < nC && wac0 != wac1;
    int pos[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int vi = 64 * s + lane;
        int p = wave_order_pos(vi - 4, wac0, wac1, warm);
        if (vi < 4) p = -1;          // box rows: projected in every pass, never pivots
        if (vi >= nV) p = kWaveBig;  // no row
        pos[s] = p;
    }
    int kpos = -1, pivot_vi = -1, want = 0;
    double T = 0;
    double ts[S];
    int cls[S];  // 0 = not a candidate, 1 = upper bound on t, 2 = lower bound on t
#pragma unroll
    for (int s = 0; s < S; ++s) { ts[s] = 0; cls[s] = 0; }
    bool success = false;
    while (wave_any(active)) {
        // first violated structural row after position kpos, in the reference's order
        int key = kWaveBig;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const double val = R.a[s] * cu + R.b[s] * cx + R.c[s];
            const bool viol = (pos[s] > kpos) & (pos[s] < kWaveBig) & !(val < kTiny);
            const int cand = viol ? pos[s] * 256 + (64 * s + lane) : kWaveBig;
            key = cand < key ? cand : key;
        }
        key = wave_uni(wave_min_i32(key));
        if (key == kWaveBig) { success = true; break; }
        const int k = key >> 8;
        pivot_vi = key & 255;
        double pa, pb, pc;
        wave_fetch<S>(R, pivot_vi, pa, pb, pc);
        const double den = pa * pa + pb * pb;
        if (wave_any(den == 0.0)) break;  // the reference raises ZeroDivisionError
        const double zp0 = (-pa * pc) / den;
        const double zp1 = (-pb * pc) / den;
        const double dt0 = -pb, dt1 = pa;
        const double v1d = dt0 * v0 + dt1 * v1;
        // project the rows at positions < k and the box rows onto the pivot line
        double tmax = kInf1d, tmin = -kInf1d;
        bool par_bad = false;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const bool need = pos[s] < k;  // box rows have pos -1
            const double denom = dt0 * R.a[s] + dt1 * R.b[s];
            const double num = R.c[s] + zp1 * R.b[s] + zp0 * R.a[s];
            const double t = -num / denom;
            const bool up = need & (denom > kTiny);
            const bool lo = need & (denom < -kTiny);
            ts[s] = t;
            cls[s] = up ? 1 : (lo ? 2 : 0);
            tmax = (up & (t < tmax)) ? t : tmax;
            tmin = (lo & (t > tmin)) ? t : tmin;
            par_bad |= need & !up & !lo & (num > kSmall);
        }
        const double gmax = wave_min_f64(tmax);
        const double gmin = wave_max_f64(tmin);
        if (wave_any(par_bad) || wave_any(gmin > gmax)) break;
        const bool pick_min = fabs(v1d) < kTiny || v1d < 0;
        T = pick_min ? gmin : gmax;
        want = pick_min ? 2 : 1;
        // the +-1e10 line bounds being active is "infeasible" in the reference (:366-383)
        if (wave_any(pick_min ? !(T > -kInf1d) : !(T < kInf1d))) break;
        cu = zp0 + T * dt0;
        cx = zp1 + T * dt1;
        kpos = k;
    }
    if (success) {
        o.ok = true; o.u = cu; o.x = cx;
        if (pivot_vi >= 0) {
            // active set of the last pivot: the pivot row, and the row attaining T in its 1-D LP (smallest order
            // index among ties; box rows sort after every structural row, in the order low0, high0, low1, high1)
            int akey = kWaveBig;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int vi = 64 * s + lane;
                const int j = vi < 4 ? nC + vi : pos[s];
                const int cand = (cls[s] == want && ts[s] == T) ? (j << 10) + ((row_id_of(vi) + 8) & 0x3ff) : kWaveBig;
                akey = cand < akey ? cand : akey;
            }
            akey = wave_uni(wave_min_i32(akey));
            o.ac0 = pivot_vi - 4;
            o.ac1 = (akey & 0x3ff) - 8;
        }
    }
    return o;
}

// Stage constants the certificates share.
struct WaveStage {
    int nC, lane;
    double low1, high1;
    double norm_bound;  // >= |a| + |b| of every row of the trajectory (prologue)
    double limit_min;   // min over the dofs of min(amax, -amin): a floor of -c over the acceleration rows (prologue)
    double two_delta, n0, n1;  // the stage's x_next rows as scalars (wave_lower_trace)
    bool norms_ok;      // every row of the stage is null or longer than 0.05 in 1-norm (computed with the rows)
    bool stage_ok;      // norms_ok, low1 <= high1, norm_bound < 1e6, finite limits: what the lean certificates share
    unsigned long long rows[3];  // per slot: the lanes that hold a row (vi < nC + 4)
};

// The lean certificates express their per-row tests as SIGN BITS (a value that must be negative) and combine them
// with integer AND / OR on the high words: one instruction per test instead of a compare into a lane mask plus a
// scalar mask operation -- a lone wave issues one instruction of any kind every ~5 cycles, so the certificate costs
// its instruction count.  NaNs cannot slip through as "negative": rows, limits and K are finite where these run
// (WaveStage::stage_ok, the trajectory-wide norm bound, the scans' own NaN checks), and a NaN produced on the way
// (0 * inf cannot occur with finite operands; inf - inf gives the canonical positive quiet NaN) has its sign clear.
__device__ __forceinline__ int hi32(double x) { return __double2hiint(x); }
// "|cross| is exactly 0 (or denormal: the solver takes its |.| < 1e-10 branch just the same) or clearly above 1e-7", on
// the high word: (hi & 0x7fffffff) - 1 wraps for a zero high word and must otherwise reach the high word past 1e-7
constexpr unsigned kCrossKeyMin = 0x3e7ad7f2u + 1u;
__device__ __forceinline__ bool cross_bad(double cross) {
    return (((unsigned)hi32(cross) & 0x7fffffffu) - 1u) < kCrossKeyMin - 1u;
}
// bit of virtual row vi in slot s's lane mask (0 when the row lives in another slot)
template <int S>
__device__ __forceinline__ unsigned long long wave_row_bit(int vi, int s) {
    if (S == 1) return 1ull << vi;  // (every row lives in slot 0)
    return (vi >> 6) == s ? 1ull << (vi & 63) : 0ull;
}

// Certificate of the WARM pair of the upper-bound LP -- the previous stage's active set (k, l) = (ac0, ac1): k is the
// row the reference pivoted on last (a structural row, vi >= 4), l the row that limited it.  With that pair as warm
// start the reference visits l first and k second (cy_seidel_solverwrapper.pyx:253-264; a box row l never pivots), so
// if the pair is still the optimum the last pivot is k limited by l again and no order logic is needed.  Conditions as
// wave_cert_pair (which handles arbitrary pairs for the proposal), tests as sign bits.  `valid`: the caller's verdict
// on (k, l) -- when false any valid row numbers are passed and the certificate fails.
template <int S>
__device__ __forceinline__ bool wave_cert_warm(const WaveRows<S> &R, const WaveStage &G, double v0, double v1, int k, int l,
                                               bool valid, WaveLp &o, double (&vert)[4], bool &pair_ok) {
    constexpr double kSlack = TPR_SLACK_ABS, kRelSlack = TPR_SLACK_REL;
    double ka, kb, kc, la, lb, lc;
    wave_fetch<S>(R, k, ka, kb, kc);
    wave_fetch<S>(R, l, la, lb, lc);
    const double Dm = ka * lb - la * kb;  // == the last pivot's denominator (-kb) la + ka lb, bit for bit
    const double rD = rcp_approx(Dm);     // the vertex only feeds margin tests and searches
    const double u = (kb * lc - lb * kc) * rD;
    const double x = (la * kc - ka * lc) * rD;
    const double v1d = -kb * v0 + ka * v1;
    const double lamk = (v0 * lb - v1 * la) * rD, laml = v1d * rD;  // v = lamk n_k + laml n_l
    vert[0] = u; vert[1] = x; vert[2] = lamk; vert[3] = laml;
    pair_ok = fabs(Dm) > 1e-7;
    const bool ok = valid & pair_ok & (lamk > 0) & (laml > 0) & (fabs(v1d) > 1e-6) & G.stage_ok;
    const double thr = 1e-8 * (G.norm_bound * (fabs(la) + fabs(lb)));
    const double aDm = fabs(Dm);
    unsigned long long badbits = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const double au = R.a[s] * u, bx = R.b[s] * x;
        const double res = au + bx + R.c[s];
        const double sc = res + __builtin_fma(kRelSlack, fabs(au) + fabs(bx) + fabs(R.c[s]), kSlack);  // (A) < 0
        const double w = __builtin_fma(aDm, res, thr);                                                   // (B) < 0
        const unsigned long long m_ab = __builtin_amdgcn_ballot_w64((hi32(sc) & hi32(w)) >= 0);
        const unsigned long long m_c = __builtin_amdgcn_ballot_w64(cross_bad(ka * R.b[s] - kb * R.a[s]));  // (C)
        badbits |= ((m_ab & ~(wave_row_bit<S>(k, s) | wave_row_bit<S>(l, s))) | m_c) & G.rows[s];
    }
    // the reference's arithmetic for (pivot k, limiter l): cy_seidel_solverwrapper.pyx:287-364 (beside the scan)
    const double den = ka * ka + kb * kb;
    const double zp0 = (-ka * kc) / den;
    const double zp1 = (-kb * kc) / den;
    const double num = lc + zp1 * lb + zp0 * la;
    const double T = -num / Dm;
    const bool good = (__builtin_amdgcn_ballot_w64(!ok) | badbits) == 0;  // (a scalar: what follows is scalar control flow)
    o.ok = good;
    o.u = zp0 + T * -kb;
    o.x = zp1 + T * ka;
    o.ac0 = row_id_of(k);
    o.ac1 = row_id_of(l);
    return good;
}

// Certificate for "rows (p, q) -- virtual row numbers, not both box rows -- are the unique, well separated optimal
// vertex of max v0 u + v1 x": predict_upper_lp's verdict (tpr_group.hip.inc) on a given pair, rows across the 64
// lanes.  The reference's result is then a function of its LAST pivot only -- the later of the two rows in its
// visiting order, limited by the other -- and is evaluated with the reference's own formulas.  Conditions and
// margins are family 2's; the two reductions it needs (largest residual, largest row norm) are replaced by one
// test per lane against the trajectory-wide norm bound, which is stricter.
// vert[4] returns the pair's vertex and multipliers (u, x, lam_p, lam_q) for the proposal that follows a refusal.
template <int S>
__device__ __forceinline__ bool wave_cert_pair(const WaveRows<S> &R, const WaveStage &G, double v0, double v1, int p, int q,
                                               int wac0, int wac1, WaveLp &o, double (&vert)[4], bool &pair_ok) {
    constexpr double kSlack = TPR_SLACK_ABS, kRelSlack = TPR_SLACK_REL;
    const int nC = G.nC, nV = nC + 4, lane = G.lane;
    double pa, pb, pc, qa, qb, qc;
    wave_fetch<S>(R, p, pa, pb, pc);
    wave_fetch<S>(R, q, qa, qb, qc);
    const double Dm = pa * qb - qa * pb;
    bool ok = fabs(Dm) > 1e-7;
    const double rD = rcp_approx(Dm);  // the vertex only feeds margin tests and searches
    const double u = (pb * qc - qb * pc) * rD;
    const double x = (qa * pc - pa * qc) * rD;
    const double lamp = (v0 * qb - v1 * qa) * rD, lamq = (pa * v1 - pb * v0) * rD;  // v = lamp n_p + lamq n_q
    vert[0] = u; vert[1] = x; vert[2] = lamp; vert[3] = lamq;
    pair_ok = ok;
    ok &= (lamp > 0) & (lamq > 0) & (G.low1 <= G.high1) & !((p < 4) & (q < 4)) & (G.norm_bound < 1e6) & G.norms_ok;
    // roles in the reference's last pivot: the later row in its order is the pivot (box rows never are)
    const bool warm = wac0 >= 0 && wac0 < nC && wac1 >= 0 && wac1 < nC;  // (wac0 != wac1: the caller's precondition)
    const int pp = p >= 4 ? wave_order_pos(p - 4, wac0, wac1, warm) : -1;
    const int pq = q >= 4 ? wave_order_pos(q - 4, wac0, wac1, warm) : -1;
    const bool p_pivot = pp > pq;
    const int k = p_pivot ? p : q, l = p_pivot ? q : p;
    const double ka = p_pivot ? pa : qa, kb = p_pivot ? pb : qb, kc = p_pivot ? pc : qc;
    const double la = p_pivot ? qa : pa, lb = p_pivot ? qb : pb, lc = p_pivot ? qc : pc;
    const double v1d = -kb * v0 + ka * v1;
    ok &= fabs(v1d) > 1e-6;
    // (B) the pivot row is violated by >= 1e-8 at the optimum of the rows before it: |D| m / (max|n| |n_l|) with m the
    // smallest margin of the other rows -- tested row by row against the norm bound
    const double thr = 1e-8 * (G.norm_bound * (fabs(la) + fabs(lb)));
    const double aDm = fabs(Dm);
    bool bad = !ok;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int vi = 64 * s + lane;
        const bool row = vi < nV;
        const bool other = row & (vi != p) & (vi != q);
        const double au = R.a[s] * u, bx = R.b[s] * x;
        const double res = au + bx + R.c[s];
        const double sc = res + (kSlack + kRelSlack * (fabs(au) + fabs(bx) + fabs(R.c[s])));
        bad |= other & !(sc < 0);                  // (A) every other row holds with a margin
        bad |= other & !(aDm * (-res) > thr);      // (B)
        const double cross = ka * R.b[s] - kb * R.a[s];
        bad |= row & (vi != k) & (cross != 0.0) & !(fabs(cross) > 1e-7);  // (C) nothing almost parallel to the pivot row
    }
    // the reference's arithmetic for (pivot k, limiter l): cy_seidel_solverwrapper.pyx:287-364.  Evaluated whether
    // or not the certificate holds (straight-line code: its two dependent divisions run beside the residual scan)
    const double den = ka * ka + kb * kb;
    const double zp0 = (-ka * kc) / den;
    const double zp1 = (-kb * kc) / den;
    const double dt0 = -kb, dt1 = ka;
    const double denom = dt0 * la + dt1 * lb;
    const double num = lc + zp1 * lb + zp0 * la;
    const double T = -num / denom;
    const bool good = __builtin_amdgcn_ballot_w64(bad) == 0;
    o.ok = good;
    o.u = zp0 + T * dt0;
    o.x = zp1 + T * dt1;
    o.ac0 = row_id_of(k);
    o.ac1 = row_id_of(l);
    return good;
}

// Inclusive prefix minimum over the 64 lanes in lane order (Hillis-Steele inside the rows of 16 with DPP row shifts,
// then the two row broadcasts of gfx9): the running record of a cold lower-bound run, whose rows sit in the lanes in
// visiting order.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64_or_top(double v) {  // lanes without a source (or outside ROW_MASK) read +3e300
    constexpr double kTop = 3.0e300;
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(kTop), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(kTop), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_prefix_min_f64(double x) {
    x = fmin(x, dpp_f64_or_top<0x111, 0xf>(x));  // row_shr:1
    x = fmin(x, dpp_f64_or_top<0x112, 0xf>(x));  // row_shr:2
    x = fmin(x, dpp_f64_or_top<0x114, 0xf>(x));  // row_shr:4
    x = fmin(x, dpp_f64_or_top<0x118, 0xf>(x));  // row_shr:8
    x = fmin(x, dpp_f64_or_top<0x142, 0xa>(x));  // row_bcast:15 into rows 1, 3
    x = fmin(x, dpp_f64_or_top<0x143, 0xc>(x));  // row_bcast:31 into rows 2, 3
    return x;
}

// The TRACE of the lower-bound LP (round 4; tpr_cert_lane.hip.inc, cert_lower_sound, for rows across the lanes of a wave):
// the certificate below verifies the final vertex; the reference reaches it through a cold run -- the x_next row the start
// corner (1e8, low1) violates pivots against the box and lands on the wall x = low1 at u0, then every row that bounds u
// more tightly than the running record pivots in turn, limited by the wall -- and each of those pivots must be
// predictable: a clear verdict where a row is visited (|a M + g| > tol at the running record M, g = b low1 + c), and for a
// new record a clearly signed 1-D objective on its line and the previous record holding at its vertex with a margin (the
// previous record's slope is (-g_prev) / M; a per-trajectory floor of -g stands in for it: no reduction per stage).  The rows sit in
// the lanes in visiting order, so the running record is an exclusive prefix minimum.  r_vi: the row the certificate names.
template <int S>
__device__ __forceinline__ bool wave_lower_trace(const WaveRows<S> &R, const WaveStage &G, int r_vi) {
    constexpr double kSlack = TPR_SLACK_ABS, kTraceRel = 1e-12, kTop = 3.0e300;
    const double low1 = G.low1;
    const double d2 = G.two_delta, n0 = G.n0, n1 = G.n1;
    // prologue: the corner's verdicts on the two x_next rows, the pivot of the violated one onto the wall
    const double nb45 = 1.0 + d2;  // |a| + |b| of the x_next rows: all the prologue touches
    const double tol_c = kSlack + kTraceRel * (nb45 * (kVarMax + fabs(low1)) + fabs(n0) + fabs(n1));
    bool ok = (-d2 * kVarMax + (n0 - low1) < -tol_c) & (d2 * kVarMax + (low1 - n1) > tol_c) & (d2 > 1e-6) &
              (G.high1 - low1 > 1e-6 * (1.0 + fabs(G.high1) + fabs(low1)));
    const double u0 = (n1 - low1) * rcp_approx(d2);
    ok &= fabs(u0) < kVarMax * (1.0 - 1e-6);
    const double tol0 = kSlack + kTraceRel * (nb45 * (fabs(u0) + fabs(low1)) + fabs(n0) + fabs(n1));
    ok &= n0 - n1 < -tol0;
    // the rows' bounds on u at the wall, in visiting order
    const int nV = G.nC + 4;
    double t[S], g[S];
    bool push[S];
    // a floor of -g = -(b low1 + c) over the rows that can be records: the previous record's slope is (-g_prev) / M, which
    // stands in for it in the margin test below (no reduction per stage)
    const double mg_lo = G.limit_min - G.norm_bound * fabs(low1);  // (the first record's predecessor is the x_next row: slope 2 delta)
    ok &= mg_lo > 0.0;
    bool bad = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int vi = 64 * s + G.lane;
        const bool row = (vi >= 6) & (vi < nV);
        g[s] = R.b[s] * low1 + R.c[s];
        push[s] = row & (R.a[s] > 1e-7);
        t[s] = push[s] ? -g[s] * rcp_approx(R.a[s]) : kTop;
        // a row that rises with u by less than the solver can tell from 0 must simply hold at u0
        bad |= row & (R.a[s] > 0.0) & !push[s] & !(R.a[s] * u0 + g[s] < -tol0);
    }
    double carry = u0, tmin = kTop;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const double inc = wave_prefix_min_f64(t[s]);
        // exclusive: the lanes before this one in the slot, and everything before the slot
        const double M = fmin(carry, dpp_f64_or_top<0x138, 0xf>(inc));  // wave_shr:1
        const double r = R.a[s] * M + g[s];                       // the row's residual where it is visited
        const double tol = kSlack + kTraceRel * (fabs(R.a[s] * M) + fabs(R.b[s] * low1) + fabs(R.c[s]));
        const bool viol = r > tol;
        bad |= push[s] & !viol & !(r < -tol);
        // a new record: dual feasible vertex with the wall, the previous record holding there with a margin
        const bool prev_ok = M >= u0 ? d2 * (M - t[s]) > 1e-2 * tol : mg_lo * (M - t[s]) > 1e-2 * tol * M;
        bad |= push[s] & viol & !((R.a[s] + 1e-9 * R.b[s] > 1e-6) & prev_ok);
        const double last = wave_bcast(inc, 63);
        carry = fmin(carry, last);
        tmin = fmin(tmin, last);
    }
    // the last record is the row the certificate is about
    double tr = t[0];
#pragma unroll
    for (int s = 1; s < S; ++s) tr = (r_vi >> 6) == s ? t[s] : tr;
    const double t_r = wave_bcast(tr, r_vi & 63);
    ok &= (r_vi >= 6) ? (t_r == tmin) & (tmin < u0) : !(tmin < u0);
    return ok & (__builtin_amdgcn_ballot_w64(bad) == 0);
}

// Lower-bound LP of a backward stage (max 1e-9 u - x) from the vertex "x on its box bound, u on row r": predict_lower_lp
// (tpr_group.hip.inc) for a given r -- that every other row holds at the vertex with a margin also proves r to be the
// tightest bound on u, so the previous stage's r is simply tried first.
template <int S>
__device__ __forceinline__ bool wave_cert_lower(const WaveRows<S> &R, const WaveStage &G, int r_vi, bool valid, double low0,
                                                double high0, WaveLp &o) {
    constexpr double kSlack = TPR_SLACK_ABS, kRelSlack = TPR_SLACK_REL;
    static_assert(kVarMin == -kVarMax, "one test for both ends of the u box");
    const double low1 = G.low1;
    double pa, pb, pc;
    wave_fetch<S>(R, r_vi, pa, pb, pc);
    const double u1 = -(pb * low1 + pc) * rcp_approx(pa);
    // the pivot row itself: well conditioned, u inside its box, and the tilt (1e-9) must not make a larger x worthwhile
    const bool ok = valid & (pa > 1e-6) & (fabs(u1) < high0 - 1.0) & (pb > -1e8 * pa) & (fabs(pc) < 1e15) & G.stage_ok;
    (void)low0;
    unsigned long long badbits = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const double au = R.a[s] * u1, bl = R.b[s] * low1;
        const double val = au + (bl + R.c[s]);
        const double sc = val + __builtin_fma(kRelSlack, fabs(au) + fabs(bl) + fabs(R.c[s]), kSlack);  // < 0: holds with a margin
        const unsigned long long m_a = __builtin_amdgcn_ballot_w64(hi32(sc) >= 0);
        const unsigned long long m_c = __builtin_amdgcn_ballot_w64(cross_bad(pa * R.b[s] - pb * R.a[s]));
        // structural rows only (vi >= 4); the row itself is exactly parallel to itself and is left out of the margin test
        badbits |= ((m_a & ~wave_row_bit<S>(r_vi, s)) | m_c) & G.rows[s] & (s == 0 ? ~0xfull : ~0ull);
    }
    // the reference's arithmetic for (pivot r, limiter = box row x >= low1), beside the scan
    const double den = pa * pa + pb * pb;
    const double zp0 = (-pa * pc) / den;
    const double zp1 = (-pb * pc) / den;
    const double dt0 = -pb, dt1 = pa;
    const double denom = dt0 * 0.0 + dt1 * -1.0;
    const double num = low1 + zp1 * -1.0 + zp0 * 0.0;
    const double T = -num / denom;
    const bool trace_ok = wave_lower_trace<S>(R, G, r_vi);  // round 4: every pivot of the reference's run, not only its last
    const bool good = ((__builtin_amdgcn_ballot_w64(!ok) | badbits) == 0) & trace_ok;  // (a scalar: what follows is scalar control flow)
    o.ok = good;
    o.u = zp0 + T * dt0;
    o.x = zp1 + T * dt1;
    o.ac0 = r_vi - 4;
    o.ac1 = -3;
    return good;
}

// The tightest upper bound on u at x = low1 (a search: fp32 keys, reciprocal estimate).
template <int S>
__device__ __forceinline__ int wave_lower_search(const WaveRows<S> &R, const WaveStage &G) {
    const int nV = G.nC + 4;
    float key[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int vi = 64 * s + G.lane;
        const bool cand = (vi >= 4) & (vi < nV) & (R.a[s] > 0.0);
        key[s] = cand ? (float)(-(R.b[s] * G.low1 + R.c[s]) * rcp_approx(R.a[s])) : 3.4e38f;
    }
    return wave_argmin<S>(key);
}

// 1-D LP of the forward pass: max v0 u  s.t.  a u + (b x + c) <= 0 over the structural rows, low0 <= u <= high0
// (cy_seidel_solverwrapper.pyx:93-144 through :631-650).  The quotients are the reference's; their exact minimum is
// first looked for at the row that attained it at the previous stage (`guess`, updated) -- one compare per lane and a
// ballot -- before the exact reduction.
// want_active: also return the reference's solution.active_c[0] -- the first row (in index order) that attains the
// optimum, -2 / -1 when it is the box (cy_seidel_solverwrapper.pyx:103-142) -- which the 1-D path writes into the
// wrapper's warm-start state (:646-649).
template <int S>
__device__ __forceinline__ bool wave_lp1d(const WaveRows<S> &R, int nC, int lane, double v0, double x, double low0,
                                          double high0, int &guess, double &u_out, bool want_active, int &active) {
    const int nV = nC + 4;
    double t[S];
    bool up[S], lo[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int vi = 64 * s + lane;
        const bool need = (vi >= 4) & (vi < nV);
        const double bxc = R.b[s] * x + R.c[s];
        t[s] = -bxc / R.a[s];
        up[s] = need & (R.a[s] > kTiny);
        lo[s] = need & (R.a[s] < -kTiny);
    }
    // tmax = min(high0, min over the upper-bound rows)
    double cand = high0;
    if (guess >= 0) {
        double tg = t[0];
        bool ug = up[0];
#pragma unroll
        for (int s = 1; s < S; ++s) { const bool hit = (guess >> 6) == s; tg = hit ? t[s] : tg; ug = hit ? up[s] : ug; }
        const bool valid = (__builtin_amdgcn_ballot_w64(ug) >> (guess & 63)) & 1;
        const double tb = wave_bcast(tg, guess & 63);
        cand = (valid && tb < high0) ? tb : high0;
    }
    bool below[S];
#pragma unroll
    for (int s = 0; s < S; ++s) below[s] = up[s] & (t[s] < cand);
    double tmax = cand;
    if (wave_any_slot<S>(below)) {  // the binding row moved: exact minimum, and who attains it
        double m = high0;
#pragma unroll
        for (int s = 0; s < S; ++s) m = (up[s] & (t[s] < m)) ? t[s] : m;
        tmax = wave_min_f64(m);
        bool hit[S];
#pragma unroll
        for (int s = 0; s < S; ++s) hit[s] = up[s] & (t[s] == tmax);
        guess = wave_first<S>(hit);
    }
    const bool pick_min = fabs(v0) < kTiny || v0 < 0;
    if (wave_any(pick_min)) {  // (a vanishing grid interval: the answer is the largest lower bound)
        double m = low0;
#pragma unroll
        for (int s = 0; s < S; ++s) m = (lo[s] & (t[s] > m)) ? t[s] : m;
        const double tmin = wave_max_f64(m);
        if (wave_any(tmin > tmax)) return false;
        u_out = tmin;
        if (want_active) {
            bool hit[S];
#pragma unroll
            for (int s = 0; s < S; ++s) hit[s] = lo[s] & (t[s] == tmin) & (tmin > low0);
            const int r = wave_first<S>(hit);
            active = r >= 0 ? r - 4 : -1;
        }
        return true;
    }
    bool above[S];
#pragma unroll
    for (int s = 0; s < S; ++s) above[s] = lo[s] & (t[s] > tmax);
    if (wave_any_slot<S>(above) || wave_any(low0 > tmax)) return false;  // cur_min > cur_max
    u_out = tmax;
    if (want_active) {
        bool hit[S];
#pragma unroll
        for (int s = 0; s < S; ++s) hit[s] = up[s] & (t[s] == tmax) & (tmax < high0);
        const int r = wave_first<S>(hit);
        active = r >= 0 ? r - 4 : -2;
    }
    return true;
}

// LDS of one trajectory, in doubles: one record {s_j, low1_j, high1_j, K_lo_j, K_hi_j} per gridpoint (the x box from
// the velocity limits; the forward scan reuses its two fields as output staging for sd2_j, u_j), the velocity
// limits, two 16-bit arrays (the spline segment of every gridpoint, and the gridpoints after which the segment
// changes), then the spline table (c0, c1, c2 per segment and dof) and the breakpoints when they fit.
// 10 240 bytes let 16 blocks share a CU (four waves per SIMD): N = 200, d = 7 takes 9.7 KB.
constexpr int kWaveRec = 5;
__host__ __device__ inline size_t wave_lds_doubles(int N, int nseg, int d, bool table_in_lds) {
    return (size_t)kWaveRec * (N + 1) + 2 * d + (size_t)(2 * (N + 1) + 3) / 4 + (table_in_lds ? (size_t)3 * nseg * d + (nseg + 1) : 0);
}


// SPLIT (round 6): TWO waves per trajectory for a handful of trajectories (BASELINE config 1) -- the two LPs of a backward stage
// (reachability_algorithm.py:229-236) depend only on K[i+1], so wave 0 answers the upper-bound LP and wave 1 the lower-bound LP
// of the same stage side by side, each with its own copy of the rows and its own half of the wrapper's warm-start state; the
// two bounds meet in LDS behind one block barrier per stage.  A lone wave issues an instruction every ~5 cycles whatever it is,
// so the backward scan's time is its instruction count per wave, and that count drops from both certificates to the longer of
// the two.  The forward scan (one LP per stage) runs on wave 0 alone.  Not for feasible sets (launch_wave never asks).
template <int S, bool TABLE_LDS, bool SPLIT = false>
__global__ void __launch_bounds__(SPLIT ? 128 : 64) wave_solve_kernel(BatchArgs A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x & 63;
    const int wv = SPLIT ? (int)(threadIdx.x >> 6) : 0;
    const bool do_u = !SPLIT || wv == 0, do_l = !SPLIT || wv == 1;  // which of a backward stage's LPs this wave answers
    const int bb = blockIdx.x;
    const int N = A.N, nseg = A.nseg, d = A.d;
    const bool has_vel = A.flags & TPR_HAS_VELOCITY;
    const int nblk = (A.flags & TPR_HAS_ACCELERATION) ? ((A.flags & TPR_ACC_INTERPOLATION) ? 4 : 2) : 0;
    const int nC = 2 + 4 * d;  // slot layout of the Interpolation row set; missing blocks hold the disabled row (0, 0, -1)
    const int nV = nC + 4;
    // per-gridpoint records: [0] s_j, [1] low1_j (forward scan: sd2_j), [2] high1_j (forward scan: u_j), [3] K_lo, [4] K_hi
    double *P = lds;
    double *lvl = P + kWaveRec * (N + 1);                                        // [d][2] velocity limits
    unsigned short *sgi = reinterpret_cast<unsigned short *>(lvl + 2 * d);      // [N+1] spline segment of every gridpoint
    unsigned short *chg = sgi + (N + 1);                                         // [<= N] j with segment(j) != segment(j+1), ascending
    const double *gcf = A.coef + (size_t)bb * 4 * nseg * d;
    const double *gbrk = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? (size_t)bb * (nseg + 1) : 0);
    const double *ggrid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)bb * (N + 1) : 0);
    const double *cf = gcf, *brk = gbrk;
    // (every global input is fetched once, by coalesced loads issued together: with host-mapped inputs -- the
    // small-call path of tpr_solve_batch -- each dependent access would be a PCIe round trip)
    if (TABLE_LDS) {
        double *lcf = lvl + 2 * d + (2 * (N + 1) + 3) / 4, *lbrk = lcf + 3 * nseg * d;
        for (int e = lane; e < 3 * nseg * d; e += 64) lcf[e] = gcf[e];
        for (int e = lane; e <= nseg; e += 64) lbrk[e] = gbrk[e];
        cf = lcf;
        brk = lbrk;
    }
    for (int e = lane; e <= N; e += 64) P[kWaveRec * e] = ggrid[e];
    if (has_vel) for (int e = lane; e < 2 * d; e += 64) lvl[e] = A.vlim[(size_t)bb * 2 * d + e];
    const double sd_start = A.sd_start ? A.sd_start[bb] : 0.0;
    const double sd_end = A.sd_end ? A.sd_end[bb] : 0.0;
    const double sd_end_hi = A.sd_end_hi ? A.sd_end_hi[bb] : sd_end;
    __syncthreads();

    // ---- prologue: everything that does not depend on the scans, one gridpoint per lane -----------------
    double dmax = 0.0;
    for (int j = lane; j < N; j += 64) { const double dj = P[kWaveRec * (j + 1)] - P[kWaveRec * j]; dmax = dj > dmax ? dj : dmax; }
    dmax = wave_max_f64(dmax);
    const double wq2 = 1.0 + 2.0 * dmax;  // |q' + 2 delta q''| + |q''| <= |q'| + wq2 |q''|
    double nb = wq2;                       // x_next rows: 2 delta + 1; box rows: 1
    const double *vlim = lvl;
    for (int j = lane; j <= N; j += 64) {
        const double s = P[kWaveRec * j];
        const int seg = find_segment(brk, nseg, s);
        sgi[j] = (unsigned short)seg;
        const double t = s - brk[seg];
        double mmax = (double)kJvelMaxSd;
        bool pos_lower = false;
        for (int k = 0; k < d; ++k) {
            double q1, q2;
            cubic_d1_d2(cf[(0 * nseg + seg) * d + k], cf[(1 * nseg + seg) * d + k], cf[(2 * nseg + seg) * d + k], t, q1, q2);
            const double n1 = fabs(q1) + wq2 * fabs(q2);
            nb = n1 > nb ? n1 : nb;
            if (has_vel) {
                // _create_velocity_constraint: sdmax / sdmin are C floats updated dof by dof; rounding to fp32 is
                // monotone, so the running fp32 minimum equals the fp64 minimum rounded once (as in families 2, 3)
                const double vlo = vlim[2 * k], vhi = vlim[2 * k + 1];
                const bool valid = (q1 != 0) & !isnan(q1);
                const double rmax = (q1 > 0 ? vhi : vlo) / q1;
                mmax = (valid & (rmax <= mmax)) ? rmax : mmax;
                pos_lower |= (q1 > 0) ? vlo > 0 : ((q1 < 0) & (vhi < 0));
            }
        }
        double low1 = kVarMin, high1 = kVarMax;
        if (has_vel) {
            const float sdmax = (float)mmax;
            double xlo = 0.0;
            if (pos_lower) {  // a velocity range that excludes 0: a positive lower bound on sd
                float sdmin = -kJvelMaxSd;
                for (int k = 0; k < d; ++k) {
                    double q1, q2;
                    cubic_d1_d2(cf[(0 * nseg + seg) * d + k], cf[(1 * nseg + seg) * d + k], cf[(2 * nseg + seg) * d + k], t, q1, q2);
                    const double rmin = (q1 > 0 ? vlim[2 * k] : vlim[2 * k + 1]) / q1;
                    if (q1 != 0 && !isnan(q1)) sdmin = (float)(rmin >= (double)sdmin ? rmin : (double)sdmin);
                }
                const double lo = (double)sdmin >= 0.0 ? (double)sdmin : 0.0;
                xlo = lo * lo;
            }
            const float up = sdmax * sdmax;
            const double xhi = (double)up;
            low1 = low1 > xlo ? low1 : xlo;
            high1 = high1 < xhi ? high1 : xhi;
        }
        P[kWaveRec * j + 1] = low1;
        P[kWaveRec * j + 2] = high1;
    }
    nb = wave_max_f64(isnan(nb) ? 3.0e300 : nb) * (1.0 + 1e-12);
    __syncthreads();
    // the gridpoints after which the spline segment changes, ascending (the scans test two scalar compares per stage
    // instead of locating every gridpoint on the spline again)
    int nchg = 0;
    for (int base = 0; base < N; base += 64) {
        const int j = base + lane;
        const bool c = j < N && sgi[j] != sgi[j + 1];
        const unsigned long long m = __builtin_amdgcn_ballot_w64(c);
        if (c) chg[nchg + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0))] = (unsigned short)j;
        nchg += __builtin_popcountll(m);
    }
    __syncthreads();

    // ---- per-lane row constants --------------------------------------------------------------------------
    // Every row is produced by ONE formula, whatever its kind (no selects on the row type):
    //     q1 = (d2 + d1 t) + d0 t^2,  q2 = e1 + e0 t,  t = (nextpt ? s_{i+1} : s_i) - seg_b      (scipy's order)
    //     a = +-(nextpt ? q1 + 2 delta q2 : q1),  b = +-q2
    // acceleration rows: d0..e0 are the (scaled) derivative coefficients of the lane's dof on its current segment;
    // the other rows are constants in the same clothes: box rows (a, b) = (d2, e1) with everything else 0, the x_next
    // pair a "next point" row with q1 = 0, q2 = -+1 (0 + 2 delta (-+1) = -+2 delta exactly), a disabled row all zero.
    bool is_acc[S], nextpt[S];
    int dof[S], sgn[S];
    double ccst[S];
    double d0[S], d1[S], d2[S], e0[S], e1[S], seg_b[S];
    bool cfinite = true;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int vi = 64 * s + lane, m = vi - 6;
        is_acc[s] = m >= 0 && m < nblk * d;
        const int blk = is_acc[s] ? m / d : 0;
        dof[s] = is_acc[s] ? m - blk * d : 0;
        sgn[s] = (blk & 1) ? (int)0x80000000 : 0;
        nextpt[s] = is_acc[s] ? (blk >> 1) != 0 : (vi == 4 || vi == 5);
        const double *alim = A.alim + (size_t)bb * 2 * d;
        // c: the acceleration limit, the u box, or the disabled row's -1 (rows 2..5 take the stage's scalars)
        ccst[s] = is_acc[s] ? ((blk & 1) ? alim[2 * dof[s]] : -alim[2 * dof[s] + 1]) : (vi == 0 ? kVarMin : (vi == 1 ? -kVarMax : -1.0));
        cfinite &= fabs(ccst[s]) < 1e300;
        d0[s] = d1[s] = e0[s] = 0.0;
        d2[s] = vi == 0 ? -1.0 : (vi == 1 ? 1.0 : 0.0);                                   // q1 of the constant rows
        e1[s] = (vi == 2 || vi == 4) ? -1.0 : ((vi == 3 || vi == 5) ? 1.0 : 0.0);          // q2 of the constant rows
        seg_b[s] = 0.0;  // (acceleration rows: `settle` loads their segment)
    }
    cfinite = __builtin_amdgcn_ballot_w64(!cfinite) == 0;
    // a and b depend on the gridpoints only, so they are computed one stage AHEAD of the scans, in the shadow of the
    // current stage's dependent chain (`rows_ab`, branch-free); c of the four rows that carry the stage's scalars is
    // set when they are known (`rows_c`).  The spline segment of a lane's gridpoint changes at the few gridpoints
    // listed in `chg`; `settle(jc, jn, which)` reloads the lanes at gridpoint jc (which & 1) / jn (which & 2).
    auto settle = [&](int jc, int jn, int which) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (is_acc[s] && (which & (nextpt[s] ? 2 : 1))) {
                const int j = sgi[nextpt[s] ? jn : jc];
                d0[s] = cf[(0 * nseg + j) * d + dof[s]] * 3.0;  // the derivative's coefficients (cubic_d1_d2_scaled)
                d1[s] = cf[(1 * nseg + j) * d + dof[s]] * 2.0;
                d2[s] = cf[(2 * nseg + j) * d + dof[s]];
                e0[s] = d0[s] * 2.0;
                e1[s] = d1[s];
                seg_b[s] = brk[j];
            }
        }
    };
    auto chg_at = [&](int k) { return (k >= 0 && k < nchg) ? __builtin_amdgcn_readfirstlane((int)chg[k]) : -2; };
    WaveStage G;
    G.nC = nC; G.lane = lane; G.norm_bound = nb;
    {   // floor of -c over the acceleration rows (= min over the dofs of min(amax, -amin)); no acceleration rows: none can be a record
        double lm = 3.0e300;
#pragma unroll
        for (int s = 0; s < S; ++s) lm = (is_acc[s] & (-ccst[s] < lm)) ? -ccst[s] : lm;
        G.limit_min = wave_min_f64(lm);
    }
    G.two_delta = 0.0; G.n0 = 0.0; G.n1 = 0.0;
#pragma unroll
    for (int s = 0; s < 3; ++s) G.rows[s] = s < S ? __builtin_amdgcn_ballot_w64(64 * s + lane < nV) : 0ull;
    const bool traj_ok = cfinite && nb < 1e6;
    // last: the stage of the final gridpoint (feasible sets only) -- its interpolation block repeats the stage's own
    // rows (linear_constraint.py:172,177)
    auto rows_ab = [&](double sc, double sn, double two_delta, WaveRows<S> &Q, bool &norms_ok, bool last = false) {
        unsigned long long short_rows = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const double t = (nextpt[s] ? sn : sc) - seg_b[s];
            const double q1 = (d2[s] + d1[s] * t) + d0[s] * (t * t);
            const double q2 = e1[s] + e0[s] * t;
            const double av = (nextpt[s] && !last) ? q1 + two_delta * q2 : q1;
            const double a = __hiloint2double(hi32(av) ^ sgn[s], __double2loint(av));
            const double b = __hiloint2double(hi32(q2) ^ sgn[s], __double2loint(q2));
            Q.a[s] = a; Q.b[s] = b; Q.c[s] = ccst[s];
            // the certificates' row-norm guard: null, or longer than 0.05 in 1-norm -- on the high word of the (non-negative)
            // norm: hi - 1 wraps for a zero high word (0 or a denormal) and must otherwise reach the high word past 0.05
            const unsigned nk = (unsigned)hi32(fabs(a) + fabs(b)) - 1u;
            short_rows |= __builtin_amdgcn_ballot_w64(nk < 0x3fa99999u) & G.rows[s];
        }
        norms_ok = short_rows == 0;
    };
    // (the four lane masks live in VGPRs as all-ones / zero words and select bitwise: as compare masks they would sit
    // in scalar registers, which this kernel has none to spare of)
    int m2 = lane == 2 ? -1 : 0, m3 = lane == 3 ? -1 : 0, m4 = lane == 4 ? -1 : 0, m5 = lane == 5 ? -1 : 0;
    asm volatile("" : "+v"(m2), "+v"(m3), "+v"(m4), "+v"(m5));
    auto bitsel = [](int m, double a, double b) {  // m ? a : b
        return __hiloint2double((m & hi32(a)) | (~m & hi32(b)), (m & __double2loint(a)) | (~m & __double2loint(b)));
    };
    auto rows_c = [&](WaveRows<S> &Q, double n0, double n1, double low1, double high1) {
        double c = Q.c[0];  // (slot 0 holds rows 0..5)
        c = bitsel(m2, low1, c);
        c = bitsel(m3, -high1, c);
        c = bitsel(m4, n0, c);
        c = bitsel(m5, -n1, c);
        Q.c[0] = c;
    };

    const bool use_cert = !(A.flags & TPR_STRICT_SEIDEL);

    // warm-start state of the reference's wrapper object (active_c_up / active_c_down, reference row ids): zeros for a
    // fresh object, or what an earlier pass on the same object left behind (tpr_problem.active)
    int up0 = 0, up1 = 0, dn0 = 0, dn1 = 0;
    const bool want_state = A.active != nullptr;
    if (want_state) {
        const int32_t *st = A.active + (size_t)bb * 4;
        up0 = __builtin_amdgcn_readfirstlane(st[0]); up1 = __builtin_amdgcn_readfirstlane(st[1]);
        dn0 = __builtin_amdgcn_readfirstlane(st[2]); dn1 = __builtin_amdgcn_readfirstlane(st[3]);
    }
    auto put_state = [&]() {  // (SPLIT: active_c_up lives in wave 1, active_c_down in wave 0)
        if (want_state && lane == 0) {
            int32_t *st = A.active + (size_t)bb * 4;
            if (do_l) { st[0] = up0; st[1] = up1; }
            if (do_u) { st[2] = dn0; st[3] = dn1; }
        }
    };

    if (A.feasible_X) {
        // ---- compute_feasible_sets: reachability_algorithm.py:131-164 ------------------------------------------
        // Per stage two 2-D LPs (min x, max x) with x and x_next boxed to +-CVXPY_MAXX, in stage order with the
        // warm-start state carried along as the reference does (group_feasible_kernel is the throughput form).
        double *X = A.feasible_X + (size_t)bb * 2 * (N + 1);
        WaveRows<S> R;
        for (int i = 0; i <= N; ++i) {
            const bool last = i == N;
            const double s_c = P[kWaveRec * i], s_x = P[kWaveRec * (last ? i : i + 1)];
            double low1 = P[kWaveRec * i + 1], high1 = P[kWaveRec * i + 2];
            // x_min / x_max of solve_stagewise_optim intersect the box (cy_seidel_solverwrapper.pyx:598-601)
            low1 = low1 > -kFeasMaxX ? low1 : -kFeasMaxX;
            high1 = high1 < kFeasMaxX ? high1 : kFeasMaxX;
            settle(i, last ? i : i + 1, 3);
            rows_ab(s_c, s_x, 2 * (s_x - s_c), R, G.norms_ok, last);
            rows_c(R, -kFeasMaxX, kFeasMaxX, low1, high1);
            if (last) {  // ... and the x_next pair is disabled: (0, 0, -1)
                R.a[0] = bitsel(m4 | m5, 0.0, R.a[0]);
                R.b[0] = bitsel(m4 | m5, 0.0, R.b[0]);
                R.c[0] = bitsel(m4 | m5, -1.0, R.c[0]);
            }
            G.low1 = low1; G.high1 = high1;
            G.stage_ok = G.norms_ok & traj_ok & !wave_any(!(low1 <= high1));
            WaveLp sl, su;
            double vert[4];
            bool pair_ok;
            for (int which = 0; which < 2; ++which) {
                const double v0 = which ? 1e-9 : -1e-9, v1 = which ? 1.0 : -1.0;
                const int w0 = which ? dn0 : up0, w1 = which ? dn1 : up1;
                WaveLp &o = which ? su : sl;
                bool got = false;
                const int p = w0 < 0 ? -1 - w0 : w0 + 4, q = w1 < 0 ? -1 - w1 : w1 + 4;
                if (use_cert && w0 != w1 && p < nV && q < nV && !(p < 4 && q < 4) && w0 >= -4 && w1 >= -4)
                    got = wave_cert_pair<S>(R, G, v0, v1, p, q, w0, w1, o, vert, pair_ok);
                if (!got) o = wave_lp2d<S>(R, nC, lane, v0, v1, kVarMin, kVarMax, low1, high1, w0, w1);
                if (o.ok) {
                    if (which) { dn0 = o.ac0; dn1 = o.ac1; } else { up0 = o.ac0; up1 = o.ac1; }
                }
            }
            double lo = sl.ok ? sl.x : qnan();
            if (lo < 0) lo = 0;
            if (lane == 0) { X[2 * i] = lo; X[2 * i + 1] = su.ok ? su.x : qnan(); }
        }
        put_state();
        return;
    }

    // ---- backward scan: controllable sets ------------------------------------------------------------------
    int wk = 4, wl = 5, wr = 5;  // what the warm certificates try, as virtual rows: the state's pairs when they are usable
    bool uvalid = use_cert && dn0 >= 0 && dn0 < nC && dn1 >= -4 && dn1 < nC && dn0 != dn1;
    bool lvalid = use_cert && up1 == -3 && up0 >= 0 && up0 < nC;
    if (uvalid) { wk = dn0 + 4; wl = dn1 < 0 ? -1 - dn1 : dn1 + 4; }
    if (lvalid) wr = up0 + 4;
    double kn0 = boundary_x(A.flags, sd_end), kn1 = boundary_x(A.flags, sd_end_hi);
    if (lane == 0) { P[kWaveRec * N + 3] = kn0; P[kWaveRec * N + 4] = kn1; }
    // `live`: the scan is still producing sets.  A NaN K[N] makes stage N-1 NaN without solving it; the first NaN
    // stage ends the scan and the rows above it stay 0 (reachability_algorithm.py:190-197)
    bool live = !wave_any(isnan(kn0) || isnan(kn1));
    const bool nan_start = !live;
    WaveRows<S> R;
    // LDS values are fetched ahead of their use: the gridpoint of stage i - 2 and the box of stage i - 1 while stage i
    // is being solved (a lone wave has nothing else to hide an LDS round trip behind)
    double s_n = P[kWaveRec * N], s_i = P[kWaveRec * (N - 1)], s_m = P[kWaveRec * (N >= 2 ? N - 2 : 0)];
    double low1 = P[kWaveRec * (N - 1) + 1], high1 = P[kWaveRec * (N - 1) + 2];
    settle(N - 1, N, 3);
    rows_ab(s_i, s_n, 2 * (s_n - s_i), R, G.norms_ok);
    // segment changes ahead: the lanes at s_i cross after gridpoint c when the scan reaches i - 1 == c, the lanes at
    // s_{i+1} one stage later
    int ka = nchg - 1, kb = nchg - 1;
    if (chg_at(ka) == N - 1) ka -= 1;
    int ca = chg_at(ka), cb = chg_at(kb);
    for (int i = N - 1; i >= 0; --i) {
        const int imm = i > 1 ? i - 2 : 0, im = i > 0 ? i - 1 : 0;
        const double s_mm = P[kWaveRec * imm];
        const double low1_m = P[kWaveRec * im + 1], high1_m = P[kWaveRec * im + 2];
        if (ca == i - 1 || cb == i) {  // rare: the next stage's gridpoints sit on another spline segment
            settle(im, i, (ca == i - 1 ? 1 : 0) | (cb == i ? 2 : 0));
            if (ca == i - 1) ca = chg_at(--ka);
            if (cb == i) cb = chg_at(--kb);
        }
        // One straight-line block per stage whether or not the scan is still live (a dead scan computes and discards):
        // the next stage's rows, and both LPs of this one from their warm certificates -- two independent chains of
        // fetches, divisions and ballots that fill each other's latencies: the previous stage's active pair (upper
        // bound: max x - 1e-9 u) and its binding row (lower bound: max 1e-9 u - x)
        WaveRows<S> Rm;
        bool norms_ok_m;
        rows_c(R, kn0, kn1, low1, high1);
        G.low1 = low1; G.high1 = high1; G.n0 = kn0; G.n1 = kn1; G.two_delta = 2 * (s_n - s_i);
        G.stage_ok = G.norms_ok & traj_ok & live & !wave_any(!(low1 <= high1));
        rows_ab(s_m, s_i, 2 * (s_i - s_m), Rm, norms_ok_m);
        WaveLp su, sl;
        su.ok = sl.ok = false; su.u = su.x = sl.u = sl.x = qnan(); su.ac0 = su.ac1 = sl.ac0 = sl.ac1 = 0;
        double vert[4];
        bool pair_ok;
        bool got_u = true, got_l = true;
        if (do_u) got_u = wave_cert_warm<S>(R, G, -1e-9, 1.0, wk, wl, uvalid, su, vert, pair_ok);
        // The lower-bound certificate follows the reference's COLD run (wave_lower_trace).  A valid warm start of that LP -- two
        // distinct structural rows in the wrapper's state: after a full iteration that ended on two structural rows (K_lo above
        // the box), or carried in through tpr_problem.active -- makes the reference visit [up1, up0, ...] first: another trace,
        // which is left to the iteration (cy_seidel_solverwrapper.pyx:253-264; as families 2 and 3 do: ADVICE r4).
        const bool lcold = !(up0 >= 0 && up0 < nC && up1 >= 0 && up1 < nC && up0 != up1);
        if (do_l) got_l = wave_cert_lower<S>(R, G, wr, lvalid & lcold, kVarMin, kVarMax, sl);
        if (live && !(got_u && got_l)) {  // rare: a certificate did not hold
            if (!got_u) {
                // A moved active pair runs the reference's iteration: conditions (A)-(C) bound its LAST pivot only, and
                // on the way to a moved pair the reference passes through intermediate optima whose 1-D problems they say
                // nothing about (tpr_cert.hip.inc, cert_propose2).  A full iteration costs this kernel about what a
                // proposal and a second certificate did.
                su = wave_lp2d<S>(R, nC, lane, -1e-9, 1.0, kVarMin, kVarMax, low1, high1, dn0, dn1);
            }
            if (!got_l) {
                if (use_cert) {
                    const int r1 = wave_lower_search<S>(R, G);
                    if (lcold && r1 >= 0 && !(lvalid && r1 == wr)) got_l = wave_cert_lower<S>(R, G, r1, true, kVarMin, kVarMax, sl);
                }
                if (!got_l) {
                    sl = wave_lp2d<S>(R, nC, lane, 1e-9, -1.0, kVarMin, kVarMax, low1, high1, up0, up1);
                }
            }
        }
        double lo = 0, hi = 0;
        if (live) {
            if (do_u && su.ok) {
                dn0 = su.ac0; dn1 = su.ac1;
                // the warm pair of the next stage as virtual rows: (k, l) = (ac0, ac1), usable when k is a structural row
                uvalid = use_cert && dn0 >= 0 && dn0 != dn1;
                wk = uvalid ? dn0 + 4 : 4;
                wl = uvalid ? (dn1 < 0 ? -1 - dn1 : dn1 + 4) : 5;
            }
            if (do_l && sl.ok) {
                up0 = sl.ac0; up1 = sl.ac1;
                lvalid = use_cert && up1 == -3 && up0 >= 0;  // "x on its box bound, u on row up0"
                wr = lvalid ? up0 + 4 : 5;
            }
            hi = su.ok ? su.x : qnan();
            lo = sl.ok ? sl.x : qnan();
            if (lo < 0) lo = 0;
        } else if (nan_start && i == N - 1) {
            lo = qnan(); hi = qnan();
        }
        if (SPLIT) {  // each wave publishes its bound; both read the pair back behind the stage's barrier
            if (lane == 0) P[kWaveRec * i + (wv == 0 ? 4 : 3)] = wv == 0 ? hi : lo;
            __syncthreads();
            lo = P[kWaveRec * i + 3]; hi = P[kWaveRec * i + 4];
        } else if (lane == 0) {
            P[kWaveRec * i + 3] = lo; P[kWaveRec * i + 4] = hi;
        }
        if (live) live = !wave_any(isnan(lo) || isnan(hi));
        kn0 = lo; kn1 = hi;
        s_n = s_i; s_i = s_m; s_m = s_mm; low1 = low1_m; high1 = high1_m;
        R = Rm; G.norms_ok = norms_ok_m;
    }
    const bool failed = !live;
    __syncthreads();  // K rows written by lane 0 are read by the whole wave below

    // the controllable sets leave for HBM only when the caller wants them (SPLIT: wave 1's last job, with its half of the
    // warm-start state; the rest is wave 0's)
    if (A.K && do_l) {
        double *K = A.K + (size_t)bb * 2 * (N + 1);
        for (int e = lane; e < 2 * (N + 1); e += 64) K[e] = P[kWaveRec * (e >> 1) + 3 + (e & 1)];
    }
    if (SPLIT && wv == 1) {
        put_state();
        return;
    }
    double *xs = A.sd2 ? A.sd2 + (size_t)bb * (N + 1) : nullptr;
    double *sdv = A.sd ? A.sd + (size_t)bb * (N + 1) : nullptr;
    double *us = A.u ? A.u + (size_t)bb * N : nullptr;
    const double x_start = boundary_x(A.flags, sd_start);
    const bool dead = wave_any(failed || x_start + kPySmall < kn0 || kn1 + kPySmall < x_start);
    if (A.backward_only) {  // controllable sets on their own (+ the controllability verdict for TOPPRAsd)
        if (lane == 0 && A.status) A.status[bb] = dead ? TPR_STATUS_FAIL_UNCONTROLLABLE : TPR_STATUS_OK;
        put_state();
        return;
    }
    if (dead) {
        for (int e = lane; e <= N; e += 64) { if (xs) xs[e] = qnan(); if (sdv) sdv[e] = qnan(); }
        for (int e = lane; e < N; e += 64) if (us) us[e] = qnan();
        if (lane == 0 && A.status) A.status[bb] = TPR_STATUS_FAIL_UNCONTROLLABLE;
        put_state();
        return;
    }

    // ---- forward scan: parameterization --------------------------------------------------------------------
    // sd2_j and u_j are staged in fields 1, 2 of the records (the box is not needed any more)
    double x = x_start;
    bool any_nan = !(x >= 0.0);  // "sqrt(x) is NaN" (reachability_algorithm.py:365-372 looks at sd_vec = sqrt(xs))
    if (lane == 0) P[1] = x;
    int tries = 0, guess = -1;
    int nan_from = N + 1, zero_from = N;  // a failed forward pass leaves sd2 = NaN / u = 0 from here on
    double s_cur = P[0], s_nx = P[kWaveRec], s_pp = P[kWaveRec * (N >= 2 ? 2 : N)];
    double k0 = P[kWaveRec + 3], k1 = P[kWaveRec + 4];
    settle(0, 1, 3);
    rows_ab(s_cur, s_nx, 2 * (s_nx - s_cur), R, G.norms_ok);
    // segment changes ahead: stage i + 1's own gridpoint crosses when chg holds i, its next gridpoint when it holds i + 1
    int fa = 0, fb = 0;
    if (chg_at(fb) == 0) fb += 1;
    ca = chg_at(fa); cb = chg_at(fb);
    for (int i = 0; i < N; ++i) {
        const int ip = i + 2 <= N ? i + 2 : N, ipp = i + 3 <= N ? i + 3 : N;
        const double s_ppp = P[kWaveRec * ipp];
        const double k0_p = P[kWaveRec * ip + 3], k1_p = P[kWaveRec * ip + 4];
        const double delta = s_nx - s_cur;
        if (ca == i || cb == i + 1) {  // rare: the next stage's gridpoints sit on another spline segment
            settle(i + 1, ip, (ca == i ? 1 : 0) | (cb == i + 1 ? 2 : 0));
            if (ca == i) ca = chg_at(++fa);
            if (cb == i + 1) cb = chg_at(++fb);
        }
        WaveRows<S> Rp;
        bool norms_ok_p;
        rows_c(R, k0, k1, 0.0, 0.0);  // (the x box rows have a = 0: no part in the 1-D LP)
        rows_ab(s_nx, s_pp, 2 * (s_pp - s_nx), Rp, norms_ok_p);
        // the reference's retries: lower x_i and solve again, at most 10 times (reachability_algorithm.py:303-363)
        double uu = qnan();
        int act1d = 0;
        bool ok = wave_lp1d<S>(R, nC, lane, 2 * delta, x, kVarMin, kVarMax, guess, uu, want_state, act1d);
        ok = !wave_any(isnan(x)) && ok;
        while (!ok && tries < kMaxTries) {
            const double t1 = x - kPyTiny, t2 = 0.999 * x;
            x = t2 > t1 ? t2 : t1;
            tries += 1;
            if (lane == 0) P[kWaveRec * i + 1] = x;
            ok = wave_lp1d<S>(R, nC, lane, 2 * delta, x, kVarMin, kVarMax, guess, uu, want_state, act1d);
            ok = !wave_any(isnan(x)) && ok;
        }
        if (ok && want_state) dn0 = act1d;  // the 1-D path's write into active_c_down (cy_seidel_solverwrapper.pyx:646-649)
        if (!ok) {
            nan_from = i + 1; zero_from = i;
            any_nan = true;
            break;
        }
        tries = 0;
        double xn = x + (2 * delta) * uu;
        const double t1 = xn - kPyTiny, t2 = 0.9999 * xn;
        xn = t2 > t1 ? t2 : t1;
        const double m1 = xn > k0 ? xn : k0;
        x = m1 < k1 ? m1 : k1;
        if (lane == 0) { P[kWaveRec * i + 2] = uu; P[kWaveRec * (i + 1) + 1] = x; }
        any_nan |= !(x >= 0.0);
        s_cur = s_nx; s_nx = s_pp; s_pp = s_ppp; k0 = k0_p; k1 = k1_p;
        R = Rp;
    }
    if (SPLIT) {  // (wave 1 has left: only this wave's own LDS writes are waited for)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
    for (int e = lane; e <= N; e += 64) {
        const double v = e >= nan_from ? qnan() : P[kWaveRec * e + 1];
        if (xs) xs[e] = v;
        if (sdv) sdv[e] = sqrt(v);
    }
    for (int e = lane; e < N; e += 64) if (us) us[e] = e >= zero_from ? 0.0 : P[kWaveRec * e + 2];
    if (lane == 0 && A.status) A.status[bb] = any_nan ? TPR_STATUS_ERR_UNKNOWN : TPR_STATUS_OK;
    put_state();
}

}  // namespace tpr

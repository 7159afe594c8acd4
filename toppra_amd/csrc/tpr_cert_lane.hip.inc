// tpr_cert_lane.hip.inc -- kernel family 3, the LANE-LEVEL certificates: everything a lane does on its own for a stage LP
// (proposal of the active pair, certificate of a pair, lower-bound certificate, the equality stage).  Straight-line
// per-lane code without cross-lane operations or LDS traffic of its own (a lane's row columns are plain pointers), so that
// the same source also compiles for the host: tests/host_cert/ drives these functions against the CPU restatement of the
// reference on millions of stage LPs (tests/test_host_cert.py) -- every certified answer must be the reference's bits.
// Included by tpr_cert.hip.inc (which holds the cooperative batches and the kernels).

#pragma once
#ifndef TPR_SLACK_ABS
#define TPR_SLACK_ABS 1e-6
#endif
#ifndef TPR_SLACK_REL
#define TPR_SLACK_REL 1e-9
#endif
namespace tpr {

constexpr double kCertSlack = TPR_SLACK_ABS;    // absolute margin on row residuals (solver tolerances: 1e-10, 1e-8)
constexpr double kCertRelSlack = TPR_SLACK_REL; // relative margin against rounding of the residuals
constexpr double kCertMinNorm = 5e-2;   // rows are null or at least this long (keeps |t| < 1e10 on every pivot line)
constexpr double kCertMinCross = 1e-7;  // rows are exactly parallel to the pivot row or clearly not
constexpr double kCertMinRange = 1e-3;  // amax - amin of every joint (a pivot row's twin is not re-checked)
constexpr int kCertXch = 10;            // LDS exchange area per lane in doubles: 9 fields + the queue of waiting LPs (2 ints; see cert_needy_batch)
// An opaque use of a value in the main flow of control (no instruction): what feeds it cannot be sunk into a conditional region.
#if defined(__HIP_DEVICE_COMPILE__)
#define TPR_PIN(x) asm volatile("" : "+v"(x))
#else
#define TPR_PIN(x)
#endif

constexpr int kCertBatchLanes = 16;     // lanes per LP in the cooperative batches: 4 LPs at a time (0.3 LPs wait per wave and stage)
// groups that work per batch: as many row mirrors (3 (4 D + 6) doubles each) as keep the block under 160 KB / 4 of LDS -- a CU must
// hold four blocks, one wave per SIMD.  Up to round 6's first session: four up to 7 dof, two at 8..12, one at 13; with the exchange
// area 2 KB smaller (cert_needy_batch: n0, n1, low1, high1 from the column of row constants) all four fit up to 12 dof (40.0 KB
// there), two at 13 / 14 (39.6 / 39.8 KB), one at 15 (40.5 KB).
template <int D>
constexpr int cert_batch_groups() { return D >= 15 ? 1 : (D >= 13 ? 2 : 64 / kCertBatchLanes); }

// Up to 7 dof CertStage::fetch reads rows 0..5 as (q1, q2) pairs from a six-double LDS table of the block (kSpecRows there); the
// pointer is a member only where it is used, so that the other dofs' stage objects are what they were.
template <bool PAIRS>
struct CertSpecTable { const double *spec = nullptr; };
template <>
struct CertSpecTable<false> {};

template <int D, int BS>
struct CertStage : CertSpecTable<(D <= 7)> {
    static constexpr int nC = 2 + 4 * D;
    // Row numbering INSIDE this kernel family ("vi"): 0..3 box rows, 4,5 the x_next pair, and the acceleration
    // rows at 8 + 8 blk + k (blk 0: +q(s_i), 1: -q(s_i), 2: +q(s_{i+1}), 3: -q(s_{i+1}); k < D <= 8), so that
    // block and joint of a row are a shift and a mask instead of a division by D.  It is order-isomorphic to
    // the reference's numbering (row id = vi - 4 for the x_next pair, 2 + blk D + k for the others, -1 - vi for
    // the box rows), which is all the visiting-order logic needs; ids are converted at the batch interface only.
    // (round 3: 9..16 dof use a block stride of 16 -- rows at 16 + 16 blk + k -- with the same 0..5 in front)
    static constexpr int SH = D <= 8 ? 3 : 4, ST = 1 << SH;
    static constexpr int V0 = ST, V1 = 2 * ST, V2 = 3 * ST, V3 = 4 * ST, nV = 5 * ST;
    static_assert(D <= 16, "block stride of the internal row numbering");
    __device__ __forceinline__ static int id_of(int vi) {  // internal -> reference row id
        return vi < 4 ? -1 - vi : (vi < 8 ? vi - 4 : 2 + ((vi >> SH) - 1) * D + (vi & (ST - 1)));
    }
    __device__ __forceinline__ static int vi_of(int id) {  // reference row id -> internal (off the hot path)
        const int m = id - 2, blk = m / D;
        return id < 0 ? -1 - id : (id < 2 ? id + 4 : ST + ST * blk + (m - blk * D));
    }
    // Above 8 dof the block is SLIM (round 3): the acceleration rows' c is taken from the registers through a select
    // chain instead of a second copy in LDS (2 D columns), and K is staged two stages at a time instead of four -- 54
    // columns + exchange area instead of 105 at 12 dof, i.e. 39.5 KB: four blocks per CU (one wave per SIMD) instead of
    // three, and a 65536-trajectory batch in one round instead of two.
    static constexpr bool kSlim = D > 8;
    static constexpr int kLimCols = kSlim ? 6 : 6 + 2 * D;   // LDS columns of row constants per lane
    static constexpr int kRing = kSlim ? 2 : 4;              // stages of K (X) staged in LDS between transposed stores
    // 14 dof (round 6): no staging at all -- every lane stores its own (lo, hi) pair of a stage straight to its trajectory's row
    // (16 B per lane and stage; the four stages of a 64-B line meet in L2).  The ring's 2 KB are what keeps the block under
    // 160 KB / 4: four blocks per CU, a 65536-trajectory batch in one round.
    static constexpr bool kDirectK = D >= 14;
    const double *cur1, *cur2, *nxt1, *nxt2;  // this lane's LDS columns: q', q'' at s_i and s_{i+1}, stride BS
    const double *lim;                        // this lane's LDS column of row constants: c of rows 0..5 (, cpos[D], cneg[D])
    // slim blocks: this trajectory's acceleration limits [D][2] in global memory (fetch).  On the device they sit in the block's
    // TRANSPOSED workspace (GroupArgs::tws, [field][lane]: a wave's load of one limit is 512 contiguous bytes instead of one
    // cache line per lane -- round 5: 19.5 x the algorithmic traffic at 12 dof); the host harness hands a plain [D][2] array.
#if defined(__HIP_DEVICE_COMPILE__)
    static constexpr int kAlimStride = BS;
#else
    static constexpr int kAlimStride = 1;
#endif
    const double *alim_lane = nullptr;
    // The pair form of fetch (below): up to 7 dof.  At 8 dof it left the TOPPRAsd instantiation with 12 B of scratch per lane, and
    // the slim blocks keep their own form (the sunk-load story in fetch).
    static constexpr bool kPairFetch = D <= 7;
    static constexpr int kSpecDoubles = kPairFetch ? 6 : 0;
    double rc1[D], rc2[D], rn1[D], rn2[D];    // q', q'' again, in registers for the unrolled scans
    double cpos[D], cneg[D];                  // c of the + rows (-amax) and of the - rows (+amin)
    double cmax;                              // max |c| over the acceleration rows
    double min_range;                         // min over joints of amax - amin
    double two_delta, n0, n1, low1, high1;

    // One row by (per-lane) index.
    __device__ __forceinline__ void fetch(int vi, double &a, double &b, double &c) const {
        if constexpr (kPairFetch) {
            // Every row as "q1 (+ 2 delta q2), q2" of one pair of loads, signed by an XOR on the high words: rows 0..5 take their
            // pair from a six-double table (`spec`: (1, 0) for the u box, (+0, 1) for the x box, (-0, 1) for the x_next pair,
            // whose a = -0 + 2 delta * 1 is 2 delta bit for bit, signed zeros included), the acceleration rows from the lane's
            // columns (cur2 / nxt2 follow cur1 / nxt1 at D * BS).  No select between values, one index for c.
#if defined(__HIP_DEVICE_COMPILE__)
            const double *sp = this->spec;
#else
            static const double kSpecRows[6] = {1.0, 0.0, 0.0, 1.0, -0.0, 1.0};
            const double *sp = kSpecRows;
#endif
            const bool acc = vi >= ST;
            const int k = vi & (ST - 1);                                   // (rows 0..5: the row itself)
            const bool nx = vi >= (acc ? V2 : 4);                          // the row's a is q1 + 2 delta q2
            // the negated twin: blocks 1 and 3 of the acceleration rows (vi >> SH even), the even rows of 0..5
            const unsigned sgn = ~((unsigned)(acc ? vi >> SH : vi) << 31) & 0x80000000u;
            // (both addresses formed before the select between them: an arm with arithmetic in it becomes a divergent region)
            const double *pa = (nx ? nxt1 : cur1) + k * BS, *ps = sp + (vi & 6);
            const int st2 = acc ? D * BS : 1;
            const double *p1 = acc ? pa : ps;
            const double *p2 = p1 + st2;
            const double q1 = *p1, q2 = *p2;
            const double av = nx ? q1 + two_delta * q2 : q1;
            a = __hiloint2double(__double2hiint(av) ^ (int)sgn, __double2loint(av));
            b = __hiloint2double(__double2hiint(q2) ^ (int)sgn, __double2loint(q2));
            // c: rows 0..5 at their own index, the + blocks' (vi >> SH odd) at 6 + k, the - blocks' at 6 + D + k
            c = lim[(k + (acc ? ((vi >> SH) & 1 ? 6 : 6 + D) : 0)) * BS];
            return;
        }
        const bool acc = vi >= ST;
        const int blk = acc ? (vi >> SH) - 1 : 0, k = acc ? (vi & (ST - 1)) : 0;
        const bool nx = blk >> 1;
        const double q1 = (nx ? nxt1 : cur1)[k * BS], q2 = (nx ? nxt2 : cur2)[k * BS];
        const double av = nx ? q1 + two_delta * q2 : q1;
        // rows 0..5 are +- twins of three base rows as well: (1, 0) for the u box, (0, 1) for the x box,
        // (2 delta, 1) for the x_next pair, the even row being the negated one; their c sits in front of
        // the acceleration rows' in the lane's LDS column of row constants (`lim`: c[6], cpos[D], cneg[D])
        const int g = vi >> 1;
        const double sa = g == 0 ? 1.0 : (g == 2 ? two_delta : 0.0), sb = g == 0 ? 0.0 : 1.0;
        const bool neg = acc ? (blk & 1) : !(vi & 1);
        const double ba = acc ? av : sa, bb = acc ? q2 : sb;
        a = neg ? -ba : ba;
        b = neg ? -bb : bb;
        if (!kSlim) {
            c = lim[(acc ? 6 + ((blk & 1) ? D : 0) + k : vi) * BS];
        } else {
            // Round 4: rows 0..5 from the lane's LDS column, the acceleration rows from the trajectory's limits in global
            // memory (L2-hot).  BOTH loads are needed on every path as far as the compiler can tell -- an in-range LDS index
            // for the acceleration rows too, and the merge as integer operations under a mask it cannot see through.  A load
            // that only one arm of a select needs (round 3: `lim[(acc ? 0 : vi) * BS]`, whose value for acc is a known
            // constant; or `acc ? al : cs`) is sunk into a divergent region, and with the ~10 fetches per stage of the
            // trace-following certificates those regions cut the stage's straight-line block to pieces: the 9-dof kernel went
            // from 0 to 1.4 KB of scratch per lane, the 12-dof one from 0.5 to 2.4 KB (DESIGN.md section 3.2).
            const double cs = lim[(acc ? (k & 3) : vi) * BS];
            const double al = alim_lane[(2 * k + ((blk & 1) ? 0 : 1)) * kAlimStride];
            int m = -(int)acc;                                        // -1 for an acceleration row, else 0 ...
            TPR_PIN(m);                                               // ... and opaque: no select may be recognised in what follows
            const int flip = (int)(~((unsigned)blk << 31) & 0x80000000u);      // cpos = -amax: the sign bit for an even block
            const int hs = __double2hiint(cs), ls = __double2loint(cs);
            c = __hiloint2double(hs ^ ((hs ^ __double2hiint(al) ^ flip) & m), ls ^ ((ls ^ __double2loint(al)) & m));
        }
    }
    // c of rows 0..5 of the current stage into the LDS column fetch() reads (call after low1 .. n1 are set)
    __device__ __forceinline__ void publish_special(double *lim_w) const {
        lim_w[2 * BS] = low1; lim_w[3 * BS] = -high1; lim_w[4 * BS] = n0; lim_w[5 * BS] = -n1;
    }

    // Index of the +- pair an acceleration row belongs to (0..2D-1), -1 for the other rows.
    __device__ __forceinline__ static int pair_of(int vi) {
        return (((vi - ST) >> (SH + 1)) * D + (vi & (ST - 1))) | -(int)(vi < ST);  // mask instead of ?: (no branch)
    }

    // Row-norm guard of the stage (shared by both LPs): every row null or longer than kCertMinNorm;
    // nmax = largest |a|+|b|.
    __device__ __forceinline__ bool norms(double &nmax) const {
        // on bits 62..31 of the (non-negative) norms, as unsigned running minimum and maximum: key - 2 wraps for a
        // zero, and a NaN or an infinity has the largest keys of all; three integer operations per norm instead of
        // two compares, two mask operations and a maximum
        auto key = [](double v) { return (unsigned)((unsigned long long)__double_as_longlong(v) >> 31); };
        static_assert(kCertMinNorm == 5e-2, "key of the threshold below");
        // first key past 5e-2; key of 1e6.  The upper limit is part of the certificate's argument: with rows between
        // 0.05 and 1e6 long, a margin of kCertRelSlack (1e-6, relative to the stage's magnitudes) on every residual is
        // > 70 x the rounding error of the quotients the reference compares on the pivot line (|zero_prj| <= 29 cmax,
        // numerators <= cmax (1 + 29 nmax), quotient error <= 4 eps of that over the same denominator), so none of
        // its strict comparisons can come out differently from exact arithmetic.
        constexpr unsigned kKeyMinNorm = 0x7f533333u + 1u, kKeyHuge = 0x825d0900u;
        unsigned kmin = 0xffffffffu, kmax = key(two_delta + 1.0);  // x_next rows; box rows have norm 1
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double n1c = fabs(rc1[k]) + fabs(rc2[k]);
            const double q2 = rn2[k];
            const double n1n = fabs(rn1[k] + two_delta * q2) + fabs(q2);
            const unsigned k1 = key(n1c), k2 = key(n1n);
            const unsigned lo = k1 - 2u < k2 - 2u ? k1 - 2u : k2 - 2u, hi = k1 > k2 ? k1 : k2;
            kmin = lo < kmin ? lo : kmin;
            kmax = hi > kmax ? hi : kmax;
        }
        // an upper bound of the largest norm (low bits filled up): nmax only enters tolerances, where larger is stricter
        nmax = __longlong_as_double((long long)((unsigned long long)(kmax + 1u) << 31));
        return (kmin >= kKeyMinNorm - 2u) & (kmax < kKeyHuge) & (min_range > kCertMinRange) & (two_delta > 0.0) & (low1 <= high1);
    }
};

// x, or a value below -2.9e300 when `excl`: rows left out of a running maximum.  Only the high word is replaced
// (one select instead of two; whatever the low word holds, the value stays below -2.9e300).
__device__ __forceinline__ double cert_unless(bool excl, double x) {
    return __hiloint2double(excl ? (int)0xfe51eb2du : __double2hiint(x), __double2loint(x));
}

// The same with the decision in bit k of a mask: a sign-extending bit-field extract and a bitwise select.
__device__ __forceinline__ double cert_unless_bit(unsigned mask, int k, double x) {
    const int m = (int)(mask << (31 - k)) >> 31;  // 0 or -1
    return __hiloint2double((m & (int)0xfe51eb2du) | (~m & __double2hiint(x)), __double2loint(x));
}

// (w << 1) | (sign bit of y): one v_alignbit_b32.  A scan that only asks "does every row hold, and which is the first that
// does not" appends one bit per row in visiting order -- y = residual + tolerance, sign set = the row clearly holds -- and
// reads the answer off the word afterwards (count-leading-zeros): two instructions per row where a running minimum of row
// numbers with a bit-mask exclusion took seven.  (The sign of a rounded sum is the sign of the exact sum, and an exact 0 is
// +0: the bit is exactly "residual < -tolerance" for finite operands.)
__device__ __forceinline__ unsigned cert_push_sign(unsigned w, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(w, (unsigned)__double2hiint(y), 31);
#else
    return (w << 1) | ((unsigned)__double2hiint(y) >> 31);
#endif
}
__device__ __forceinline__ int cert_clz(unsigned w) {  // 32 for 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int)w);
#else
    return w ? __builtin_clz(w) : 32;
#endif
}

// Position of row vi in the reference's visiting order for the warm start (w0, w1) -- all three in the
// internal numbering, which is order-isomorphic to the reference's, and positions are only ever compared.
// Box rows (never pivots) get -1.  The warm pair counts when both are structural rows and distinct
// (cy_seidel_solverwrapper.pyx:253-264), else the order is the identity.
// Written with masks on purpose: as nested ?: the compiler turns it into divergent branches, which cut the
// straight-line certificate block in two and stop its halves from overlapping each other's latencies.
__device__ __forceinline__ int cert_pos(int vi, int w0, int w1) {
    const int warm = -(int)((w0 >= 4) & (w1 >= 4) & (w0 != w1));  // all ones or 0
    const int is1 = -(int)(vi == w1), is0 = -(int)(vi == w0) & ~is1;
    const int base = 2 + vi - (int)(vi > w0) - (int)(vi > w1);
    const int pw = (base & ~(is1 | is0)) | (1 & is0);             // w1 -> 0, w0 -> 1, the rest keep their order
    return ((pw & warm) | (vi & ~warm)) | -(int)(vi < 4);
}

// The reference's last pivot, pivot row (ka,kb,kc) limited by row (la,lb,lc): cy_seidel_solverwrapper.pyx:287-364.
__device__ __forceinline__ void cert_last_pivot(double ka, double kb, double kc, double la, double lb, double lc,
                                                double &u, double &x) {
    const double den = ka * ka + kb * kb;
    const double zp0 = (-ka * kc) / den;
    const double zp1 = (-kb * kc) / den;
    const double dt0 = -kb, dt1 = ka;
    const double denom = dt0 * la + dt1 * lb;
    const double num = lc + zp1 * lb + zp0 * la;
    const double T = -num / denom;
    u = zp0 + T * dt0;
    x = zp1 + T * dt1;
}

// "No row is nearly parallel to the pivot row (ka, kb)": every cross product is exactly 0 (the row
// itself, its twin, a joint that stands still) or clearly away from the solver's 1e-10.
template <int D, int BS>
__device__ __forceinline__ bool cert_cross_ok(const CertStage<D, BS> &S, double ka, double kb) {
    // as one unsigned running minimum over key = (bits 62..31 of |cross|) - 2: it wraps to 0xfffffffe / f for a zero
    // (or denormal: the solver takes its |.| < 1e-10 branch just the same) and must otherwise reach the key of
    // kCertMinCross, rounded up; 2.5 integer operations per row instead of two compares and two mask operations.
    // Rows are finite (CertStage::norms), so is every cross product.
    static_assert(kCertMinCross == 1e-7, "high word of the threshold below");
    unsigned key = 0xffffffffu;
    auto chk = [&](double cross) {
        const unsigned k2 = (unsigned)((unsigned long long)__double_as_longlong(cross) >> 31) - 2u;  // the shift drops the sign
        key = k2 < key ? k2 : key;
    };
    chk(kb);                      // box rows (-+1, 0): cross = -+kb * ... ; (0, -+1): -+ka
    chk(ka);
    chk(ka - kb * S.two_delta);   // x_next pair (+-2 delta, +-1)
#pragma unroll
    for (int k = 0; k < D; ++k) {
        chk(ka * S.rc2[k] - kb * S.rc1[k]);
        const double q2 = S.rn2[k];
        chk(ka * q2 - kb * (S.rn1[k] + S.two_delta * q2));
    }
    return key >= 2u * (0x3e7ad7f2u + 1u) - 2u;  // |cross| >= 2^-24 * 1.67772..., the first double past 1e-7 with a larger high word
}

// Is the previous active pair (wac0, wac1) still the unique, well separated optimal vertex of
//   max v0 u + v1 x ?  If so, the reference's result follows from its last-pivot formulas (see
// predict_upper_lp).  No search: anything else returns false and goes to cert_needy_batch.
// Residual margins: the structural rows share one conservative tolerance
//   tol_s >= kCertSlack + kCertRelSlack (|a u| + |b x| + |c|);  the pivot pair's +- twins are not
// re-checked: their residual is -(amax - amin) <= -min_range, compared with tol_s below.
//
// EQ: the stage's x_next rows form an equality (n0 == n1: the first backward stage, where K[N] is the
// single point sd_end^2).  Both of them pass through the optimum, so the candidate pair is (p0 = the
// row that binds along the equality line, q0 = one of the x_next rows); the other x_next row is
// skipped by the residual scan like a twin, and only p0's multiplier has a sign (see cert_equality).
//
// cert_pair_rows: p, q are valid row numbers whose rows the caller has fetched already (cert_propose has two of
// the three rows it needs in registers); `ok` carries the caller's verdict on the pair and the stage.
// TRACE (round 5): the caller is a trace-following proposal (cert_propose_sound), which has established more than this
// function asks for -- p IS the pivot of the reference's last pivot and q its limiter (p: the last record of a slide or the last
// pivot of the prologue, visited after q), and p was clearly violated when it was visited (condition (B): the slide's own
// verdict) -- so the roles are not derived from the visiting order again, the violation bound is not evaluated, and the margin
// scan over the acceleration rows only has to say "all hold" (one sign bit per +- pair, cert_push_sign) instead of
// returning the largest residual.
template <int D, int BS, bool EQ, bool TRACE = false>
__device__ __forceinline__ bool cert_pair_rows(const CertStage<D, BS> &S, double v0, double v1, int p, int q, bool ok,
                                               double pa, double pb, double pc, double qa, double qb, double qc,
                                               int wac0, int wac1, double nmax, Lp2dOut &o) {
    using C = CertStage<D, BS>;
    // straight-line on purpose (flags instead of early exits): together with cert_lower this is one
    // basic block, and the scheduler overlaps one check's LDS / division latencies with the other's work
    const double Dm = pa * qb - qa * pb;
    ok &= fabs(Dm) > kCertMinCross;
    const double rD = rcp_approx(Dm);  // the vertex only feeds margin tests / searches
    const double u = (pb * qc - qb * pc) * rD;
    const double x = (qa * pc - pa * qc) * rD;
    const double lamp = (v0 * qb - v1 * qa) * rD, lamq = (pa * v1 - pb * v0) * rD;  // v = lamp n_p + lamq n_q
    ok &= (lamp > 0) & (EQ || lamq > 0);
    // largest residual + tolerance over the rows other than p, q
    const double au = fabs(u), ax = fabs(x);
    const double tol_s = kCertSlack + kCertRelSlack * (nmax * (au + ax) + fmax(S.cmax, fmax(fabs(S.n0), fabs(S.n1))));
    double mx = -3.0e300;  // max of (residual + its tolerance)
    auto other = [&](int vi, double sc) { mx = fmax(mx, cert_unless((vi == p) | (vi == q), sc)); };
    // the u box is symmetric: one test for rows 0 and 1, which are therefore never the pair (they never are
    // the optimum of a sane problem: |u| = 1e8)
    static_assert(kVarMin == -kVarMax, "one test for both u box rows");
    ok &= (p >= 2) & (q >= 2);
    mx = (au - kVarMax) + (kCertSlack + kCertRelSlack * (au + kVarMax));
    other(2, (S.low1 - x) + (kCertSlack + kCertRelSlack * (ax + fabs(S.low1))));
    other(3, (x - S.high1) + (kCertSlack + kCertRelSlack * (ax + fabs(S.high1))));
    const double s45 = S.two_delta * u + x;
    // Row 5 (x + 2 delta u <= K_hi[i+1]) apart: on the maximum-velocity curve it passes through the vertex of the two
    // rows that defined K_hi[i+1] BY CONSTRUCTION (residual ~1e-16: "in the tolerance band" at every such stage).
    // When the pair is the warm pair, row 5 is visited after both of them and takes no part in the last pivot; all
    // the reference does with it is its violation test at the vertex the last pivot produced -- which is evaluated
    // below, in its arithmetic, on its vertex, instead of being bounded by a margin.
    bool band5 = false;
    if (!EQ) {
        other(4, (S.n0 - s45) + tol_s);
        band5 = (p != 5) & (q != 5) & !((s45 - S.n1) + tol_s < 0);
    }
    // bit k: pair k holds p or q
    // (a row outside the acceleration blocks sets no bit: at 16 dof all 32 bits belong to pairs)
    const int pp_ = C::pair_of(p), pq_ = C::pair_of(q);
    bool rows_hold = true;
    if constexpr (TRACE && !EQ) {
        // one bit per +- pair in the order of the loops below (pair 0 ends up in bit 2 D - 1): set = both twins hold with the margin
        static_assert(2 * D <= 32, "one word of pair bits");
        const unsigned own = ((unsigned)(pp_ >= 0) << ((2 * D - 1 - pp_) & 31)) | ((unsigned)(pq_ >= 0) << ((2 * D - 1 - pq_) & 31));
        unsigned held = 0u;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double s = __builtin_fma(S.rc1[k], u, S.rc2[k] * x);
            held = cert_push_sign(held, fmax(s + S.cpos[k], S.cneg[k] - s) + tol_s);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double q2 = S.rn2[k];
            const double s = __builtin_fma(S.rn1[k] + S.two_delta * q2, u, q2 * x);
            held = cert_push_sign(held, fmax(s + S.cpos[k], S.cneg[k] - s) + tol_s);
        }
        rows_hold = ((held | own) & (unsigned)((1ull << (2 * D)) - 1ull)) == (unsigned)((1ull << (2 * D)) - 1ull);
    } else {
        const unsigned own = ((unsigned)(pp_ >= 0) << (pp_ & 31)) | ((unsigned)(pq_ >= 0) << (pq_ & 31));
        double ms = -3.0e300;  // max residual over the acceleration rows outside the pivot pairs
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double s = S.rc1[k] * u + S.rc2[k] * x;
            const double m2 = fmax(s + S.cpos[k], S.cneg[k] - s);
            ms = fmax(ms, cert_unless_bit(own, k, m2));
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double q2 = S.rn2[k];
            const double s = (S.rn1[k] + S.two_delta * q2) * u + q2 * x;
            const double m2 = fmax(s + S.cpos[k], S.cneg[k] - s);
            ms = fmax(ms, cert_unless_bit(own, D + k, m2));
        }
        mx = fmax(mx, ms + tol_s);
    }
    // a usable, dual feasible pair whose vertex violates no row but has one inside the tolerance band (concurrent
    // rows): the batches' walk would arrive at the same vertex and refuse it too, so it is skipped for this LP
    o.hint_full = ok & !(mx - tol_s > 1e-9);
    ok &= (mx < 0) & rows_hold & (S.min_range > tol_s);
#ifdef TPR_TOLERANCE_MODE
    ok &= !band5;
    // measurement build (not the product): the verified vertex itself is the answer -- no replication of the
    // reference's last pivot, hence none of the guards that make that replication exact
    o.ok = ok; o.u = u; o.x = x; o.ac0 = p; o.ac1 = q;
    return ok;
#endif
#ifdef TPR_SOUND_TOLERANCE
    // Second measurement build (round 5, VERDICT r4 item 3; NOT the product): the SOUND, trace-following certificates with
    // tolerance arithmetic in what they return -- the verified vertex itself (reciprocal estimate) instead of the
    // reference's last-pivot formulas, hence no cross-product guard (it exists to make that replication exact); the roles
    // (pivot, limiter: the warm start of the next stage) and the verdict on row 5 stay.  The cooperative batches run the
    // reference's iteration exactly as in the product, so no infeasibility verdict can flip there.
    if constexpr (TRACE && !EQ) {
        const bool warm_pair_t = (p >= 4) & (q >= 4) & (((p == wac0) & (q == wac1)) | ((p == wac1) & (q == wac0)));
        const double t5t = (S.two_delta * u + x) + -S.n1;
        ok &= !band5 | (warm_pair_t & (t5t < kTiny));
        ok &= fabs(-pb * v0 + pa * v1) > 1e-6;
        o.ok = ok; o.u = u; o.x = x; o.ac0 = p; o.ac1 = q;
        return ok;
    }
#endif
    // roles in the reference's last pivot: the later row in its order is the pivot
    const int pos_p = (TRACE && !EQ) ? 1 : cert_pos(p, wac0, wac1), pos_q = (TRACE && !EQ) ? 0 : cert_pos(q, wac0, wac1);
    const bool p_pivot = (TRACE && !EQ) ? true : pos_p > pos_q;
    // EQ: a structural p must come after BOTH x_next rows, so that the running optimum already sits on
    // the equality line when p is visited (a box row p never pivots: q is the pivot, chosen by the caller)
    if (EQ) ok &= (p < 4) || (pos_p > cert_pos(4, wac0, wac1) && pos_p > cert_pos(5, wac0, wac1));
    const int k = p_pivot ? p : q, l = p_pivot ? q : p;
    const double ka = p_pivot ? pa : qa, kb = p_pivot ? pb : qb, kc = p_pivot ? pc : qc;
    const double la = p_pivot ? qa : pa, lb = p_pivot ? qb : pb, lc = p_pivot ? qc : pc;
    const bool g_cross = cert_cross_ok<D, BS>(S, ka, kb);
    ok &= g_cross;
    const double v1d = -kb * v0 + ka * v1;
    ok &= fabs(v1d) > 1e-6;
    // violation of the pivot row at the optimum of the rows visited before it is at least
    // |D| m / (max|n| |n_l|), m = smallest margin of the other rows at z* (>= -mx)
    const bool g_viol = (TRACE && !EQ) ? true : fabs(Dm) * (-mx) > 1e-8 * (nmax * (fabs(la) + fabs(lb)));
    ok &= g_viol;
    cert_last_pivot(ka, kb, kc, la, lb, lc, o.u, o.x);
    if (!EQ) {
        // cy_seidel_solverwrapper.pyx:274 for row 5 = (2 delta, 1, -K_hi[i+1]):  a u + b x + c < TINY  <=>  satisfied
        const bool warm_pair = (p >= 4) & (q >= 4) & (((p == wac0) & (q == wac1)) | ((p == wac1) & (q == wac0)));
        const double t5 = (S.two_delta * o.u + o.x) + -S.n1;
        ok &= !band5 | (warm_pair & (t5 < kTiny));
    }
    o.ok = ok;
    o.ac0 = k;  // internal numbering (see CertStage)
    o.ac1 = l;
    return ok;
}

template <int D, int BS, bool EQ>
__device__ __forceinline__ bool cert_pair(const CertStage<D, BS> &S, double v0, double v1, int p0, int q0, bool pair_ok,
                                          int wac0, int wac1, bool norms_ok, double nmax, Lp2dOut &o) {
    using C = CertStage<D, BS>;
    const bool ok = norms_ok & pair_ok & (p0 != q0) & (p0 >= 0) & (q0 >= 0) & (p0 < C::nV) & (q0 < C::nV) & !((p0 < 4) & (q0 < 4));
    const int p = ok ? p0 : 4, q = ok ? q0 : 5;  // any valid pair keeps the arithmetic defined
    double pa, pb, pc, qa, qb, qc;
    S.fetch(p, pa, pb, pc);
    S.fetch(q, qa, qb, qc);
    return cert_pair_rows<D, BS, EQ>(S, v0, v1, p, q, ok, pa, pb, pc, qa, qb, qc, wac0, wac1, nmax, o);
}

// Proposal of the active pair for the upper-bound LP when the previous stage's pair may have moved.
//
// Most active-set changes keep one of the two rows (one simplex pivot).  From the warm pair's vertex
// z_w the two 1-D problems "maximise the objective along row p's line / along row q's line subject to
// the rows that block in the improving direction" are each one pass over the rows (blocking parameter
// t = -res / (n . d), running minimum by cross-multiplication; violated rows give t < 0, the other warm
// row gives t ~ 0), and together they cover the dual pivot (a row of z_w is violated: the optimum moves
// back along p or q to the nearest blocking row), the primal step (a multiplier went negative: slide
// forward along the other row) and "nothing moved".  This only PROPOSES a pair -- any arithmetic will do;
// cert_pair then certifies it with the usual margins and evaluates the reference's formulas, so a wrong
// proposal costs a trip to the batches, never a wrong answer.
// Outputs: the proposed pair (p2, q2) -- valid row numbers -- with its rows, and whether it is usable at all.
template <int D, int BS>
__device__ __forceinline__ void cert_propose(const CertStage<D, BS> &S, double v0, double v1, int p0, int q0, bool pair_ok,
                                             int &p2, int &q2, bool &ok2, double (&prow)[3], double (&qrow)[3]
                                             ) {
    using C = CertStage<D, BS>;
    bool ok = pair_ok & (p0 != q0) & (p0 >= 0) & (q0 >= 0) & (p0 < C::nV) & (q0 < C::nV);
    const int p = ok ? p0 : 4, q = ok ? q0 : 5;
    double pa, pb, pc, qa, qb, qc;
    S.fetch(p, pa, pb, pc);
    S.fetch(q, qa, qb, qc);
    const double Dm = pa * qb - qa * pb;
    ok &= fabs(Dm) > kCertMinCross;
    const double rD = rcp_approx(Dm);  // the vertex only feeds margin tests / searches
    const double u = (pb * qc - qb * pc) * rD, x = (qa * pc - pa * qc) * rD;
    const double lamp = (v0 * qb - v1 * qa) * rD, lamq = (pa * v1 - pb * v0) * rD;
    // improving directions along the two lines
    const double vtp = -pb * v0 + pa * v1, vtq = -qb * v0 + qa * v1;
    const double dp0 = vtp < 0 ? pb : -pb, dp1 = vtp < 0 ? -pa : pa;
    const double dq0 = vtq < 0 ? qb : -qb, dq1 = vtq < 0 ? -qa : qa;
    // blocking rows along p and q: minimum of t = num / den over rows with den = n . d > 0 (num = -res)
    // (the running minimum starts at t = 1e300 / 1 instead of "none yet": one compare and one mask operation less
    // per row and line; rp / rq stay -1 until a row blocks)
    double np_ = 1e300, dp_ = 1.0, nq_ = 1e300, dq_ = 1.0;
    int rp = -1, rq = -1;
    auto row = [&](int vi, double a, double b, double res) {
        const double ep = a * dp0 + b * dp1, eq = a * dq0 + b * dq1, num = -res;
        const bool bp = (ep > 0.0) & (num * dp_ < np_ * ep);
        np_ = bp ? num : np_; dp_ = bp ? ep : dp_; rp = bp ? vi : rp;
        const bool bq = (eq > 0.0) & (num * dq_ < nq_ * eq);
        nq_ = bq ? num : nq_; dq_ = bq ? eq : dq_; rq = bq ? vi : rq;
    };
    // (the u box, +-1e8, is left out of the search: it binds in no sane problem, and cert_pair checks it anyway)
    row(2, 0.0, -1.0, S.low1 - x);
    row(3, 0.0, 1.0, x - S.high1);
    const double s45 = S.two_delta * u + x;
    row(4, -S.two_delta, -1.0, S.n0 - s45);
    row(5, S.two_delta, 1.0, s45 - S.n1);
    // acceleration rows, a +- pair at a time: on a line only the twin whose normal points along d blocks
#ifdef TPR_TOLERANCE_MODE  // contracted arithmetic: a row is no longer exactly parallel to its own line
    const int own_p = C::pair_of(p), own_q = C::pair_of(q);
#endif
    auto pair = [&](int vplus, int vminus, double a, double b, double cp, double cn) {
        // both residuals lowered by kBias (fused arithmetic is fine in a proposal): the line's own row, whose
        // residual is rounding noise of either sign over a denominator of exactly 0, must not look violated
        constexpr double kBias = 1e-11;
        const double sp = __builtin_fma(a, u, __builtin_fma(b, x, -kBias));
        const double resp = sp + cp, resn = cn - (sp + 2 * kBias);
#ifdef TPR_TOLERANCE_MODE
        const int pi = C::pair_of(vplus);
        const double ep = pi == own_p ? 0.0 : a * dp0 + b * dp1, eq = pi == own_q ? 0.0 : a * dq0 + b * dq1;
#else
        const double ep = a * dp0 + b * dp1, eq = a * dq0 + b * dq1;
#endif
        // a pair parallel to the line (den == 0: the line's own pair, a joint that stands still) has num > 0 -- the
        // own row's residual is ~0 - kBias, its twin's -(amax - amin), a null row's its c < 0 -- and never wins:
        // num dp_ > 0 = np_ den.  (A violated parallel row would win; no point of the line is feasible then and
        // cert_pair refuses.)
        {
            const bool pos = ep > 0.0;
            const double den = fabs(ep), num = pos ? -resp : -resn;
            const bool better = num * dp_ < np_ * den;
            np_ = better ? num : np_; dp_ = better ? den : dp_; rp = better ? (pos ? vplus : vminus) : rp;
        }
        {
            const bool pos = eq > 0.0;
            const double den = fabs(eq), num = pos ? -resp : -resn;
            const bool better = num * dq_ < nq_ * den;
            nq_ = better ? num : nq_; dq_ = better ? den : dq_; rq = better ? (pos ? vplus : vminus) : rq;
        }
    };
#pragma unroll
    for (int k = 0; k < D; ++k) pair(C::V0 + k, C::V1 + k, S.rc1[k], S.rc2[k], S.cpos[k], S.cneg[k]);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double q2v = S.rn2[k];
        pair(C::V2 + k, C::V3 + k, S.rn1[k] + S.two_delta * q2v, q2v, S.cpos[k], S.cneg[k]);
    }
    // pick the line
    const bool okp = lamp > 0, okq = lamq > 0;
    const bool hp = rp >= 0, hq = rq >= 0;
    // violated rows: candidates that move back (t < 0; the other warm row sits at t ~ 0, a residual of
    // rounding size); the one that gives up less objective wins
    const bool cp = hp & (np_ < -1e-9), cq = hq & (nq_ < -1e-9);
    const bool viol = cp | cq;
    const double gp = np_ * fabs(vtp) * dq_, gq = nq_ * fabs(vtq) * dp_;  // t (v . d), cross-multiplied
    const bool back_p = cp & (!cq | (gp >= gq));
    // (bitwise on purpose, no ?: -- the compiler would sink the products above into divergent branches)
    const bool use_p = (viol & back_p) | (!viol & okp & !okq);   // primal step: slide along the row whose multiplier is fine
    const bool use_q = (viol & cq & !back_p) | (!viol & okq & !okp);
    const bool keep = !ok | !(use_p | use_q);
    // the other warm row shows up as its own line's partner (t ~ 0): then nothing moved
    const int r = use_p ? rp : rq;  // -1: nothing blocks along the line (unbounded; refused)
    const bool from_q = !keep & !use_p;
    const int pA = from_q ? q : p, qA = (keep | (r < 0)) ? q : r;
    double ra, rb, rc;
    S.fetch(qA, ra, rb, rc);
    const bool both = false;
    const int ro = 5;
    const double oa = 0, ob = 0, oc = 0, res_o = 0;
    p2 = both ? r : pA;
    q2 = both ? ro : qA;
    prow[0] = both ? ra : (from_q ? qa : pa); prow[1] = both ? rb : (from_q ? qb : pb); prow[2] = both ? rc : (from_q ? qc : pc);
    qrow[0] = both ? oa : ra; qrow[1] = both ? ob : rb; qrow[2] = both ? oc : rc;
    ok2 = ok & (keep | (r >= 0)) & (p2 != q2) & !((p2 < 4) & (q2 < 4));
}

// Second version of the proposal (the default): ONE line search, along the row that must be active.
//
// Pass 1 over the rows finds the most violated one at the warm vertex z_w.  If there is one (v), it is active at
// the new optimum, which is the solution of the 1-D problem on v's line -- exactly the step the solver itself
// takes when it meets a violated row -- whether the partner turns out to be one of the warm rows (one pivot) or a
// third row (two pivots: a third of what version 1 left to the batches).  If no row is violated and a multiplier
// went negative, the line is the other warm row's (primal step).  Pass 2 is the blocking-row search along that
// one line, from a point on it (v: the foot of z_w; a warm row: z_w itself).  28 instead of 40 operations per
// pair of rows, and only a proposal as before: cert_pair_rows decides.
//
// SOUND mode (TPR_SOUND_CERTIFICATES, round 3): which moved pairs may be certified at all.  Conditions (A)-(C) of
// cert_pair_rows bound everything the reference's LAST pivot does; they say nothing about its EARLIER pivots, and one of
// those can end the reference's run with "infeasible" although the LP has a well separated optimum: a row r, slack at the
// optimum, that is violated (by as little as 1e-10) at an intermediate running optimum where two earlier rows cross r's
// line at the same point to within rounding -- the 1-D problem on r's line is then empty by 1e-14
// (tests/test_gpu_fullsize.py::test_concurrent_rows_and_sliver_pivots_are_bit_exact builds such stages: 1 in 1.5e5
// trajectories of that family, estimated 1e-5 events per 65536 x 200 natural batch, never observed in one).
// The WARM pair is immune: with it as warm start the reference visits its two rows first, reaches their vertex through
// 1-D problems bounded by the box and by each other (long segments: the vertex has margins to everything), and never
// pivots again.  In sound mode a MOVED pair is accepted only where the run is just as predictable: the warm vertex z_w is
// still the optimum of its own two rows (both multipliers positive), exactly ONE row v is violated there and every other
// row holds with the certificate's margin -- the reference walks from z_w straight to v, pivots, and its 1-D problem on
// v's line contains z* with margins on both sides -- and the blocker w is part of that 1-D problem: visited before v (a
// box row v is not visited at all: it moves the optimum inside the warm rows' own pivots, so its partner must be one of
// them).  Everything else -- a primal step (the reference then runs to the far end of a warm row's line and comes back
// through several pivots), several violated rows, a partner visited later -- runs the full iteration.  The default
// (fast) mode certifies every proposal as in round 2.
template <int D, int BS>
__device__ __forceinline__ void cert_propose2(const CertStage<D, BS> &S, double v0, double v1, int p0, int q0, bool pair_ok,
                                              bool sound, double nmax, int &p2, int &q2, bool &ok2, double (&prow)[3], double (&qrow)[3]
                                              ) {
    using C = CertStage<D, BS>;
    bool ok = pair_ok & (p0 != q0) & (p0 >= 0) & (q0 >= 0) & (p0 < C::nV) & (q0 < C::nV);
    const int p = ok ? p0 : 4, q = ok ? q0 : 5;
    double pa, pb, pc, qa, qb, qc;
    S.fetch(p, pa, pb, pc);
    S.fetch(q, qa, qb, qc);
    const double Dm = pa * qb - qa * pb;
    ok &= fabs(Dm) > kCertMinCross;
    const double rD = rcp_approx(Dm);  // the vertex only feeds margin tests / searches
    const double u = (pb * qc - qb * pc) * rD, x = (qa * pc - pa * qc) * rD;
    const double lamp = (v0 * qb - v1 * qa) * rD, lamq = (pa * v1 - pb * v0) * rD;
    constexpr double kBias = 1e-11;  // see cert_propose: a row through the point must not look violated by rounding
    // pass 1: the most violated row at z_w (fused arithmetic is fine in a proposal), and how many rows do NOT hold there
    // with the certificate's margin (sound mode: the two warm rows, residual ~0, and v -- one more disqualifies)
    const double tol_w = kCertSlack + kCertRelSlack * (nmax * (fabs(u) + fabs(x)) + fmax(S.cmax, fmax(fabs(S.n0), fabs(S.n1))));
    double worst = 1e-9;  // what counts as violated
    int v = -1, loose = 0;
    auto viol1 = [&](int vi, double res) {
        const bool w = res > worst; worst = w ? res : worst; v = w ? vi : v;
        loose += !(res < -tol_w);
    };
    viol1(2, S.low1 - x);
    viol1(3, x - S.high1);
    const double s45 = __builtin_fma(S.two_delta, u, x);
    viol1(4, S.n0 - s45);
    viol1(5, s45 - S.n1);
    auto viol2 = [&](int vplus, int vminus, double a, double b, double cp, double cn) {
        const double s = __builtin_fma(a, u, b * x);
        const double resp = s + cp, resn = cn - s;
        const bool plus = resp > resn;
        const double res = plus ? resp : resn;
        const bool w = res > worst;
        worst = w ? res : worst; v = w ? (plus ? vplus : vminus) : v;
        loose += !(res < -tol_w);  // (the other twin holds by the joint's range: min_range > tol in the certificate)
    };
#pragma unroll
    for (int k = 0; k < D; ++k) viol2(C::V0 + k, C::V1 + k, S.rc1[k], S.rc2[k], S.cpos[k], S.cneg[k]);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double q2v = S.rn2[k];
        viol2(C::V2 + k, C::V3 + k, S.rn1[k] + S.two_delta * q2v, q2v, S.cpos[k], S.cneg[k]);
    }
    // the line
    const bool viol = v >= 0, okp = lamp > 0, okq = lamq > 0;
    // nothing moved (or both multipliers gone -- sound mode: any multiplier gone -- : left to the batches)
    const bool keep = !ok | (!viol & (sound | !(okp ^ okq)));
    const int L = viol ? v : (okp ? p : q);          // primal step: slide along the row whose multiplier is fine
    double la, lb, lc;
    S.fetch(L, la, lb, lc);
    // a point on the line: z_w itself for a warm row, its foot on v otherwise
    const double n2 = __builtin_fma(la, la, lb * lb);
    double rn2 = __builtin_amdgcn_rcp(n2);
    rn2 = __builtin_fma(__builtin_fma(-n2, rn2, 1.0), rn2, rn2);
    const double step = viol ? worst * rn2 : 0.0;
    const double u0 = __builtin_fma(-step, la, u), x0 = __builtin_fma(-step, lb, x);
    const double vt = -lb * v0 + la * v1;
    const double d0 = vt < 0 ? lb : -lb, d1 = vt < 0 ? -la : la;  // improving direction along the line
    // pass 2: the blocking row, minimum of t = num / den over the rows with den = n . d > 0 (num = -res at the point)
    double bn = 1e300, bd = 1.0;
    int w = -1;
    auto row = [&](int vi, double a, double b, double res) {
        const double e = a * d0 + b * d1, num = kBias - res;
        const bool better = (e > 0.0) & (num * bd < bn * e);
        bn = better ? num : bn; bd = better ? e : bd; w = better ? vi : w;
    };
    row(2, 0.0, -1.0, S.low1 - x0);
    row(3, 0.0, 1.0, x0 - S.high1);
    const double t45 = __builtin_fma(S.two_delta, u0, x0);
    row(4, -S.two_delta, -1.0, S.n0 - t45);
    row(5, S.two_delta, 1.0, t45 - S.n1);
    auto pair = [&](int vplus, int vminus, double a, double b, double cp, double cn) {
        const double sp = __builtin_fma(a, u0, __builtin_fma(b, x0, -kBias));
        const double resp = sp + cp, resn = cn - (sp + 2 * kBias);
        const double e = a * d0 + b * d1;  // unfused: exactly 0 for the line's own pair
        const bool pos = e > 0.0;
        const double den = fabs(e), num = pos ? -resp : -resn;
        const bool better = num * bd < bn * den;
        bn = better ? num : bn; bd = better ? den : bd; w = better ? (pos ? vplus : vminus) : w;
    };
#pragma unroll
    for (int k = 0; k < D; ++k) pair(C::V0 + k, C::V1 + k, S.rc1[k], S.rc2[k], S.cpos[k], S.cneg[k]);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double q2v = S.rn2[k];
        pair(C::V2 + k, C::V3 + k, S.rn1[k] + S.two_delta * q2v, q2v, S.cpos[k], S.cneg[k]);
    }
    const bool moved = !keep & (w >= 0);
    q2 = moved ? w : q;
    double wa, wb, wc;
    S.fetch(q2, wa, wb, wc);
    // several violated rows: the most violated one need not be active, its blocker w usually is.  Of the pairs
    // (v, w), (p, w), (q, w) take the first whose multipliers are positive (signs only: no division).
    const double cw = v0 * wb - v1 * wa;
    auto dual_ok = [&](double aa, double ab) {
        const double dm = aa * wb - wa * ab, ma = aa * v1 - ab * v0;
        return (cw * dm > 0.0) & (ma * dm > 0.0);
    };
    const bool fl = dual_ok(la, lb), fp = dual_ok(pa, pb), fq = dual_ok(qa, qb);
    const bool alt = !sound & moved & viol & !fl & (fp | fq);
    const bool alt_q = alt & !fp;
    p2 = alt ? (alt_q ? q : p) : (moved ? L : p);
    const bool from_l = moved & !alt;
    prow[0] = from_l ? la : (alt_q ? qa : pa); prow[1] = from_l ? lb : (alt_q ? qb : pb); prow[2] = from_l ? lc : (alt_q ? qc : pc);
    qrow[0] = wa; qrow[1] = wb; qrow[2] = wc;
    // sound mode: "one violated row at a dual feasible warm vertex, partner inside its 1-D problem" (see above)
    const bool partner_first = (L < 4) ? ((q2 == p) | (q2 == q)) : (cert_pos(q2, p, q) < cert_pos(L, p, q));
    const bool predictable = okp & okq & (loose == 3) & partner_first;
    ok2 = ok & (keep | ((w >= 0) & (!sound | predictable))) & (p2 != q2) & !((p2 < 4) & (q2 < 4));
}

// Both backward LPs of a stage whose x_next rows form an equality  x + 2 delta u = n  (n0 == n1).
//
// Seidel visits the two x_next rows first (cold start: the reference's order is the identity), so from
// then on its running optimum lives on the equality line and every later pivot row k just cuts that
// line: on k's line the two x_next rows project to the same t (their (num, denom) are exact negatives
// of each other), one as a lower and one as an upper bound, so the 1-D LP has that single point.  The
// final vertex is where the row k* that binds along the line in the objective's direction crosses it,
// the last pivot is k* (it is violated on its visit because without it the optimum lies strictly
// further along the line -- margin-checked as in cert_pair), and the limiter is whichever x_next row
// has the bound class the 1-D objective picks.  E2: when the x box binds instead (the lower-bound LP of
// a rest-to-rest problem: x >= 0 at n = 0), no later row is violated and the last pivot is the first
// x_next row violated at the start corner, limited by the box row.  Everything is certified with the
// margins of cert_pair<EQ = true>; what does not fit goes to the batches' full iteration.
template <int D, int BS>
__device__ __forceinline__ void cert_equality(const CertStage<D, BS> &S, bool norms_ok, double nmax, int dn0, int dn1,
                                              int up0, int up1, Lp2dOut &ou, Lp2dOut &ol) {
    using C = CertStage<D, BS>;
    const double n = S.n0, d2 = S.two_delta;
    // binding rows along the line: u >= max of lower bounds (upper-bound LP, min u), u <= min of upper
    // bounds (lower-bound LP, max u); bounds are num / den with den > 0, compared by cross-multiplication
    double ln = 0, ld = 0, hn = 0, hd = 0;
    int lvi = -1, hvi = -1;
    auto lower_cand = [&](int vi, double num, double den) {  // u >= num / den
        const bool better = (den > 0.0) & ((lvi < 0) | (num * ld > ln * den));
        ln = better ? num : ln; ld = better ? den : ld; lvi = better ? vi : lvi;
    };
    auto upper_cand = [&](int vi, double num, double den) {  // u <= num / den
        const bool better = (den > 0.0) & ((hvi < 0) | (num * hd < hn * den));
        hn = better ? num : hn; hd = better ? den : hd; hvi = better ? vi : hvi;
    };
    upper_cand(2, n - S.low1, d2);   // x >= low1
    lower_cand(3, n - S.high1, d2);  // x <= high1
    auto pair = [&](int vplus, int vminus, double a, double b, double cp, double cn) {
        const double alpha = a - d2 * b, bp = b * n + cp, bn = cn - b * n;  // + row: alpha u + bp <= 0, - row: -alpha u + bn <= 0
        const bool pos = alpha > 0.0;
        const double den = fabs(alpha);
        lower_cand(pos ? vminus : vplus, pos ? bn : bp, den);
        upper_cand(pos ? vplus : vminus, pos ? -bp : -bn, den);
    };
#pragma unroll
    for (int k = 0; k < D; ++k) pair(C::V0 + k, C::V1 + k, S.rc1[k], S.rc2[k], S.cpos[k], S.cneg[k]);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double q2 = S.rn2[k];
        pair(C::V2 + k, C::V3 + k, S.rn1[k] + d2 * q2, q2, S.cpos[k], S.cneg[k]);
    }
    // limiter among the x_next rows for a structural pivot k: denominators on k's line are +-alpha_k
    // (row 5: +alpha_k); the 1-D objective picks the lower-bound class (denom < 0) when v1d < 0
    auto limiter = [&](int kvi, double v0, double v1) {
        double ka, kb, kc;
        S.fetch(kvi, ka, kb, kc);
        const double alpha = ka - d2 * kb, v1d = -kb * v0 + ka * v1;
        return ((v1d < 0) == (alpha < 0)) ? 5 : 4;
    };
    {   // upper-bound LP: binding lower bound on u; only a structural row is handled (E1)
        const bool have = lvi >= C::V0;
        const int k = have ? lvi : C::V0;
        cert_pair<D, BS, true>(S, -1e-9, 1.0, k, limiter(k, -1e-9, 1.0), have, dn0, dn1, norms_ok, nmax, ou);
    }
    {   // lower-bound LP: a structural row (E1) or the box row x >= low1 (E2, cold start only)
        const bool e1 = hvi >= C::V0;
        const bool cold = !((up0 >= 4) & (up1 >= 4) & (up0 != up1));
        // start corner (high0, low1): row 0 (vi 4) clearly satisfied, row 1 (vi 5) clearly violated -> pivot row 1
        const bool corner = (-d2 * kVarMax - S.low1 + n < -1.0) & (d2 * kVarMax + S.low1 - n > 1.0);
        const bool e2 = (hvi == 2) & cold & corner;
        const int k = e1 ? hvi : 2;
        cert_pair<D, BS, true>(S, 1e-9, -1.0, k, e1 ? limiter(k, 1e-9, -1.0) : 5, e1 | e2, up0, up1, norms_ok, nmax, ol);
    }
}

template <int D, int BS, bool UMAX, bool TRACE = false>
__device__ __forceinline__ bool cert_lower_finish(const CertStage<D, BS> &S, bool norms_ok, double nmax, int r_vi, double u1, Lp2dOut &o,
                                                  const double *row = nullptr);

// Lower-bound LP of a backward stage from the vertex (u*, low1): see predict_lower_lp.
// UMAX: the sign of the objective's tilt in u.  true: max 1e-9 u - x (the backward scan's lower-bound LP: u* on the
// tightest UPPER bound at x = low1).  false: max -1e-9 u - x (compute_feasible_sets' lower-bound LP,
// reachability_algorithm.py:149-157: u* on the tightest LOWER bound) -- the mirror image under u -> -u: rows (a, b, c)
// become (-a, b, c), so the search runs on sg a and sg u with sg = -1, while the margin scan and the reference's
// last-pivot formulas see the rows as they are.
template <int D, int BS, bool UMAX = true>
__device__ __forceinline__ bool cert_lower(const CertStage<D, BS> &S, bool norms_ok, double nmax, Lp2dOut &o) {
    const double low1 = S.low1;
    // tightest upper bound on u at x = low1: running minimum of -g/a over the rows with a > 0 (of a
    // +- pair that is the one with a > 0), compared by cross-multiplication -- this is search
    // (starts at 1e300 / 1 instead of "none yet"; a null row, a = 0, has mg > 0 and never wins: mg bd > 0 = bn a)
    double bn = 1e300, bd = 1.0;
    int r_vi = -1;
    auto cand = [&](int vi, double a, double mg) {  // a >= 0, bound = mg / a
        const bool better = mg * bd < bn * a;
        bn = better ? mg : bn;
        bd = better ? a : bd;
        r_vi = better ? vi : r_vi;
    };
    if (UMAX) cand(5, S.two_delta, S.n1 - low1);  // row 4 has a < 0
    else cand(4, S.two_delta, low1 - S.n0);       // mirrored: row 4 bounds u from below, row 5 from above
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double a = S.rc1[k], bl = S.rc2[k] * low1;
        const bool posr = UMAX ? a > 0.0 : a < 0.0;  // which twin bounds u from above (UMAX) / from below
        cand(posr ? CertStage<D, BS>::V0 + k : CertStage<D, BS>::V1 + k, fabs(a), posr ? -(bl + S.cpos[k]) : bl - S.cneg[k]);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double q2 = S.rn2[k];
        const double a = S.rn1[k] + S.two_delta * q2, bl = q2 * low1;
        const bool posr = UMAX ? a > 0.0 : a < 0.0;
        cand(posr ? CertStage<D, BS>::V2 + k : CertStage<D, BS>::V3 + k, fabs(a), posr ? -(bl + S.cpos[k]) : bl - S.cneg[k]);
    }
    const double u1m = bn * rcp_approx(bd);  // only for the margin tests: the answer comes from cert_last_pivot
    return cert_lower_finish<D, BS, UMAX>(S, norms_ok, nmax, r_vi, UMAX ? u1m : -u1m, o);
}

// The rest of the lower-bound certificate: the binding row r_vi (-1: none) with u1 ~ the u of its crossing with the wall.
// TRACE (round 5, the caller is cert_lower_sound): the margin scan only says "all hold" -- one sign bit per +- pair.
template <int D, int BS, bool UMAX, bool TRACE>
__device__ __forceinline__ bool cert_lower_finish(const CertStage<D, BS> &S, bool norms_ok, double nmax, int r_vi, double u1, Lp2dOut &o,
                                                  const double *row) {
    const double low1 = S.low1;
    bool ok = norms_ok & (r_vi >= 0);
    r_vi = r_vi >= 0 ? r_vi : (UMAX ? 5 : 4);
    ok &= (u1 < kVarMax - 1.0) & (u1 > kVarMin + 1.0);
    double pa, pb, pc;
    if (TRACE) { pa = row[0]; pb = row[1]; pc = row[2]; }  // (the caller has fetched row r_vi, a valid row number, already)
    else S.fetch(r_vi, pa, pb, pc);
    // every other structural row holds at z* = (u1, low1) with a margin
    const double au1 = fabs(u1), al = fabs(low1);
    const double tol_s = kCertSlack + kCertRelSlack * (nmax * (au1 + al) + fmax(S.cmax, fmax(fabs(S.n0), fabs(S.n1))));
    const int pr = CertStage<D, BS>::pair_of(r_vi);
    double ms = -3.0e300;
    const double s45 = S.two_delta * u1 + low1;
    if (UMAX) {
        ms = fmax(ms, S.n0 - s45);
        ms = fmax(ms, cert_unless(r_vi == 5, s45 - S.n1));
    } else {
        ms = fmax(ms, cert_unless(r_vi == 4, S.n0 - s45));
        ms = fmax(ms, s45 - S.n1);
    }
    bool rows_hold = true;
    if constexpr (TRACE) {
        static_assert(2 * D <= 32, "one word of pair bits");
        const unsigned own = (unsigned)(pr >= 0) << ((2 * D - 1 - pr) & 31);
        unsigned held = 0u;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double s = __builtin_fma(S.rc1[k], u1, S.rc2[k] * low1);
            held = cert_push_sign(held, fmax(s + S.cpos[k], S.cneg[k] - s) + tol_s);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double q2 = S.rn2[k];
            const double s = __builtin_fma(S.rn1[k] + S.two_delta * q2, u1, q2 * low1);
            held = cert_push_sign(held, fmax(s + S.cpos[k], S.cneg[k] - s) + tol_s);
        }
        rows_hold = ((held | own) & (unsigned)((1ull << (2 * D)) - 1ull)) == (unsigned)((1ull << (2 * D)) - 1ull);
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double s = S.rc1[k] * u1 + S.rc2[k] * low1;
            const double m2 = fmax(s + S.cpos[k], S.cneg[k] - s);
            ms = fmax(ms, cert_unless(pr == k, m2));
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double q2 = S.rn2[k];
            const double s = (S.rn1[k] + S.two_delta * q2) * u1 + q2 * low1;
            const double m2 = fmax(s + S.cpos[k], S.cneg[k] - s);
            ms = fmax(ms, cert_unless(pr == D + k, m2));
        }
    }
    ok &= (ms + tol_s < 0) & rows_hold & (S.min_range > tol_s);
#ifdef TPR_TOLERANCE_MODE
    o.ok = ok & ((UMAX ? pa : -pa) > 1e-6) & (pb > -1e8 * (UMAX ? pa : -pa)); o.u = u1; o.x = low1; o.ac0 = r_vi; o.ac1 = 2;
    return o.ok;
#endif
#ifdef TPR_SOUND_TOLERANCE  // (see cert_pair_rows: the vertex itself, no cross-product guard)
    if constexpr (TRACE) {
        o.ok = ok & ((UMAX ? pa : -pa) > 1e-6) & (pb > -1e8 * (UMAX ? pa : -pa)) & (fabs(pc) < 1e15); o.u = u1; o.x = low1; o.ac0 = r_vi; o.ac1 = 2;
        return o.ok;
    }
#endif
    ok &= cert_cross_ok<D, BS>(S, pa, pb);
    // the pivot row itself: well conditioned, and the tilt (1e-9) must not make a larger x worthwhile
    const double pam = UMAX ? pa : -pa;
    ok &= (pam > 1e-6) & (pb > -1e8 * pam) & (fabs(pc) < 1e15);
    o.ok = ok;
    cert_last_pivot(pa, pb, pc, 0.0, -1.0, low1, o.u, o.x);
    o.ac0 = r_vi;  // internal numbering: the binding row and the box row x >= low1
    o.ac1 = 2;
    return ok;
}

// =====================================================================================================================
// SOUND proposals (round 4): the reference's pivot TRACE, followed with margins.
//
// cert_pair_rows bounds everything the reference's LAST pivot does.  Its earlier pivots can end the run too ("infeasible":
// an intermediate 1-D problem that is empty by rounding -- cy_seidel_solverwrapper.pyx:127,:342,:353 -- although the LP has
// a well separated optimum), so a certificate may only answer where EVERY pivot of the reference's run is predictable.
// What the run looks like (tools/pivot_trace.c on the benchmark's batches, 96 % of the LPs whose pair moved, and every
// kept pair): from the start corner the first two rows of the visiting order (the warm pair: w1, then w0; rows 0, 1 of a
// cold start) pivot against the box and each other; from the vertex (A, B) they leave, every later pivot row r is limited by
// the SAME row L of {A, B} -- the running optimum slides along L's line, and the pivot rows are the prefix records, in
// visiting order, of where the rows cut that line.  Along a line every residual is linear in the parameter t, so ONE pass
// over the rows follows the whole slide:
//   * a row visited while the optimum sits at t_cur must be robustly satisfied or robustly violated there
//     (|residual| > tol: the reference's own test is "< 1e-10" on a value with ~1e-16 relative rounding);
//   * a violated row must cut the line further on (a "pusher": its residual falls along the slide), the vertex it forms
//     with L must be dual feasible (the 1-D objective on its line points at L: sign of its v1d) and the previous record row
//     must hold there with the margin -- then every row visited before it holds at that vertex with the margin (pushers:
//     their residual fell from a robustly negative value or they are older records; blockers: their residual rises
//     towards the final vertex, where cert_pair_rows demands the margin), so the 1-D problem on its line has a long
//     feasible segment bounded by L with every other bound a margin away: no sliver, no parallel-row exit (a row parallel
//     to it within the solver's 1e-10 keeps its residual along the line to within 1e-10 |distance| / |n|, far inside
//     the margin), and the limiter the reference finds is L.
// Anything else -- a pivot limited by a third row, an ambiguous test, a degenerate start -- is not certified and runs the
// reference's iteration in the cooperative batches.

#ifdef TPR_CERT_WHY  // host harness only: why a proposal was refused
#define TPR_WHY(code, cond) do { if (!(cond) && tpr_cert_why == 0) tpr_cert_why = (code); } while (0)
static thread_local int tpr_cert_why = 0;
#else
#define TPR_WHY(code, cond)
#endif

// The improving end of the 1-D problem on the line of row (la, lb, lc) subject to the four box rows and one optional
// structural row (oa, ob, oc; `have_o`): the reference's pivot on one of the first two rows of its order.
// Returns the limiter (internal row number: 0..3 a box row, `o_vi` the other row; -1: not predictable) and the new point.
template <int D, int BS>
__device__ __forceinline__ int cert_box_pivot(const CertStage<D, BS> &S, double v0, double v1, double la, double lb, double lc,
                                              bool have_o, int o_vi, double oa, double ob, double oc, double nmax, double cbig,
                                              double &pu, double &px, double (&lrow)[3]) {
    // the line must cross both box directions properly (the reference tests |denom| against 1e-10: denom = +-la, +-lb)
    bool ok = (fabs(la) > kCertMinCross) & (fabs(lb) > kCertMinCross);
    const double v1d = -lb * v0 + la * v1;
    ok &= fabs(v1d) > 1e-6;
    const double sg = v1d < 0 ? -1.0 : 1.0;
    const double g0 = -lb * sg, g1 = la * sg;  // improving direction along the line
    // walls hit in direction g: u -> (g0 > 0 ? high0 : low0), x -> (g1 > 0 ? high1 : low1); parametrise by the wall itself
    const double uw = g0 > 0 ? kVarMax : kVarMin, xw = g1 > 0 ? S.high1 : S.low1;
    const double r_la = rcp_approx(la), r_lb = rcp_approx(lb);
    // the line's point on the x wall / on the u wall
    const double u_at_xw = -(lb * xw + lc) * r_la, x_at_uw = -(la * uw + lc) * r_lb;
    // which wall comes first: the x wall iff the line's point on it lies inside the u range (with a margin)
    const bool x_first = fabs(u_at_xw) < kVarMax * (1.0 - 1e-6);
    const bool u_first = (x_at_uw > S.low1 + 1e-6 * (1.0 + fabs(S.low1))) & (x_at_uw < S.high1 - 1e-6 * (1.0 + fabs(S.high1)));
    ok &= x_first != u_first;
    double qu = x_first ? u_at_xw : uw, qx = x_first ? xw : x_at_uw;
    int lim = x_first ? (g1 > 0 ? 3 : 2) : (g0 > 0 ? 1 : 0);
    // the limiter's row (what CertStage::fetch(lim) returns: rows 0..3 are (-1, 0, low0), (1, 0, -high0), (0, -1, low1), (0, 1, -high1))
    double ma = x_first ? 0.0 : (g0 > 0 ? 1.0 : -1.0), mb = x_first ? (g1 > 0 ? 1.0 : -1.0) : 0.0;
    double mc = x_first ? (g1 > 0 ? -S.high1 : S.low1) : (g0 > 0 ? -kVarMax : kVarMin);
    // the other row: does it stop the line before the wall?  Its residual at the wall point decides (with the margin)
    const double tol_q = kCertSlack + kCertRelSlack * (nmax * (fabs(qu) + fabs(qx)) + cbig);
    if (have_o) {  // (callers pass have_o = false at an equality stage, where the other row is the line's exact twin)
        const double ro = oa * qu + ob * qx + oc;
        const double Dm = la * ob - oa * lb;
        const bool cut = ro > tol_q;  // violated at the wall point: the optimum is where the two rows cross ...
        ok &= cut | (ro < -tol_q);
        ok &= !cut | (fabs(Dm) > kCertMinCross);
        const double rD = rcp_approx(Dm);
        const double zu = (lb * oc - ob * lc) * rD, zx = (oa * lc - la * oc) * rD;
        // ... provided the crossing lies BEHIND the wall point along g (else the other row bounds the far side only, and
        // a row that is violated on the whole near side means an empty problem: not predictable)
        const double back = (qu - zu) * g0 + (qx - zx) * g1;
        ok &= !cut | (back > 0);
        qu = cut ? zu : qu; qx = cut ? zx : qx;
        lim = cut ? o_vi : lim;
        ma = cut ? oa : ma; mb = cut ? ob : mb; mc = cut ? oc : mc;
        // at the crossing the walls must hold with the margin
        const double tol_z = kCertSlack + kCertRelSlack * (nmax * (fabs(qu) + fabs(qx)) + cbig);
        ok &= !cut | ((fabs(qu) < kVarMax * (1.0 - 1e-6)) & (S.low1 - qx < -tol_z) & (qx - S.high1 < -tol_z));
    }
    // the box must be a box (a long segment behind the optimum as well)
    ok &= S.high1 - S.low1 > 1e-6 * (1.0 + fabs(S.high1) + fabs(S.low1));
    pu = qu; px = qx;
    lrow[0] = ma; lrow[1] = mb; lrow[2] = mc;
    return ok ? lim : -1;
}

constexpr double kPrevRecordSlack = 1e-2;  // margin of the previous record at the new one, in units of tol
// Relative part of the margins along the trace: the points of a trace can lie far out (|u| ~ 1e6 where a line meets the box),
// where a residual is a difference of large terms; 1e-12 of those terms is still 1e4 x their rounding (reference and
// proposal alike), while the 1e-9 of the final vertex's margins would swallow every decision made from such a start.
constexpr double kTraceRelSlack = 1e-12;

// The phases of a stage's certificates are independent enough for the scheduler to interleave all of them, which multiplies
// the registers in flight (round 4: 600 B of scratch per lane); a fence between phases keeps each one's values short-lived.
#if defined(__HIP_DEVICE_COMPILE__)
#define TPR_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define TPR_SCHED_FENCE()
#endif

// Running record of a slide: t_cur = Nn / Dn with Dn = |e| of the record row.  One visit of a row in the reference's order:
// res = its residual at the start point, e = the slope of its residual along the slide, w = its v1d (the 1-D objective on
// its own line).  Everything a visit has to establish is folded into ONE running minimum (`acc` must end up positive): a
// single wave issues an instruction of any kind every ~5 cycles, so a compare into a lane mask and the mask logic behind it
// cost as much as arithmetic -- the boolean form of this step was 17 vector + 8 scalar instructions per row.
//   not violated at t_cur:  -(rho + thr) > 0          (clearly satisfied: rho = Dn x residual at t_cur, thr = Dn x tol)
//   violated (rho > thr):   a record -- min of  -e - kCertMinCross  (a pusher, clearly crossing L),
//                                               rho + kPrevRecordSlack tol e  (the previous record holds at the new one),
//                                               sg w - 1e-6  (its vertex with L is dual feasible; not on an equality line)
// PRECONDITIONS of the accumulator (ADVICE r4): fmin() drops a NaN operand, so a NaN verdict would read as "clearly satisfied".
// No quantity of a visit can be NaN or infinite when (i) the rows are finite and at most 1e6 long -- CertStage::norms, which
// every certificate's `ok` carries -- (ii) the start point of the slide is finite, |u0|, |x0| <= 1e8-ish, and (iii) the tolerance
// is finite: then |res|, |e|, |w| <= 1e15, the record's fraction |Nn|, |Dn| <= 1e15 and every product below stays under 1e31.
// (ii) and (iii) are checked where a slide starts (cert_slide, cert_slide_wall: `finite`), not per visit.
struct SlideState {
    double Nn, Dn, acc;
    unsigned bad;  // SB form: bit 31 = some visit was not predictable
    int rec;
};
// SB (round 5): the verdicts go into the SIGN BITS of the high words instead of a running minimum of doubles -- everything a
// visit demands is "this quantity is positive", so the high words are or-ed into one flag word (v_or3_b32), the violated-row
// demands under one 32-bit select, and bit 31 of the word is the answer: 7 instructions of bookkeeping per visit where the
// minimum form takes 10 (headline kernel: -0.06 ms).  Same verdicts under the preconditions above (finite quantities; an exact 0,
// which the minimum form refuses, is accepted -- a tie at the tolerance boundary, 1e4 x rounding away from any decision).  NOT used
// by the TOPPRAsd instantiations: cert_solve_kernel<5, ..., SDFWD> built with it returned wrong forward profiles (K correct; -O1
// for that translation unit correct; profiles/r05_sd5_signbit_miscompile.log) -- one more instance of DESIGN section 9's defect.
template <bool EQLINE, bool WALL = false, bool SB = false>
__device__ __forceinline__ void cert_slide_visit(SlideState &T, int vi, double res, double e, double w, double sg, double tol) {
    const double rho = __builtin_fma(res, T.Dn, e * T.Nn);
    const double thr = tol * T.Dn;
    const bool viol = rho > thr;
    const double s1 = WALL ? w : -e - kCertMinCross;                            // a pusher, clearly crossing L (WALL: and dual feasible)
    const double s2 = __builtin_fma(kPrevRecordSlack * tol, e, rho);            // the previous record holds at the new one
    if constexpr (SB) {
        const double clear = fabs(rho) - thr;                                   // > 0: a clear verdict either way
        unsigned m = (unsigned)__double2hiint(s1) | (unsigned)__double2hiint(s2);
        if (!EQLINE && !WALL) m |= (unsigned)__double2hiint(__builtin_fma(sg, w, -1e-6));    // its vertex with L is dual feasible
        T.bad |= (unsigned)__double2hiint(clear) | (viol ? m : 0u);
    } else {
        double score = fmin(s1, s2);
        if (!EQLINE && !WALL) score = fmin(score, __builtin_fma(sg, w, -1e-6));
        const double q = viol ? score : -rho - thr;
        T.acc = fmin(T.acc, q);
    }
#ifdef TPR_CERT_WHY
    TPR_WHY(10, viol | (-rho - thr > 0));
    TPR_WHY(11, !viol | WALL | (-e - kCertMinCross > 0));
    TPR_WHY(11, !viol | !WALL | (w > 0));
    TPR_WHY(12, !viol | (__builtin_fma(kPrevRecordSlack * tol, e, rho) > 0));
    TPR_WHY(13, !viol | EQLINE | WALL | (__builtin_fma(sg, w, -1e-6) > 0));
#endif
    T.Nn = viol ? res : T.Nn;
    T.Dn = viol ? -e : T.Dn;
    T.rec = viol ? vi : T.rec;
}

// The rows a scan does not visit (the first two rows of the order, L, R0), as bits over the internal row numbers: up to 40
// of them to 8 dof, 80 above (block stride 16): three words.
struct RowMask {
    unsigned w[3];
    __device__ __forceinline__ RowMask() : w{0u, 0u, 0u} {}
    __device__ __forceinline__ void set(int vi) {  // vi: a runtime row number, 0 <= vi < 96
        const unsigned bit = 1u << (vi & 31);
        w[0] |= (vi >> 5) == 0 ? bit : 0u;
        w[1] |= (vi >> 5) == 1 ? bit : 0u;
        w[2] |= (vi >> 5) == 2 ? bit : 0u;
    }
    // The residual of row vi (a compile-time number at every call), or a hugely negative one -- clearly satisfied, never a
    // record -- when its bit is set: a sign-extending bit-field extract and a bitwise select on the high word (cert_unless_bit).
    __device__ __forceinline__ double res(int vi, double r) const {
        const int m = (int)(w[vi >> 5] << (31 - (vi & 31))) >> 31;  // 0 or -1
        return __hiloint2double((m & (int)0xfe51eb2du) | (~m & __double2hiint(r)), __double2loint(r));
    }
};

// One slide along the line of row L = (La, Lb, .) from the point (u0, x0) on it, in the direction that leaves row R0
// (the other row through the start point; normal (Ra, Rb)) behind: the prefix records of the rows in visiting order -- the
// structural rows 4, 5, acceleration blocks 0..3 in index order, without the rows whose bit is set in `skip` (bit vi: the
// first two rows of the order, L and R0).  Returns false when the run is not predictable; `rec` = the last record row
// (-1: no row is violated at the start point).
// EQLINE: L is the line of an equality stage's two x_next rows -- on a record's line they leave a single point, which is
// the 1-D optimum whatever the objective's direction: no dual test.
template <int D, int BS, bool EQLINE = false, bool SB = false>
__device__ __forceinline__ bool cert_slide(const CertStage<D, BS> &S, double v0, double v1, bool L_is_box, double La, double Lb,
                                           double Ra, double Rb, double u0, double x0, const RowMask &skip, double tol, int &rec) {
    using C = CertStage<D, BS>;
    // direction: R0's residual falls along it
    const double eR = -Lb * Ra + La * Rb;            // n_R0 . (-Lb, La)
    const double sg = eR > 0 ? -1.0 : 1.0;
    const double d0 = -Lb * sg, d1 = La * sg;
    SlideState T;
    bool ok = fabs(eR) > kCertMinCross;
    TPR_WHY(14, ok);
    ok &= fabs(u0) + fabs(x0) + tol < 1e300;  // finite start point and tolerance (see SlideState): a NaN compares false
    // the objective falls along the slide, clearly (along a box row the value is exactly -+v0 or -+v1: its sign is all
    // there is to ask)
    const double vd = v0 * d0 + v1 * d1;
    ok &= vd < (L_is_box ? 0.0 : -1e-6);
    TPR_WHY(15, vd < (L_is_box ? 0.0 : -1e-6));
    T.Nn = 0.0; T.Dn = fabs(eR); T.rec = -1; T.acc = 1.0; T.bad = 0u;
    {
        const double s45 = __builtin_fma(S.two_delta, u0, x0), e45 = __builtin_fma(S.two_delta, d0, d1), w45 = __builtin_fma(S.two_delta, v1, -v0);
        cert_slide_visit<EQLINE, false, SB>(T, 4, skip.res(4, S.n0 - s45), -e45, -w45, sg, tol);
        cert_slide_visit<EQLINE, false, SB>(T, 5, skip.res(5, s45 - S.n1), e45, w45, sg, tol);
    }
    // an acceleration block pair (+ rows, then - rows): the twins share their products
    auto blocks = [&](int vplus, int vminus, const double (&aa)[D], const double (&bb)[D]) {
        double s[D], e[D], w[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            s[k] = __builtin_fma(aa[k], u0, bb[k] * x0);
            e[k] = __builtin_fma(aa[k], d0, bb[k] * d1);
            w[k] = __builtin_fma(aa[k], v1, -(bb[k] * v0));
        }
#pragma unroll
        for (int k = 0; k < D; ++k) cert_slide_visit<EQLINE, false, SB>(T, vplus + k, skip.res(vplus + k, s[k] + S.cpos[k]), e[k], w[k], sg, tol);
        TPR_SCHED_FENCE();
#pragma unroll
        for (int k = 0; k < D; ++k) cert_slide_visit<EQLINE, false, SB>(T, vminus + k, skip.res(vminus + k, S.cneg[k] - s[k]), -e[k], -w[k], sg, tol);
        TPR_SCHED_FENCE();
    };
    blocks(C::V0, C::V1, S.rc1, S.rc2);
    {
        double an[D];
#pragma unroll
        for (int k = 0; k < D; ++k) an[k] = S.rn1[k] + S.two_delta * S.rn2[k];
        blocks(C::V2, C::V3, an, S.rn2);
    }
    rec = T.rec;
    return ok & (SB ? !(T.bad >> 31) : T.acc > 0.0);
}

// The slide of a lower-bound LP along the box row of x (x = xw: the wall the objective runs into) from (u0, xw), in the
// direction sg_u of u (-1: u falls -- the backward scan's lower-bound LP; +1: compute_feasible_sets' min-x LP), leaving the
// x_next row `r0` (5 / 4) behind: cert_slide with d = (sg_u, 0), where the slope of a row's residual is sg_u a and nothing
// needs multiplying out.  Rows 4, 5 are not visited (the prologue has).
template <int D, int BS, bool SB = false>
__device__ __forceinline__ bool cert_slide_wall(const CertStage<D, BS> &S, double sg_u, double u0, double xw, double tol, int &rec) {
    using C = CertStage<D, BS>;
    SlideState T;
    T.Nn = 0.0; T.Dn = S.two_delta; T.rec = -1; T.acc = 1.0; T.bad = 0u;
    // (cert_slide for L = (0, -1, xw): d = (-Lb sg, La sg) = (sg, 0), i.e. its direction sign IS sg_u)
    // A record must be a pusher that clearly crosses the wall (-e = -sg_u a > 1e-7) whose vertex with the wall is dual feasible
    // (sg w - 1e-6 > 0 with w = a v1 - b v0, v1 = -1, -sg_u v0 = 1e-9: -sg_u a + 1e-9 b > 1e-6).  Both follow from
    //     -sg_u a - (1e-9 |b| + 1e-6) > 0,
    // one score per row with the bracket shared by the twins (round 5: two products and two scores per row before).
    auto blocks = [&](int vplus, int vminus, const double (&aa)[D], const double (&bb)[D]) {
        double s[D], c[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            s[k] = __builtin_fma(aa[k], u0, bb[k] * xw);
            c[k] = __builtin_fma(1e-9, fabs(bb[k]), 1e-6);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) cert_slide_visit<false, true, SB>(T, vplus + k, s[k] + S.cpos[k], sg_u * aa[k], -sg_u * aa[k] - c[k], sg_u, tol);
        TPR_SCHED_FENCE();
#pragma unroll
        for (int k = 0; k < D; ++k) cert_slide_visit<false, true, SB>(T, vminus + k, S.cneg[k] - s[k], -sg_u * aa[k], sg_u * aa[k] - c[k], sg_u, tol);
        TPR_SCHED_FENCE();
    };
    blocks(C::V0, C::V1, S.rc1, S.rc2);
    {
        double an[D];
#pragma unroll
        for (int k = 0; k < D; ++k) an[k] = S.rn1[k] + S.two_delta * S.rn2[k];
        blocks(C::V2, C::V3, an, S.rn2);
    }
    rec = T.rec;
    return (S.two_delta > kCertMinCross) & (SB ? !(T.bad >> 31) : T.acc > 0.0) & (fabs(u0) + fabs(xw) + tol < 1e300);  // (finite: see SlideState)
}

// The pair the reference's run ends on, for the LP  max v0 u + v1 x  with the warm start (w0, w1): prologue (the first two
// rows of the order against the box and each other), the first violated row at the vertex they leave, the slide along the
// row that limits it.  (p2, q2) with their rows go to cert_pair_rows, which certifies the final vertex as before; ok2 =
// the run is predictable up to there.
// MODE 0: the general case (the line of the slide is chosen from the first violated row).
// MODE 1: the line is the prologue's LIMITER without asking (the lower-bound LPs: x sits on its box bound and the rows cut
//         that wall; pass 1 is skipped -- a wrong guess fails the slide's own tests and is refused).
// MODE 2: an equality stage (n0 == n1: the x_next rows are one line, each other's exact twin): the first x_next row that the
//         start corner violates pivots against the box, the other one lies on its line (residual: rounding) and is skipped,
//         and every later pivot slides along that line.  The reported pair is (last record, the line's row): the caller
//         picks which of the two x_next rows the reference names as limiter.
template <int D, int BS, int MODE = 0, bool SB = false>
__device__ __forceinline__ void cert_propose_sound(const CertStage<D, BS> &S, double v0, double v1, int w0, int w1, bool pair_ok,
                                                   double nmax, int &p2, int &q2, bool &ok2, double (&prow)[3], double (&qrow)[3]) {
    using C = CertStage<D, BS>;
    const bool warm = (MODE != 2) & pair_ok & (w0 >= 4) & (w1 >= 4) & (w0 != w1) & (w0 < C::nV) & (w1 < C::nV);
    const int f0 = warm ? w1 : 4, f1 = warm ? w0 : 5;  // the first two rows of the visiting order
    double a0, b0, c0, a1, b1, c1;
    S.fetch(f0, a0, b0, c0);
    S.fetch(f1, a1, b1, c1);
    // scale of a structural row's constant (the box rows are tested on their own scale in cert_box_pivot)
    const double cbig = fmax(S.cmax, fmax(fabs(S.n0), fabs(S.n1)));
    // start corner (cy_seidel_solverwrapper.pyx:232-247)
    double pu = v0 > kTiny ? kVarMax : kVarMin, px = v1 > kTiny ? S.high1 : S.low1;
    bool ok = true;
    int A = -1, B = -1;  // the vertex the prologue leaves: last pivot row, its limiter
    double Brow[3] = {0.0, -1.0, S.low1};  // ... and the limiter's row (row 2 until a pivot names one)
    // (straight-line on purpose: a branch around a pivot is divergent, and the compiler then duplicates everything that follows
    // for the two paths -- two copies of the slide, both executed by every wave)
    {   // k = 0
        const double r = a0 * pu + b0 * px + c0;
        const double tol = kCertSlack + kCertRelSlack * (nmax * (fabs(pu) + fabs(px)) + cbig);
        ok &= fabs(r) > tol;
        TPR_WHY(1, fabs(r) > tol);
        double qu, qx;
        double lr[3];
        const int lim = cert_box_pivot<D, BS>(S, v0, v1, a0, b0, c0, false, -1, 0.0, 0.0, 0.0, nmax, cbig, qu, qx, lr);
        const bool piv = r > 0;
        ok &= !piv | (lim >= 0);
        TPR_WHY(2, !piv | (lim >= 0));
        A = piv ? f0 : A; B = piv ? lim : B; pu = piv ? qu : pu; px = piv ? qx : px;
        Brow[0] = piv ? lr[0] : Brow[0]; Brow[1] = piv ? lr[1] : Brow[1]; Brow[2] = piv ? lr[2] : Brow[2];
    }
    {   // k = 1
        const double r = a1 * pu + b1 * px + c1;
        const double tol = kCertSlack + kCertRelSlack * (nmax * (fabs(pu) + fabs(px)) + cbig);
        // (equality stage: once the first x_next row has pivoted, the second one lies on its line -- its residual there is
        // rounding noise far below the solver's 1e-10 -- and is not visited as a pivot)
        const bool twin_done = (MODE == 2) & (A >= 0);
        ok &= twin_done | (fabs(r) > tol);
        TPR_WHY(3, twin_done | (fabs(r) > tol));
        double qu, qx;
        double lr[3];
        const int lim = cert_box_pivot<D, BS>(S, v0, v1, a1, b1, c1, MODE != 2, f0, a0, b0, c0, nmax, cbig, qu, qx, lr);
        const bool piv = !twin_done & (r > 0);
        ok &= !piv | (lim >= 0);
        TPR_WHY(4, !piv | (lim >= 0));
        A = piv ? f1 : A; B = piv ? lim : B; pu = piv ? qu : pu; px = piv ? qx : px;
        Brow[0] = piv ? lr[0] : Brow[0]; Brow[1] = piv ? lr[1] : Brow[1]; Brow[2] = piv ? lr[2] : Brow[2];
    }
    ok &= (A >= 0) & (B >= 0);
    TPR_WHY(5, (A >= 0) & (B >= 0));
    A = A >= 0 ? A : 4; B = B >= 0 ? B : 2;  // (any valid rows keep the arithmetic defined)
    // pass 1: the first row, in visiting order, that does not clearly hold at the vertex -- it must be clearly violated
    const double tol_p = kCertSlack + kTraceRelSlack * (nmax * (fabs(pu) + fabs(px)) + cbig);
    int r1 = -1;
    bool r1_viol = false;
    TPR_SCHED_FENCE();
    if (MODE == 0) {
        // One bit per row in visiting order (cert_push_sign): rows 4, 5 and the blocks of s_i into `wa` (2 + 2 D bits), the
        // blocks of s_{i+1} into `wb` (2 D bits); the first row of the order ends up in the highest of those bits.
        constexpr int NA = 2 + 2 * D, NB = 2 * D;
        static_assert(NA <= 32 && NB <= 32, "one word per half of the rows");
        unsigned wa = 0u, wb = 0u;
        const double s45 = __builtin_fma(S.two_delta, pu, px);
        wa = cert_push_sign(wa, (S.n0 - s45) + tol_p);
        // Row 5 (x + 2 delta u <= K_hi[i+1]) is flagged only when it is CLEARLY VIOLATED.  Where K_hi rides the maximum-velocity
        // curve it passes close by the warm vertex at stage after stage (residual -1e-7 .. -1e-6: a third of the upper-bound
        // LPs the certificates refused in round 4 were exactly this), and nothing is lost by letting it through here: a kept
        // pair's certificate evaluates the reference's own test of row 5 on the reference's own vertex (cert_pair_rows, band5:
        // a residual in (1e-10, tol) is refused there), and a slide visits row 5 before any record, where its verdict must
        // be clear (cert_slide_visit).
        wa = cert_push_sign(wa, (s45 - S.n1) - tol_p);
        // (the tolerance goes into the rows' constants once per joint: one addition per row instead of two)
        double cpt[D], cnt[D];
#pragma unroll
        for (int k = 0; k < D; ++k) { cpt[k] = S.cpos[k] + tol_p; cnt[k] = S.cneg[k] + tol_p; }
        {
            double s[D];
#pragma unroll
            for (int k = 0; k < D; ++k) s[k] = __builtin_fma(S.rc1[k], pu, S.rc2[k] * px);
#pragma unroll
            for (int k = 0; k < D; ++k) wa = cert_push_sign(wa, s[k] + cpt[k]);
#pragma unroll
            for (int k = 0; k < D; ++k) wa = cert_push_sign(wa, cnt[k] - s[k]);
        }
        {
            double s[D];
#pragma unroll
            for (int k = 0; k < D; ++k) s[k] = __builtin_fma(S.rn1[k] + S.two_delta * S.rn2[k], pu, S.rn2[k] * px);
#pragma unroll
            for (int k = 0; k < D; ++k) wb = cert_push_sign(wb, s[k] + cpt[k]);
#pragma unroll
            for (int k = 0; k < D; ++k) wb = cert_push_sign(wb, cnt[k] - s[k]);
        }
        // rows that do NOT clearly hold, without the two rows already visited.  A row's place in the order is the reference's
        // row id j (CertStage::id_of): bit NA - 1 - j of the first word, bit NA + NB - 1 - j of the second.
        unsigned na = ~wa & (unsigned)((1ull << NA) - 1ull), nb = ~wb & (unsigned)((1ull << NB) - 1ull);
        auto drop = [&](int vi) {
            const int j = C::id_of(vi);  // (vi >= 4: f0, f1 are structural rows)
            const bool first = j < NA;
            na &= ~(first ? 1u << ((NA - 1 - j) & 31) : 0u);
            nb &= ~(first ? 0u : 1u << ((NA + NB - 1 - j) & 31));
        };
        drop(f0); drop(f1);
        // (masks instead of ?: -- the compiler lays a select between a computed row number and -1 out as a divergent branch)
        const int in_a = -(int)(na != 0u), any = -(int)((na | nb) != 0u);
        const int j1 = ((NA - 32 + cert_clz(na)) & in_a) | ((NA + NB - 32 + cert_clz(nb)) & ~in_a);
        const int m1 = j1 - 2, blk1 = (m1 * (65536 / D + 1)) >> 16;  // m1 / D for 0 <= m1 < 4 D <= 64 (exact: checked below)
        static_assert(D <= 16, "the multiply-shift division above");
        const int acc1 = C::ST + C::ST * blk1 + (m1 - blk1 * D);
        const int is_x = -(int)(j1 < 2);
        r1 = ((((j1 + 4) & is_x) | (acc1 & ~is_x)) & any) | ~any;
        // (the bits are only what they say for finite residuals: a start point that is not finite is refused)
        ok &= fabs(pu) + fabs(px) < 1e300;
    }
    TPR_SCHED_FENCE();
    const bool moved = MODE != 0 || r1 >= 0;  // (MODE 1, 2: the slide itself finds out whether a row is violated)

    // the row that limits r1's pivot: A or B, whichever forms a dual feasible vertex with r1 (exactly one must)
    double Aa, Ab, Ac, Ba, Bb, Bc, ra, rb, rc;
    // (A is one of the two rows fetched for the prologue: the second one when it pivoted, else the first)
    Aa = A == f1 ? a1 : a0; Ab = A == f1 ? b1 : b0; Ac = A == f1 ? c1 : c0;
    Ba = Brow[0]; Bb = Brow[1]; Bc = Brow[2];  // (handed out by the pivot that named B: no fetch)
    S.fetch(moved && r1 >= 0 ? r1 : 4, ra, rb, rc);
    if (MODE == 0) r1_viol = __builtin_fma(ra, pu, __builtin_fma(rb, px, rc)) > tol_p;
    ok &= !moved | (MODE != 0) | r1_viol;
    TPR_WHY(6, !moved | (MODE != 0) | r1_viol);
    auto dual = [&](double ca, double cb) {  // v = lr n_r + lc n_c with lr, lc > 0 (signs only)
        const double Dc = ra * cb - ca * rb;
        return (fabs(Dc) > kCertMinCross) & ((v0 * cb - v1 * ca) * Dc > 0) & ((ra * v1 - rb * v0) * Dc > 0);
    };
    const bool dA = MODE == 2 || (MODE == 0 && dual(Aa, Ab)), dB = MODE == 1 || (MODE == 0 && dual(Ba, Bb));
    ok &= !moved | (dA != dB);
    TPR_WHY(dA ? 7 : 8, !moved | (dA != dB));
    ok &= (MODE != 1) | (B == (v1 > kTiny ? 3 : 2));  // MODE 1: the limiter is the x wall the objective runs into
    const bool useA = dA;
    const int L = useA ? A : B, R0 = useA ? B : A;
    const double La = useA ? Aa : Ba, Lb = useA ? Ab : Bb, Lc = useA ? Ac : Bc;
    const double Ra = useA ? Ba : Aa, Rb = useA ? Bb : Ab;
    int rec;
    RowMask skip;
    skip.set(f0); skip.set(f1);  // (L and R0 are among them, or box rows, which a slide does not visit)
    TPR_SCHED_FENCE();
    const bool slide_ok = cert_slide<D, BS, MODE == 2, SB>(S, v0, v1, L < 4, La, Lb, Ra, Rb, pu, px, skip, tol_p, rec);
    TPR_SCHED_FENCE();
    ok &= !moved | (slide_ok & ((MODE != 0) | (rec >= 0)));
    TPR_WHY(9, !moved | (slide_ok & ((MODE != 0) | (rec >= 0))));
    // the final pair: (last record, L) after a slide, the prologue's vertex otherwise
    const bool slid = moved & (rec >= 0);
    p2 = slid ? rec : A;
    q2 = slid ? L : B;
    double fa, fb, fc;
    S.fetch(p2, fa, fb, fc);
    prow[0] = fa; prow[1] = fb; prow[2] = fc;
    qrow[0] = slid ? La : Ba; qrow[1] = slid ? Lb : Bb; qrow[2] = slid ? Lc : Bc;
    ok2 = ok & (p2 != q2) & !((p2 < 4) & (q2 < 4));
}

// Lower-bound LP of a backward stage (max 1e-9 u - x; UMAX = false: compute_feasible_sets' min-x LP, max -1e-9 u - x), sound.
// The reference's run (cold order: the warm pair of these LPs ends on the box row -3, which is not a valid warm start;
// a valid one -- two structural rows: K_lo above the box -- is left to the batches): from the corner (+-1e8, low1) the
// x_next row that the corner violates (row 1 / vi 5; mirrored: row 0 / vi 4) pivots against the box and lands on the wall
// x = low1, the other x_next row holds there, and every later pivot is a prefix record of where the rows cut that wall
// (cert_slide_wall); the last record is the binding row, which cert_lower_finish certifies as before.
template <int D, int BS, bool UMAX = true, bool SB = false>
__device__ __forceinline__ bool cert_lower_sound(const CertStage<D, BS> &S, bool norms_ok, double nmax, int up0, int up1, Lp2dOut &o) {
    const double sg_u = UMAX ? -1.0 : 1.0;  // (the objective's tilt in u, -+1e-9, enters through the wall slide's row score)
    const double low1 = S.low1, d2 = S.two_delta;
    const bool cold = !((up0 >= 4) & (up1 >= 4) & (up0 != up1));
    const double cbig = fmax(S.cmax, fmax(fabs(S.n0), fabs(S.n1)));
    // corner (UMAX: u = +1e8; mirrored: -1e8): the x_next row on the far side holds, the near one is violated, both clearly
    const double far_res = -d2 * kVarMax + (UMAX ? S.n0 - low1 : low1 - S.n1);   // row 4 at (+1e8, low1) / row 5 at (-1e8, low1)
    const double near_res = d2 * kVarMax + (UMAX ? low1 - S.n1 : S.n0 - low1);   // row 5 at (+1e8, low1) / row 4 at (-1e8, low1)
    const double tol_c = kCertSlack + kTraceRelSlack * (nmax * (kVarMax + fabs(low1)) + cbig);
    bool ok = cold & (far_res < -tol_c) & (near_res > tol_c);
    // its pivot: the line x = n -+ 2 delta u meets the wall x = low1 at u0, inside the u range; the 1-D objective on it is
    // clearly signed (|v1d| = 2 delta + 1e-9), the box is a box, and the other x_next row holds at the wall point
    ok &= (d2 > 1e-6) & (S.high1 - low1 > 1e-6 * (1.0 + fabs(S.high1) + fabs(low1)));
    const double u0 = (UMAX ? S.n1 - low1 : S.n0 - low1) * rcp_approx(d2);
    ok &= fabs(u0) < kVarMax * (1.0 - 1e-6);
    const double tol = kCertSlack + kTraceRelSlack * (nmax * (fabs(u0) + fabs(low1)) + cbig);
    ok &= S.n0 - S.n1 < -tol;  // the other x_next row at (u0, low1): residual n0 - n1
    int rec;
    TPR_SCHED_FENCE();
    const bool slide_ok = cert_slide_wall<D, BS, SB>(S, sg_u, u0, low1, tol, rec);
    TPR_SCHED_FENCE();
    ok &= slide_ok;
    // no record: the x_next row itself binds
    const int r_vi = rec >= 0 ? rec : (UMAX ? 5 : 4);
    double ra, rb, rc;
    S.fetch(r_vi, ra, rb, rc);
    const double u1 = -(rb * low1 + rc) * rcp_approx(ra);
    const double rrow[3] = {ra, rb, rc};
    return cert_lower_finish<D, BS, UMAX, true>(S, norms_ok & ok, nmax, r_vi, u1, o, rrow);
}

// One backward LP of an equality stage (cert_equality's cases), sound: the slide along the equality line names the row that
// binds, the limiter among the two x_next rows follows from the sign of the 1-D objective on that row's line.
template <int D, int BS>
__device__ __forceinline__ void cert_equality_sound_one(const CertStage<D, BS> &S, bool norms_ok, double nmax, double v0, double v1,
                                                        int w0, int w1, Lp2dOut &o) {
    const double d2 = S.two_delta;
    int p, q;
    bool ok;
    double prow[3], qrow[3];
    cert_propose_sound<D, BS, 2>(S, v0, v1, 4, 4, false, nmax, p, q, ok, prow, qrow);
    // p: the last record (a structural row: E1) or the x_next row that pivoted at the corner with q = its box limiter (no
    // later row violated: E2).  E1: the limiter is the x_next row whose bound class the 1-D objective on p's line picks
    const bool e1 = (p >= 8) & (q >= 4);
    const double alpha = prow[0] - d2 * prow[1], v1d = -prow[1] * v0 + prow[0] * v1;
    const int lim = ((v1d < 0) == (alpha < 0)) ? 5 : 4;
    const int pp = e1 ? p : q, qq = e1 ? lim : p;   // E2: (box row, the x_next row) as cert_pair<EQ> expects them
    const bool cold = !((w0 >= 4) & (w1 >= 4) & (w0 != w1));
    cert_pair<D, BS, true>(S, v0, v1, pp, qq, ok & cold & (e1 | ((p == 4) | (p == 5))), w0, w1, norms_ok, nmax, o);
}

// Both backward LPs of an equality stage.
template <int D, int BS>
__device__ __forceinline__ void cert_equality_sound(const CertStage<D, BS> &S, bool norms_ok, double nmax, int dn0, int dn1,
                                                    int up0, int up1, Lp2dOut &ou, Lp2dOut &ol) {
    cert_equality_sound_one<D, BS>(S, norms_ok, nmax, -1e-9, 1.0, dn0, dn1, ou);
    cert_equality_sound_one<D, BS>(S, norms_ok, nmax, 1e-9, -1.0, up0, up1, ol);
}

}  // namespace tpr

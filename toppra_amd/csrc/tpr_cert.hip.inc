// tpr_cert.hip.inc -- kernel family 3: one trajectory per lane, stage LPs answered from certificates.
//
// Once the two backward LPs of a stage are answered from a verified optimal vertex (see
// predict_upper_lp / predict_lower_lp in tpr_group.hip.inc for the argument) most stages need no
// search at all: the previous stage's active pair is still the optimal vertex (~92% of the
// upper-bound LPs, ~99.5% of the lower-bound LPs).  Checking that is a couple of straight scans
// over the rows plus a handful of scalar formulas -- regular work that wants the opposite layout of
// family 2: a lane owns a whole trajectory, the scans are fully unrolled over the rows (regenerated
// from q', q'' of the stage's two gridpoints, the +- twin rows sharing their products), nothing
// crosses lanes, and the per-trajectory scalar work that family 2 replicates 8x is done once.
//
// The LPs whose warm vertex does not verify (the active set moved, ties, degenerate or badly
// scaled stages: a few lanes of every wave at every stage) are handed to family 2's machinery:
// up to 8 of them at a time are dealt onto the wave's eight 8-lane groups (rows rebuilt from the
// owning lane's LDS columns), where the certified simplex walk and, failing that, the reference's
// full Seidel iteration run exactly as in tpr_group.hip.inc.  Results are bit-identical to the
// reference in every case.  TPR_STRICT_SEIDEL is served by family 2 only.
//
// Reference map: as tpr_group.hip.inc.

#pragma once
namespace tpr {

// A cross-lane hand-off through LDS inside ONE wave: the lanes run in lockstep and the LDS queue is in order, so all the
// hardware needs is that the compiler keeps the stores before and the loads after this point.  wave_barrier() alone is a
// scheduling barrier WITHOUT memory semantics; the wavefront-scope fences state the ordering in the memory model as well
// (no instruction at this scope -- they only pin the order of the LDS accesses around the hand-off).
#define TPR_WAVE_SYNC()                                              \
    do {                                                             \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       \
        __builtin_amdgcn_wave_barrier();                             \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");       \
    } while (0)

}  // namespace tpr
#include "tpr_cert_lane.hip.inc"
namespace tpr {

// From which dof on the certified lane kernels re-read the velocity limits / the spline segment's coefficients from global
// memory instead of holding them in registers (cert_solve_kernel; measured per dof, DESIGN.md section 3.2).
// (TPR_LEAN_COEF_FROM: tpr_group.hip.inc, beside cert_tws_fields, which sizes the workspace by it.)
#ifndef TPR_LEAN_VEL_FROM
#define TPR_LEAN_VEL_FROM 10
#endif

// The LPs the lane-level certificates could not answer, handed to family 2's code: up to 8 of them
// at a time, one per 8-lane group of the wave, rows rebuilt across the group's lanes from the owning
// lane's LDS columns.  Each group runs the certified simplex walk (predict_upper_lp) and, when that
// does not verify either, the reference's full iteration (group_lp2d).  Upper-bound (need_u) and
// lower-bound (need_l) LPs of a stage share the batches.
//   xch: LDS [kCertXch - 1][BS]: fields 0-2 = what every lane publishes for its stage (two_delta, packed warm pairs of the two
//        LPs), 3-5 / 6-8 = results for the owning lane (u, x, packed ok/ac0/ac1) of its upper / lower LP; n0, n1, low1, high1
//        come from the lane's column of row constants (limtab rows 2..5: round 6, 2 KB of LDS per block less)
//   queue: LDS, 2 BS ints: the waiting LPs (an array of its own type: up to round 5 it was an int view of a 14th double field --
//        a strict-aliasing violation in the letter, although no location was ever accessed under both types)
//   rowbufs: LDS, cert_batch_groups<D>() x GroupCfg<D, kCertBatchLanes>::kRowBuf.   need_* are per lane; control flow is wave-uniform.
// MODE 0: the two LPs of a backward stage (objectives (-1e-9, 1) and (1e-9, -1)).  MODE 1: those of compute_feasible_sets
// (reachability_algorithm.py:149-157: (1e-9, 1) and (-1e-9, -1)).  MODE 2: the same at the LAST gridpoint, where the x_next
// pair is the disabled row (cy_seidel_solverwrapper.pyx:622-626) and the interpolation block repeats the stage's own rows
// (linear_constraint.py:172,177; the caller publishes two_delta = 0); nothing certifies there (duplicate rows), so every LP
// skips the walk.
// alim_blk (slim blocks, CertStage::kSlim): the block's transposed workspace (GroupArgs::tws: acceleration limits [2 D][BS]) --
// the c of another lane's rows is read from there (the lanes' own copies live in registers only); nullptr otherwise.
template <int D, int BS, bool INTERP = true, int MODE = 0, bool SOUNDB = false>
__device__ inline void cert_needy_batch(const CertStage<D, BS> &S, const double *qtab, int pc, const double *limtab,
                                        const double *alim_blk, int ntraj_blk,
                                        double *xch, int *queue, double *rowbufs, bool need_u, bool need_l, int dn0, int dn1,
                                        int up0, int up1, Lp2dOut &out_u, Lp2dOut &out_l) {
    constexpr bool sound = SOUNDB;  // (a template parameter: the sound kernels carry no simplex-walk code at all)
    static_assert(BS == 64, "one wave per block");
    constexpr int L = kCertBatchLanes;
    using G = GroupCfg<D, L>;
    const int lane = threadIdx.x & (BS - 1), gl = lane % L, g = lane / L;  // (the two-wave kernel calls this from its second wave)
    // exchange fields per lane: 0 two_delta, 1 / 2 the warm pairs, 3..5 / 6..8 the answers (u, x, packed status) of the upper / lower
    // LP.  The stage's n0, n1, low1, high1 are NOT copied here: they sit in the lane's column of row constants (`limtab`, rows 2..5:
    // low1, -high1, n0, -n1 -- CertStage::publish_special, called by every caller before this) and are read from there, negations
    // undone exactly -- four fields = 2 KB of LDS per block less, which is what lets the 15-dof slim block fit four to a CU.
    xch[0 * BS + lane] = S.two_delta;
    using CS = CertStage<D, BS>;  // family 2's code works with the reference's row ids
    xch[1 * BS + lane] = __hiloint2double(CS::id_of(dn0), CS::id_of(dn1));
    xch[2 * BS + lane] = __hiloint2double(CS::id_of(up0), CS::id_of(up1));
    TPR_WAVE_SYNC();
    // queue of waiting LPs (upper-bound LPs first): every needy lane enters itself at its rank
    const unsigned long long mask_u = __builtin_amdgcn_ballot_w64(need_u), mask_l = __builtin_amdgcn_ballot_w64(need_l);
    const int n_u = __builtin_popcountll(mask_u), n_all = n_u + __builtin_popcountll(mask_l);
    const int below_u = __builtin_amdgcn_mbcnt_hi((unsigned)(mask_u >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask_u, 0));
    const int below_l = __builtin_amdgcn_mbcnt_hi((unsigned)(mask_l >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask_l, 0));
    // (sound mode: the walk is ONE dual pivot at most and certified 1 of 10 000 of the LPs that reached it -- they go
    // straight to the iteration)
    if (need_u) queue[below_u] = lane | ((MODE == 2 || sound || out_u.hint_full) ? 512 : 0);
    if (need_l) queue[n_u + below_l] = lane | 256 | ((MODE == 2 || sound) ? 512 : 0);
    TPR_WAVE_SYNC();
    constexpr int kGroups = cert_batch_groups<D>();
    const bool working = g < kGroups;  // the other groups idle (and own no row mirror)
    double *rowbuf_w = rowbufs + (working ? g : 0) * G::kRowBuf;
    for (int base = 0; base < n_all; base += kGroups) {
        // group g takes queue entry base + g
        const bool have = working && base + g < n_all;
        const int e = queue[have ? base + g : 0];
        const int src = have ? (e & 255) : -1;
        const bool lower = have & ((e & 256) != 0);
        const bool skip_walk = have & ((e & 512) != 0);
        const bool act = src >= 0;
        const int sl = act ? src : 0;
        const double two_delta = xch[0 * BS + sl], n0 = limtab[4 * BS + sl], n1 = -limtab[5 * BS + sl],
                     low1 = limtab[2 * BS + sl], high1 = -limtab[3 * BS + sl], wpk = xch[(lower ? 2 : 1) * BS + sl];
        const int w0 = act ? __double2hiint(wpk) : 0, w1 = act ? __double2loint(wpk) : 0;
        const double v0 = (lower != (MODE != 0)) ? 1e-9 : -1e-9, v1 = lower ? -1.0 : 1.0;
        Slots<D, L> R;
#pragma unroll
        for (int s = 0; s < G::S; ++s) {
            const int vi = s * L + gl;
            // Collocation (!INTERP): the two interpolation blocks hold the disabled row, as in family 2 (GroupTraj::nblk)
            const bool acc = vi >= 6 && vi < (INTERP ? G::nV : 6 + 2 * D);
            const int m = acc ? vi - 6 : 0;
            const int blk = m / D, k = m - blk * D;
            const bool neg = blk & 1, nx = blk >> 1;
            const int par = (nx && MODE != 2) ? (pc ^ 1) : pc;
            const double q1 = qtab[((par * 2 + 0) * D + k) * BS + sl], q2 = qtab[((par * 2 + 1) * D + k) * BS + sl];
            const double av = nx ? q1 + two_delta * q2 : q1;
            double cc;
            if (!CertStage<D, BS>::kSlim) {
                cc = limtab[(6 + (neg ? D : 0) + k) * BS + sl];
            } else {  // (idle lanes shadow the block's last trajectory)
                (void)ntraj_blk;  // (the block's transposed workspace holds a column for every lane, shadows included)
                cc = neg ? alim_blk[(2 * k) * BS + sl] : -alim_blk[(2 * k + 1) * BS + sl];
            }
            // idle group / slots beyond the last row: a disabled row (0, 0, -1); rows 0..5 by a select chain
            // over small tables (a nested if / ?: on the row index would be lowered to divergent branches)
            double a = 0, b = 0, c = -1;
            if (s == 0) {
                const double ta[6] = {-1.0, 1.0, 0.0, 0.0, MODE == 2 ? 0.0 : -two_delta, MODE == 2 ? 0.0 : two_delta};
                const double tb[6] = {0.0, 0.0, -1.0, 1.0, MODE == 2 ? 0.0 : -1.0, MODE == 2 ? 0.0 : 1.0};
                const double tc[6] = {kVarMin, -kVarMax, low1, -high1, MODE == 2 ? -1.0 : n0, MODE == 2 ? -1.0 : -n1};
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const bool hit = vi == j;
                    a = hit ? ta[j] : a;
                    b = hit ? tb[j] : b;
                    c = hit ? tc[j] : c;
                }
            }
            a = acc ? (neg ? -av : av) : a;
            b = acc ? (neg ? -q2 : q2) : b;
            c = acc ? cc : c;
            a = act ? a : 0.0;
            b = act ? b : 0.0;
            c = act ? c : -1.0;
            R.a[s] = a; R.b[s] = b; R.c[s] = c;
            if (working && vi < G::nV) { rowbuf_w[vi] = a; rowbuf_w[G::nV + vi] = b; rowbuf_w[2 * G::nV + vi] = c; }
        }
        TPR_WAVE_SYNC();
        GroupLp r;
        const double bl1 = act ? low1 : 0.0, bh1 = act ? high1 : 1.0;
        bool got = false;
        if constexpr (!(SOUNDB || MODE == 2)) {
            if (__builtin_amdgcn_ballot_w64(act & !skip_walk) != 0)  // (wave-uniform; a skipped group idles through the others' walk)
                got = predict_upper_lp<D, L>(R, rowbuf_w, gl, v0, v1, bl1, bh1, w0, w1, r, sound);
        }
        if (!got) r = group_lp2d<D, L>(R, rowbuf_w, gl, v0, v1, kVarMin, kVarMax, bl1, bh1, w0, w1);
        if (act && gl == 0) {
            const int f = lower ? 6 : 3;
            xch[f * BS + sl] = r.u; xch[(f + 1) * BS + sl] = r.x;
            xch[(f + 2) * BS + sl] = __hiloint2double((r.ok ? 1 : 0) | (got ? 0 : 2), (r.ac0 & 0xffff) | (r.ac1 << 16));
        }
        TPR_WAVE_SYNC();
    }
    auto take = [&](int f, Lp2dOut &out) {  // bit 1 of the packed word: the LP went through the full iteration
        const double pk = xch[(f + 2) * BS + lane];
        const int lo = __double2loint(pk);
        out.ok = (__double2hiint(pk) & 1) != 0;
        out.u = xch[f * BS + lane];
        out.x = xch[(f + 1) * BS + lane];
        out.ac0 = CS::vi_of((int)(short)(lo & 0xffff));
        out.ac1 = CS::vi_of(lo >> 16);
    };
    if (need_u) take(3, out_u);
    if (need_l) take(6, out_l);
}

// Output staging.  A lane produces W doubles per stage for its own trajectory; written directly that
// is one 8- or 16-byte store per lane and stage, scattered over 64 rows, which the memory system
// turns into 32-byte requests (4x the bytes on the HBM side, measured).  Instead the values of 8
// consecutive stages are collected in registers and written out transposed through LDS: 8 adjacent
// lanes store one trajectory's 8 stages, i.e. 64 (W = 1) or 128 (W = 2) contiguous bytes.
template <int BS, int W>
struct StagedOut {
    double buf[8][W];
    __device__ __forceinline__ void put(int j, const double (&v)[W]) {
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int w = 0; w < W; ++w) buf[s][w] = s == j ? v[w] : buf[s][w];
    }
    // stages [base, base + cnt), cnt <= 8, base + s held in buf[(base + s) & 7]; st: LDS, 8 W BS doubles;
    // g0: the array row of the block's first trajectory; ntraj: trajectories of this block
    __device__ __forceinline__ void flush(double *st, double *g0, size_t row_stride, int base, int cnt, int ntraj) {
        const int lane = threadIdx.x;
        TPR_WAVE_SYNC();
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int w = 0; w < W; ++w) st[(s * W + w) * BS + lane] = buf[s][w];
        TPR_WAVE_SYNC();
        const int p = lane % 8;
#pragma unroll
        for (int k = 0; k < BS / 8; ++k) {
            const int t = 8 * k + lane / 8;
            if (p < cnt && t < ntraj) {
                const int slot = (base + p) & 7;
                double *dst = g0 + (size_t)t * row_stride + (size_t)(base + p) * W;
                if (W == 2) {
                    *reinterpret_cast<double2 *>(dst) = make_double2(st[(slot * 2) * BS + t], st[(slot * 2 + 1) * BS + t]);
                } else {
                    dst[0] = st[slot * BS + t];
                }
            }
        }
        TPR_WAVE_SYNC();
    }
};

// WANT_SD: also write sd = sqrt(sd2).  GRID_LDS: the grid is shared by the batch and staged in
// (dynamic) LDS, so that the per-stage gridpoint is a broadcast LDS read instead of a global load.
// sd2, u, K and status are required (launch_solve routes other requests to family 2), or
// GroupArgs::backward_only for compute_controllable_sets on its own.
// INTERP = false: Collocation -- the acceleration rows of s_{i+1} (blocks 2, 3) do not exist.  Their q', q'' are kept at
// 0 in registers, which makes them null rows (0, 0, c < 0) for every scan and guard of the certificates: never
// violated, never blocking, exactly parallel to everything; the row numbering of blocks 0, 1 is the reference's.
// SOUND: TPR_SOUND_CERTIFICATES as a compile-time constant -- the proposal is inlined, and what the sound mode counts per
// row (cert_propose2's `loose`) would otherwise ride along in the fast mode too (1.62 -> 1.68 ms when it was a runtime flag).
// SDFWD: TOPPRAsd (desired_duration_algorithm.py:42-142) -- after the backward scan the two forward scans of that
// algorithm ("fastest": objective [-2 delta, -1]; "slowest": [2 delta, 1], :219-226) run side by side instead of TOPPRA's
// own; A.sd_xf / sd_uf / sd_xl / sd_ul receive the profiles, A.status the controllability verdict.
template <int D, int BS, bool WANT_SD, bool GRID_LDS, bool INTERP = true, bool SOUND = false, bool SDFWD = false>
__global__ void __launch_bounds__(BS) cert_solve_kernel(GroupArgs A) {
    using C = CertStage<D, BS>;
    // The slides' verdicts as sign bits (cert_slide_visit<..., SB>) or as a running minimum of doubles: the same verdicts, and per
    // dof a MEASURED choice -- the two forms differ in what the register allocator makes of the kernel (65536 x d x 200, sign bits /
    // running minimum: 3.17 / 2.82 ms at 9 dof, 3.75 / 3.17 at 10, 4.57 / 4.58 at 11, 5.79 / 6.80 at 12, 11.05 / 9.68 at 13;
    // profiles/r05_signbits_per_dof.log).  TPR_SIGNBITS_DOFS / TPR_SIGNBITS_SD_DOFS (TOPPRAsd instantiations) are bit masks over the
    // dofs that use the sign bits.  Round 5 took <5 dof, TOPPRAsd, sign bits> for a miscompile of the form itself; it is the
    // register allocator's copy above an exec restore (profiles/r06_miscompile_root_cause.md), which ANY spelling can trigger and
    // which the build now checks every unit for (toppra_amd/codegen_check.py): of the 13 TOPPRAsd instantiations with sign bits,
    // 5 and 13 dof show the pattern and therefore keep the running minimum.
#ifndef TPR_SIGNBITS_DOFS
#define TPR_SIGNBITS_DOFS 0x09feu  /* 1..8, 11 (round 6, with the transposed workspace: 12 dof 5.15 / 4.76 ms with / without) */
#endif
#ifndef TPR_SIGNBITS_SD_DOFS
#define TPR_SIGNBITS_SD_DOFS 0x01deu  /* 1..4, 6..8 */
#endif
    constexpr bool kSignBits = ((SDFWD ? TPR_SIGNBITS_SD_DOFS : TPR_SIGNBITS_DOFS) >> D) & 1u;
    // q', q'' columns (two gridpoint parities), then the row constants (c of rows 0..5 per stage, cpos / cneg
    // columns); the forward scan, which fetches no rows by index, reuses the front as its output staging
    constexpr int kStageDoubles = (SDFWD ? 32 : 24) * BS;  // forward output staging: 3 (TOPPRAsd: 4) arrays x 8 stages
    constexpr int kColDoubles = (4 * D + C::kLimCols) * BS > kStageDoubles ? (4 * D + C::kLimCols) * BS : kStageDoubles;
    constexpr int kRing = C::kRing;
    __shared__ double cols[kColDoubles];
    double *qt = cols, *lim = cols + 4 * D * BS;
    __shared__ double scratch[(kCertXch - 1) * BS + cert_batch_groups<D>() * GroupCfg<D, kCertBatchLanes>::kRowBuf];  // batch exchange + row mirrors
    __shared__ int needy_queue[2 * BS];                   // the waiting LPs of a cooperative batch (cert_needy_batch)
    constexpr bool kDirectK = C::kDirectK;
    __shared__ double kst[kDirectK ? 1 : kRing * 2 * BS]; // controllable sets of the last kRing backward stages, written out transposed
    double *xch = scratch, *rowbufs = scratch + (kCertXch - 1) * BS;
    extern __shared__ double grid_lds[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x * BS + tid;
    const bool alive = b < A.B;
    // idle lanes shadow the last trajectory (computing, never storing)
    const int bb = alive ? b : A.B - 1;
    const int N = A.N, nseg = A.nseg;
    const double *gcf = A.coef + (size_t)bb * 4 * nseg * D;
    const double *brk = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? (size_t)bb * (nseg + 1) : 0);
    const double *ggrid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)bb * (N + 1) : 0);
    if (GRID_LDS) {
        for (int e = tid; e <= N; e += BS) grid_lds[e] = A.grid[e];
        __syncthreads();
    }
    auto grid = [&](int i) -> double { return GRID_LDS ? grid_lds[i] : ggrid[i]; };
    const bool has_vel = A.flags & TPR_HAS_VELOCITY;

    // Slim blocks (above 8 dof) re-read limits and, from TPR_LEAN_COEF_FROM dof on, the spline coefficients at every stage.  From the
    // caller's trajectory-major arrays that is one cache line per lane and load (round 5, 12 dof: 9.8 GB fetched per launch for
    // 0.55 GB of algorithmic traffic, half the kernel's time waiting); each block therefore transposes its 64 trajectories' values
    // ONCE into its slice of GroupArgs::tws as [field][lane], and a wave's re-read is 512 contiguous bytes.  A lane only ever
    // re-reads its own column, except in the cooperative batches, which run behind wave-level hand-offs (TPR_WAVE_SYNC).
    const double *tw = nullptr, *tw_blk = nullptr;  // this lane's column / the block's slice
    const double *cbase = gcf;                      // c0, c1, c2 of this trajectory: [3][nseg][D] at stride cstride
    int cstride = 1;
    if constexpr (C::kSlim) {
        const size_t fields = cert_tws_fields(D, nseg);
        double *wb = A.tws + (size_t)blockIdx.x * fields * BS, *w = wb + tid;
        const double *al = A.alim + (size_t)bb * 2 * D;
#pragma unroll
        for (int j = 0; j < 2 * D; ++j) w[j * BS] = al[j];
        const double *vl = has_vel ? A.vlim + (size_t)bb * 2 * D : nullptr;
#pragma unroll
        for (int j = 0; j < 2 * D; ++j) w[(2 * D + j) * BS] = has_vel ? vl[j] : 0.0;
        if constexpr (D >= TPR_LEAN_COEF_FROM) {  // (below, the coefficients live in registers: nothing would read a copy)
            if (nseg <= kTwsMaxSeg) {
                for (int e = 0; e < 3 * nseg * D; ++e) w[(size_t)(4 * D + e) * BS] = gcf[e];
                cbase = w + (size_t)4 * D * BS;
                cstride = BS;
            }
        }
        tw = w; tw_blk = wb;
        TPR_WAVE_SYNC();  // (the cooperative batches read other lanes' columns)
    }
    C S;
    if constexpr (C::kPairFetch) {  // rows 0..5 as (q1, q2) pairs for CertStage::fetch: (1, 0), (+0, 1), (-0, 1)
        __shared__ double spec_rows[C::kSpecDoubles];
        if (tid < C::kSpecDoubles) spec_rows[tid] = (tid == 0 || (tid & 1)) ? (tid == 1 ? 0.0 : 1.0) : (tid == 4 ? -0.0 : 0.0);
        S.spec = spec_rows;
        TPR_WAVE_SYNC();
    }
    double vlo[D], vhi[D];
    {
        const double *alim = A.alim + (size_t)bb * 2 * D;
#pragma unroll
        for (int k = 0; k < D; ++k) { S.cpos[k] = -alim[2 * k + 1]; S.cneg[k] = alim[2 * k]; }
        S.lim = lim + tid;
        S.alim_lane = C::kSlim ? tw : alim;
        lim[0 * BS + tid] = kVarMin; lim[1 * BS + tid] = -kVarMax;
        S.cmax = 0.0;
        S.min_range = 3.0e300;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (!C::kSlim) {
                lim[(6 + k) * BS + tid] = S.cpos[k];
                lim[(6 + D + k) * BS + tid] = S.cneg[k];
            }
            S.cmax = fmax(S.cmax, fmax(fabs(S.cpos[k]), fabs(S.cneg[k])));
            S.min_range = fmin(S.min_range, -S.cpos[k] - S.cneg[k]);
        }
        const double *vlim = has_vel ? A.vlim + (size_t)bb * 2 * D : nullptr;
#pragma unroll
        for (int k = 0; k < D; ++k) { vlo[k] = has_vel ? vlim[2 * k] : 0.0; vhi[k] = has_vel ? vlim[2 * k + 1] : 0.0; }
    }
    // From 10 dof on the velocity limits, from 11 dof on the spline segment's coefficients too, are re-read from global memory
    // where they are used (once per stage, L2-hot) instead of living in 4 D + 6 D registers: the trace-following certificates
    // need those registers -- 0.2 - 0.7 KB of scratch per lane at 10..13 dof otherwise (65536 x d x 200: 4.6 / 7.8 / 7.7 /
    // 10.9 ms at 10..13 dof with everything in registers, 3.8 / 5.0 / 6.1 / 9.2 ms like this;
    // profiles/r04_family3_lean_rereads.log.  At 7 dof, where nothing spills, the re-read costs 15 %: DESIGN 4.1.)
    constexpr bool kLean = D >= TPR_LEAN_VEL_FROM, kLeanCoef = D >= TPR_LEAN_COEF_FROM;
    static_assert(!(kLean || kLeanCoef) || C::kSlim, "the lean re-reads go to the slim blocks' transposed workspace");
    auto vsel = [&](int k, bool upper) -> double {  // one load whichever side is asked for (a select between two loads gets sunk)
        if constexpr (kLean) return tw[(2 * D + 2 * k + (upper ? 1 : 0)) * BS];
        else return upper ? vhi[k] : vlo[k];
    };
    // A velocity range that excludes 0 (vlim_lo > 0 or vlim_hi < 0) gives a positive lower bound on sd; no lane of
    // the wave having one is the normal case, and the per-stage test for it is skipped then (wave-uniform).
    bool one_sided = false;
#pragma unroll
    for (int k = 0; k < D; ++k) one_sided |= (vlo[k] > 0) | (vhi[k] < 0);
    const bool any_one_sided = __builtin_amdgcn_ballot_w64(one_sided) != 0;
    // (scaled) cubic coefficients of the current spline segment [seg_lo, seg_hi), reloaded when the gridpoint
    // leaves it (find_segment's result for increasing breakpoints, without its loads per stage)
    double c0[D], c1[D], c2[D];
    int jcur = -1;
    double seg_lo = 1.0, seg_hi = 0.0, seg_b = 0.0;
    double *col = qt + tid;
    // q', q'' at s into (o1, o2) and LDS parity slot par; optionally the x box from the velocity limits
    // par < 0: registers only (the forward scan fetches no rows by index, and reuses the q columns as output staging)
    auto eval = [&](double s, int par, bool want_box, double (&o1)[D], double (&o2)[D], double &low1, double &high1) {
        if (!(s >= seg_lo && s < seg_hi)) {
            const int j = find_segment(brk, nseg, s);
            if (j != jcur) {
                if constexpr (!kLeanCoef) {
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        c0[k] = gcf[(0 * nseg + j) * D + k] * 3.0;  // the derivative's coefficients (cubic_d1_d2_scaled)
                        c1[k] = gcf[(1 * nseg + j) * D + k] * 2.0;
                        c2[k] = gcf[(2 * nseg + j) * D + k];
                    }
                }
                jcur = j;
            }
            seg_b = brk[j];
            seg_lo = j == 0 ? -3.0e300 : seg_b;
            seg_hi = j == nseg - 1 ? 3.0e300 : brk[j + 1];
        }
        const double t = s - seg_b;
        double *d1 = col + ((par < 0 ? 0 : par) * 2 + 0) * D * BS, *d2 = col + ((par < 0 ? 0 : par) * 2 + 1) * D * BS;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            double q1, q2;
            if constexpr (kLeanCoef) {
                cubic_d1_d2_scaled(cbase[(size_t)(((0 * nseg + jcur) * D + k) * cstride)] * 3.0, cbase[(size_t)(((1 * nseg + jcur) * D + k) * cstride)] * 2.0,
                                   cbase[(size_t)(((2 * nseg + jcur) * D + k) * cstride)], t, q1, q2);
            } else {
                cubic_d1_d2_scaled(c0[k], c1[k], c2[k], t, q1, q2);
            }
            o1[k] = q1; o2[k] = q2;
            if (par >= 0) {
                d1[k * BS] = q1;
                d2[k * BS] = q2;
            }
        }
        low1 = kVarMin; high1 = kVarMax;
        if (want_box) {
            // _create_velocity_constraint: sdmax / sdmin are C floats updated dof by dof.  Rounding to
            // fp32 is monotone, so the running fp32 minimum equals the fp64 minimum rounded once (as in
            // family 2's reduction): the D quotients are independent instead of a serial chain.
            double mmax = (double)kJvelMaxSd;
            bool pos_lower = false;  // some dof gives a positive lower bound on sd (vlim_lo > 0 or vlim_hi < 0)
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double q1 = o1[k];
                const bool valid = (q1 != 0) & !isnan(q1);
                const double rmax = vsel(k, q1 > 0) / q1;
                mmax = (valid & (rmax <= mmax)) ? rmax : mmax;
            }
            if (any_one_sided) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double q1 = o1[k];
                    { const double vv = vsel(k, !(q1 > 0)); pos_lower |= (q1 > 0) ? vv > 0 : ((q1 < 0) & (vv < 0)); }
                }
            }
            const float sdmax = (float)mmax;
            // sdmin = max_k (vlim / q') is <= 0 unless pos_lower, and then the lower bound on x is 0
            // exactly (the reference's float64_max(sdmin, 0)**2): the quotients are only needed otherwise
            double xlo = 0.0;
            if (pos_lower) {
                float sdmin = -kJvelMaxSd;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double q1 = o1[k];
                    const double rmin = vsel(k, !(q1 > 0)) / q1;
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
    };
    auto bind = [&](int i) {  // stage i: cur = parity of i, nxt = parity of i+1
        const int pc = i & 1, pn = pc ^ 1;
        S.cur1 = col + (pc * 2 + 0) * D * BS; S.cur2 = col + (pc * 2 + 1) * D * BS;
        S.nxt1 = col + (pn * 2 + 0) * D * BS; S.nxt2 = col + (pn * 2 + 1) * D * BS;
    };

    const double *K = A.K + (size_t)bb * 2 * (N + 1);  // this lane's row, read back in the forward scan
    // outputs go through StagedOut: rows of the block's first trajectory, and how many rows there are
    const size_t b0 = (size_t)blockIdx.x * BS;
    const int ntraj = A.B - (int)b0 < BS ? A.B - (int)b0 : BS;
    const double *alim_blk = tw_blk;  // (cert_needy_batch: another lane's row constants, from the block's transposed workspace)
    double *K0 = A.K + b0 * 2 * (N + 1), *xs0 = A.sd2 + b0 * (N + 1), *us0 = A.u + b0 * N;
    double *sd0 = WANT_SD ? A.sd + b0 * (N + 1) : nullptr;
    double *xs = A.sd2 + (size_t)bb * (N + 1);
    double *sdv = WANT_SD ? A.sd + (size_t)bb * (N + 1) : nullptr;
    const double sd_start = A.sd_start ? A.sd_start[bb] : 0.0;
    const double sd_end = A.sd_end ? A.sd_end[bb] : 0.0;

    // ---- backward scan: controllable sets ------------------------------------------------
    int up0 = 4, up1 = 4, dn0 = 4, dn1 = 4;  // warm-start state (active_c_up / active_c_down = {0, 0}) in the internal row numbering
    double kn0 = boundary_x(A.flags, sd_end), kn1 = A.sd_end_hi ? boundary_x(A.flags, A.sd_end_hi[bb]) : kn0;
    // K rows go to LDS as they are produced (slot = stage & (kRing - 1)) and are written out every kRing stages,
    // transposed: kRing adjacent lanes store one trajectory's kRing stages = 64 (slim blocks: 32) contiguous bytes
    constexpr int kRingTraj = BS / kRing;  // trajectories per pass of a flush
    auto k_put = [&](int i, double lo_, double hi_) {
        if constexpr (kDirectK) {  // (this lane's own row: the forward scan reads it back from the same thread)
            if (alive) *reinterpret_cast<double2 *>(A.K + (size_t)bb * 2 * (size_t)(N + 1) + (size_t)i * 2) = make_double2(lo_, hi_);
        } else {
            kst[((i & (kRing - 1)) * 2 + 0) * BS + tid] = lo_;
            kst[((i & (kRing - 1)) * 2 + 1) * BS + tid] = hi_;
        }
    };
    auto k_flush = [&](int base, int cnt) {  // stages [base, base + cnt), cnt <= kRing, base % kRing == 0
        if constexpr (kDirectK) return;
        TPR_WAVE_SYNC();
        const int pst = tid & (kRing - 1), slot = (base + pst) & (kRing - 1);
        double2 v[kRing];  // LDS reads first, then the stores (see f_flush)
#pragma unroll
        for (int k = 0; k < kRing; ++k) v[k] = make_double2(kst[(slot * 2) * BS + kRingTraj * k + (tid / kRing)], kst[(slot * 2 + 1) * BS + kRingTraj * k + (tid / kRing)]);
        if (cnt == kRing && ntraj == BS) {  // wave-uniform: the full block
#pragma unroll
            for (int k = 0; k < kRing; ++k)
                *reinterpret_cast<double2 *>(K0 + (size_t)(kRingTraj * k + (tid / kRing)) * 2 * (size_t)(N + 1) + (size_t)(base + pst) * 2) = v[k];
        } else {
#pragma unroll
            for (int k = 0; k < kRing; ++k) {
                const int t = kRingTraj * k + (tid / kRing);
                if (pst < cnt && t < ntraj) *reinterpret_cast<double2 *>(K0 + (size_t)t * 2 * (size_t)(N + 1) + (size_t)(base + pst) * 2) = v[k];
            }
        }
        TPR_WAVE_SYNC();
    };
    k_put(N, kn0, kn1);
    if ((N & (kRing - 1)) == 0) k_flush(N, 1);
    bool failed = false;
    double s_n = grid(N);
    double dummy0, dummy1;
    eval(s_n, N & 1, false, S.rc1, S.rc2, dummy0, dummy1);
    double s_prefetch = grid(N - 1);
    for (int i = N - 1; i >= 0; --i) {
        const double s_i = s_prefetch;
        if (i > 0) s_prefetch = grid(i - 1);
        const double delta = s_n - s_i;
        double low1, high1;
#pragma unroll
        for (int k = 0; k < D; ++k) { S.rn1[k] = INTERP ? S.rc1[k] : 0.0; S.rn2[k] = INTERP ? S.rc2[k] : 0.0; }
        eval(s_i, i & 1, has_vel, S.rc1, S.rc2, low1, high1);
        double lo = 0, hi = 0;
        // `solve`: this lane has two LPs to answer at this stage.  The cooperative fallback below
        // needs the whole wave, so the stage body is wave-uniform and lanes are masked by flags.
        const bool solve = !failed && !(isnan(kn0) || isnan(kn1));
        bind(i);
        S.two_delta = 2 * delta; S.n0 = kn0; S.n1 = kn1; S.low1 = low1; S.high1 = high1;
        S.publish_special(lim + tid);
        double nmax;
        const bool nok = S.norms(nmax);
        // lane level: is the previous active pair still the verified optimum?  (straight-line code)
        Lp2dOut su, sl;
        int up_p, up_q;
        bool up_ok;
        double up_prow[3], up_qrow[3];
        // (cert_pair_rows' TRACE mode skips the role derivation and the violation bound: cert_propose_sound has established them)
        if constexpr (SOUND) cert_propose_sound<D, BS, 0, kSignBits>(S, -1e-9, 1.0, dn0, dn1, dn0 != dn1, nmax, up_p, up_q, up_ok, up_prow, up_qrow);
        else cert_propose2<D, BS>(S, -1e-9, 1.0, dn0, dn1, dn0 != dn1, false, nmax, up_p, up_q, up_ok, up_prow, up_qrow);
        bool need_u = solve & !cert_pair_rows<D, BS, false, SOUND>(S, -1e-9, 1.0, up_p, up_q, nok & up_ok, up_prow[0], up_prow[1], up_prow[2],
                                                            up_qrow[0], up_qrow[1], up_qrow[2], dn0, dn1, nmax, su);
        bool need_l;
        if constexpr (SOUND) need_l = solve & !cert_lower_sound<D, BS, true, kSignBits>(S, nok, nmax, up0, up1, sl);
        else need_l = solve & !cert_lower<D, BS>(S, nok, nmax, sl);
        // x_next rows forming an equality (the first stage: K[N] is a single point): neither check above
        // can succeed (both rows are active), a dedicated certificate answers both LPs
        if (__builtin_amdgcn_ballot_w64(solve & (kn0 == kn1)) != 0) {
            Lp2dOut eu, el;
            if constexpr (SOUND) cert_equality_sound<D, BS>(S, nok, nmax, dn0, dn1, up0, up1, eu, el);
            else cert_equality<D, BS>(S, nok, nmax, dn0, dn1, up0, up1, eu, el);
            const bool eq = solve & (kn0 == kn1);
            if (eq & need_u & eu.ok) { su = eu; need_u = false; }
            if (eq & need_l & el.ok) { sl = el; need_l = false; }
        }
        // the rest goes through family 2's walk / full iteration, 8 LPs at a time
        if (__builtin_amdgcn_ballot_w64(need_u | need_l) != 0) {
            cert_needy_batch<D, BS, INTERP, 0, SOUND>(S, qt, i & 1, lim, alim_blk, ntraj, xch, needy_queue, rowbufs, need_u, need_l, dn0, dn1, up0, up1, su, sl);
        }
        if (!solve) { su.ok = sl.ok = false; su.x = sl.x = qnan(); }
        if (su.ok) { dn0 = su.ac0; dn1 = su.ac1; } else su.x = qnan();
        if (sl.ok) { up0 = sl.ac0; up1 = sl.ac1; } else sl.x = qnan();
        if (!failed) {
            hi = su.x;  // NaN when the stage was not solvable (NaN K above it) or infeasible
            lo = sl.x;
            if (lo < 0) lo = 0;
            if (isnan(lo) || isnan(hi)) failed = true;
        }
        k_put(i, lo, hi);
        if ((i & (kRing - 1)) == 0) k_flush(i, N + 1 - i < kRing ? N + 1 - i : kRing);
        kn0 = lo; kn1 = hi;
        s_n = s_i;
    }

    const double x_start = boundary_x(A.flags, sd_start);
    // FailUncontrollable: the lane stays (the staged stores are cooperative) and writes NaN everywhere
    const bool dead = failed || x_start + kPySmall < kn0 || kn1 + kPySmall < x_start;
    if (A.backward_only) {  // controllable sets on their own (+ the controllability verdict for TOPPRAsd)
        if (alive && A.status) A.status[bb] = dead ? TPR_STATUS_FAIL_UNCONTROLLABLE : TPR_STATUS_OK;
        return;
    }
    __threadfence_block();  // K rows were stored by other lanes of the wave and are read back below

    if (SDFWD) {
        // ---- TOPPRAsd: the fastest and the slowest profile (desired_duration_algorithm.py:96-142) ----------------
        // Per stage two 1-D LPs in u at fixed x on the same rows (cy_seidel_solverwrapper.pyx:631-650, :93-144): the
        // fastest profile maximises u from x_fast, the slowest minimises it from x_slow.  No retries here; the shrink
        // is "- SMALL" (:117), and a failed stage poisons the rest of its profile with NaN.
        if (alive && A.status) A.status[bb] = dead ? TPR_STATUS_FAIL_UNCONTROLLABLE : TPR_STATUS_OK;
        double xq[2] = {dead ? qnan() : x_start, dead ? qnan() : x_start};   // [0] fastest, [1] slowest
        double *fst = cols;  // [4][8][BS]: x_fast, u_fast, x_slow, u_slow of 8 consecutive stages (the q columns are free)
        static_assert(!SDFWD || kColDoubles >= 4 * 8 * BS, "staging of four output arrays");
        double *o_x[2] = {A.sd_xf + b0 * (N + 1), A.sd_xl + b0 * (N + 1)};
        double *o_u[2] = {A.sd_uf + b0 * N, A.sd_ul + b0 * N};
        auto s_flush = [&](int which, double *g0, size_t row_stride, int off, int base, int cnt) {  // stage base + p -> column off + base + p
            const int pst = tid & 7;
            double v[BS / 8];
#pragma unroll
            for (int k = 0; k < BS / 8; ++k) v[k] = fst[(which * 8 + ((base + pst) & 7)) * BS + 8 * k + (tid >> 3)];
#pragma unroll
            for (int k = 0; k < BS / 8; ++k) {
                const int t = 8 * k + (tid >> 3);
                if (pst < cnt && t < ntraj) g0[(size_t)t * row_stride + (size_t)(off + base + pst)] = v[k];
            }
        };
        auto s_flush_all = [&](int base, int cnt) {
            TPR_WAVE_SYNC();
            s_flush(0, o_x[0], (size_t)(N + 1), 1, base, cnt);   // x after stage i is x[i + 1]
            s_flush(1, o_u[0], (size_t)N, 0, base, cnt);
            s_flush(2, o_x[1], (size_t)(N + 1), 1, base, cnt);
            s_flush(3, o_u[1], (size_t)N, 0, base, cnt);
            TPR_WAVE_SYNC();
        };
        if (alive) { A.sd_xf[(size_t)bb * (N + 1)] = xq[0]; A.sd_xl[(size_t)bb * (N + 1)] = xq[0]; }
        double s_cur = s_n;  // grid[0]; its q', q'' sit in S.rc1 / S.rc2
        // _compute_duration of both profiles (desired_duration_algorithm.py:11-18), summed stage by stage in the reference's order:
        // t += 2 delta_i / (sd_{i+1} + sd_i + 1e-9) on the values that are stored, NaN included
        double dur[2] = {0.0, 0.0}, sd_prev[2];
        sd_prev[0] = sd_prev[1] = sqrt(xq[0]);
        double s_pf = grid(1), k0_pf = K[2], k1_pf = K[3];
        for (int i = 0; i < N; ++i) {
            const double s_nx = s_pf, k0 = k0_pf, k1 = k1_pf;
            if (i + 2 <= N) { s_pf = grid(i + 2); k0_pf = K[2 * (i + 2)]; k1_pf = K[2 * (i + 2) + 1]; }
            if (i > 0 && (i & 7) == 0) s_flush_all(i - 8, 8);
            const double delta = s_nx - s_cur;
            double nx1[D], nx2[D];
            eval(s_nx, -1, false, nx1, nx2, dummy0, dummy1);
#pragma unroll
            for (int k = 0; k < D; ++k) { S.rn1[k] = INTERP ? nx1[k] : 0.0; S.rn2[k] = INTERP ? nx2[k] : 0.0; }
            S.two_delta = 2 * delta; S.n0 = k0; S.n1 = k1;
            s_cur = s_nx;
            const double td = S.two_delta;
            // One 1-D LP: MINIMISE u (pick_min of cy_solve_lp1d) or maximise it.  The side that carries the answer is
            // divided out row by row as the reference does; the other side only decides feasibility (tmin <= tmax) and is
            // first tested at the answer with a margin far above the rounding of a quotient, divided out only when
            // that is not conclusive.
            auto lp1d = [&](double x, bool minimise, double &u_out) -> bool {
                const double bxc5 = x - S.n1, bxc4 = S.n0 - x;  // rows 5 (a = +2 delta) and 4 (a = -2 delta)
                double au[2 * D], bu[2 * D], bl[2 * D];          // upper-bound twin: (au, bu); lower-bound twin: (-au, bl)
                auto pair = [&](int idx, double a, double b, double cp, double cn) {
                    const bool pos = a > 0;
                    const double bx = b * x;
                    au[idx] = pos ? a : -a;
                    bu[idx] = pos ? bx + cp : -bx + cn;
                    bl[idx] = pos ? -bx + cn : bx + cp;
                };
#pragma unroll
                for (int k = 0; k < D; ++k) pair(k, S.rc1[k], S.rc2[k], S.cpos[k], S.cneg[k]);
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double q2 = S.rn2[k];
                    pair(D + k, S.rn1[k] + td * q2, q2, S.cpos[k], S.cneg[k]);
                }
                constexpr double kRel = 1.0 / (1ll << 40);
                double tmax = kVarMax, tmin = kVarMin;
                auto all_upper = [&]() {
                    const double t5 = -bxc5 / td;
                    tmax = ((td > kTiny) & (t5 < tmax)) ? t5 : tmax;
#pragma unroll
                    for (int j = 0; j < 2 * D; ++j) {
                        const double t = -bu[j] / au[j];
                        tmax = ((au[j] > kTiny) & (t < tmax)) ? t : tmax;
                    }
                };
                auto all_lower = [&]() {
                    const double t4 = -bxc4 / -td;
                    tmin = ((-td < -kTiny) & (t4 > tmin)) ? t4 : tmin;
#pragma unroll
                    for (int j = 0; j < 2 * D; ++j) {
                        const double t = -bl[j] / -au[j];
                        tmin = ((-au[j] < -kTiny) & (t > tmin)) ? t : tmin;
                    }
                };
                if (!minimise) {
                    all_upper();
                    // lower bounds at u = tmax: a_l tmax + (b x + c)_l <= -margin  =>  -(b x + c)_l / a_l < tmax
                    bool sure = tmax > kVarMin;
                    {
                        const double at = -td * tmax;
                        sure &= !(td > kTiny) | (at + bxc4 <= -kRel * (fabs(at) + fabs(bxc4)));
                    }
#pragma unroll
                    for (int j = 0; j < 2 * D; ++j) {
                        const double at = -au[j] * tmax;
                        sure &= !(au[j] > kTiny) | (at + bl[j] <= -kRel * (fabs(at) + fabs(bl[j])));
                    }
                    if (!sure) all_lower();
                } else {
                    all_lower();
                    // upper bounds at u = tmin: a_u tmin + (b x + c)_u <= -margin  =>  -(b x + c)_u / a_u > tmin
                    bool sure = tmin < kVarMax;
                    {
                        const double at = td * tmin;
                        sure &= !(td > kTiny) | (at + bxc5 <= -kRel * (fabs(at) + fabs(bxc5)));
                    }
#pragma unroll
                    for (int j = 0; j < 2 * D; ++j) {
                        const double at = au[j] * tmin;
                        sure &= !(au[j] > kTiny) | (at + bu[j] <= -kRel * (fabs(at) + fabs(bu[j])));
                    }
                    if (!sure) all_upper();
                }
                u_out = minimise ? tmin : tmax;
                return !(tmin > tmax);
            };
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                // fastest: v0 = 2 delta (maximise unless |v0| < TINY); slowest: v0 = -2 delta (always the lower end)
                const bool minimise = w == 1 || td < kTiny;
                double uu = qnan();
                bool ok = false;
                if (!isnan(xq[w])) ok = lp1d(xq[w], minimise, uu);
                if (ok) {
                    const double xn = xq[w] + td * uu - kPySmall;
                    const double m1 = xn > k0 ? xn : k0;
                    xq[w] = m1 < k1 ? m1 : k1;
                } else { uu = qnan(); xq[w] = qnan(); }
                fst[((2 * w + 0) * 8 + (i & 7)) * BS + tid] = xq[w];
                fst[((2 * w + 1) * 8 + (i & 7)) * BS + tid] = uu;
                const double sd_nx = sqrt(xq[w]);
                dur[w] += td / (sd_nx + sd_prev[w] + 1e-9);
                sd_prev[w] = sd_nx;
            }
            if (i == N - 1) s_flush_all(i - (i & 7), (i & 7) + 1);
#pragma unroll
            for (int k = 0; k < D; ++k) { S.rc1[k] = nx1[k]; S.rc2[k] = nx2[k]; }
        }
        if (alive && A.sd_dur) { A.sd_dur[2 * (size_t)bb] = dur[0]; A.sd_dur[2 * (size_t)bb + 1] = dur[1]; }
        return;
    }

    // ---- forward scan: parameterization ----------------------------------------------------
    // One wave-uniform iteration per stage; the reference's retries (lower x_i, solve again, at
    // most 10 times) are an inner per-lane loop.  A lane whose retries are exhausted keeps going
    // with x = NaN, which stores exactly what the reference leaves behind (u = 0, sd2 = NaN).
    double x = dead ? qnan() : x_start;
    // sd = sqrt(x) is only evaluated when it is an output; "sqrt(x) is NaN" is "not x >= 0" (sqrt(-0.0) = -0.0)
    auto root = [](double v) { return WANT_SD ? sqrt(v) : 0.0; };
    double sq = root(x);
    bool any_nan = !(x >= 0.0);
    int tries = 0;
    bool done = dead;
    // sd2, u (and sd) of 8 consecutive stages are staged in LDS -- the q columns are free in this scan -- and
    // written out transposed: 8 adjacent lanes store one trajectory's 64 contiguous bytes
    double *fst = cols;  // [3][8][BS]: x, u, sd
    auto f_flush = [&](int which, double *g0, size_t row_stride, int base, int cnt) {
        const int pst = tid & 7;
        // all LDS reads first (every address is valid, whatever cnt and ntraj are), then the stores: a predicated
        // read-wait-store per row costs an LDS round trip each
        double v[BS / 8];
#pragma unroll
        for (int k = 0; k < BS / 8; ++k) v[k] = fst[(which * 8 + ((base + pst) & 7)) * BS + 8 * k + (tid >> 3)];
        if (cnt == 8 && ntraj == BS) {  // wave-uniform: the full block
#pragma unroll
            for (int k = 0; k < BS / 8; ++k) g0[(size_t)(8 * k + (tid >> 3)) * row_stride + (size_t)(base + pst)] = v[k];
        } else {
#pragma unroll
            for (int k = 0; k < BS / 8; ++k) {
                const int t = 8 * k + (tid >> 3);
                if (pst < cnt && t < ntraj) g0[(size_t)t * row_stride + (size_t)(base + pst)] = v[k];
            }
        }
    };
    double s_cur = s_n;  // grid[0]; its q', q'' sit in parity slot 0 and in S.rc1 / S.rc2
    double s_pf = grid(1), k0_pf = K[2], k1_pf = K[3];  // software prefetch of the next stage's inputs
    for (int i = 0; i < N; ++i) {
        const double s_nx = s_pf, k0 = k0_pf, k1 = k1_pf;
        if (i + 2 <= N) { s_pf = grid(i + 2); k0_pf = K[2 * (i + 2)]; k1_pf = K[2 * (i + 2) + 1]; }
        // The previous eight stages' outputs leave here, AFTER the prefetch above has been consumed and re-issued:
        // loads and stores share one in-order counter (vmcnt), and the wait for the prefetched K at the top of the
        // next iteration also waits for every older store -- issued here they have a whole stage to complete, issued
        // at the end of the iteration (as before) the next stage stalled on them once per eight stages.
        if (i > 0 && (i & 7) == 0) {
            TPR_WAVE_SYNC();
            f_flush(0, xs0, (size_t)(N + 1), i - 8, 8);
            f_flush(1, us0, (size_t)N, i - 8, 8);
            if (WANT_SD) f_flush(2, sd0, (size_t)(N + 1), i - 8, 8);
            TPR_WAVE_SYNC();
        }
        const double delta = s_nx - s_cur;
        double nx1[D], nx2[D];  // q', q'' at s_{i+1}: the stage's interpolation rows (INTERP) and the next stage's own rows
        eval(s_nx, -1, false, nx1, nx2, dummy0, dummy1);
#pragma unroll
        for (int k = 0; k < D; ++k) { S.rn1[k] = INTERP ? nx1[k] : 0.0; S.rn2[k] = INTERP ? nx2[k] : 0.0; }
        S.two_delta = 2 * delta; S.n0 = k0; S.n1 = k1;
        s_cur = s_nx;
        // 1-D LP in u at fixed x: max 2 delta u over the structural rows, u in [-1e8, 1e8]
        double uu = 0.0;
        bool ok = false;
        for (;;) {
            if (!isnan(x)) {
                // max 2 delta u: the answer is tmax, the smallest upper bound -(b x + c)/a over the rows
                // with a > 0 (of a +- pair that is the twin with a > 0).  The lower bounds only decide
                // feasibility (tmin <= tmax); they are first tested at u = tmax with a margin far above
                // the rounding of a quotient, and divided out only when that is not conclusive.
                const double v0 = 2 * delta;
                double tmax = kVarMax;
                const double bxc5 = x - S.n1, bxc4 = S.n0 - x;  // rows 5 (a = +2 delta) and 4 (a = -2 delta)
                {
                    const double t5 = -bxc5 / S.two_delta;
                    tmax = ((S.two_delta > kTiny) & (t5 < tmax)) ? t5 : tmax;
                }
                double al[2 * D], bl[2 * D];  // the lower-bound twin of every pair: a (< 0 when valid), b x + c
                auto pair = [&](int idx, double a, double b, double cp, double cn) {
                    const bool pos = a > 0;
                    const double bx = b * x;
                    const double au = pos ? a : -a;                       // the upper-bound twin's a
                    const double bu = pos ? bx + cp : -bx + cn;           // ... and its b x + c
#ifdef TPR_SOUND_TOLERANCE  // measurement build: reciprocal estimate + one Newton step instead of the IEEE division
                    const double t = -bu * rcp_approx(au);
#else
                    const double t = -bu / au;
#endif
                    tmax = ((au > kTiny) & (t < tmax)) ? t : tmax;
                    al[idx] = -au;
                    bl[idx] = pos ? -bx + cn : bx + cp;
                };
#pragma unroll
                for (int k = 0; k < D; ++k) pair(k, S.rc1[k], S.rc2[k], S.cpos[k], S.cneg[k]);
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double q2 = S.rn2[k];
                    pair(D + k, S.rn1[k] + S.two_delta * q2, q2, S.cpos[k], S.cneg[k]);
                }
                // lower bounds at u = tmax: a_l tmax + (b x + c)_l <= -margin  =>  -(b x + c)_l / a_l < tmax
                constexpr double kRel = 1.0 / (1ll << 40);
                bool sure = !(fabs(v0) < kTiny || v0 < 0) & (tmax > kVarMin);
                {
                    const double at = -S.two_delta * tmax;
                    sure &= !(S.two_delta > kTiny) | (at + bxc4 <= -kRel * (fabs(at) + fabs(bxc4)));
                }
#pragma unroll
                for (int j = 0; j < 2 * D; ++j) {
                    const double at = al[j] * tmax;
                    sure &= !(al[j] < -kTiny) | (at + bl[j] <= -kRel * (fabs(at) + fabs(bl[j])));
                }
                double tmin = kVarMin;
                if (!sure) {  // rare: divide the lower bounds out as the reference does
                    const double t4 = -bxc4 / -S.two_delta;
                    tmin = ((-S.two_delta < -kTiny) & (t4 > tmin)) ? t4 : tmin;
#pragma unroll
                    for (int j = 0; j < 2 * D; ++j) {
                        const double t = -bl[j] / al[j];
                        tmin = ((al[j] < -kTiny) & (t > tmin)) ? t : tmin;
                    }
                }
                ok = !(tmin > tmax);
                uu = (fabs(v0) < kTiny || v0 < 0) ? tmin : tmax;
            }
            if (ok || done || tries >= kMaxTries) break;
            const double t1 = x - kPyTiny, t2 = 0.999 * x;
            x = t2 > t1 ? t2 : t1;
            tries += 1;
            sq = root(x);
        }
        {
            fst[(0 * 8 + (i & 7)) * BS + tid] = x;
            fst[(1 * 8 + (i & 7)) * BS + tid] = dead ? qnan() : (ok ? uu : 0.0);
            if (WANT_SD) fst[(2 * 8 + (i & 7)) * BS + tid] = sq;
            if (i == N - 1) {  // the tail (a full group of eight included)
                const int base = i - (i & 7), cnt = (i & 7) + 1;
                TPR_WAVE_SYNC();
                f_flush(0, xs0, (size_t)(N + 1), base, cnt);
                f_flush(1, us0, (size_t)N, base, cnt);
                if (WANT_SD) f_flush(2, sd0, (size_t)(N + 1), base, cnt);
                TPR_WAVE_SYNC();
            }
        }
        if (!ok && !done) { done = true; any_nan = true; }
        if (ok) {
            tries = 0;
            double xn = x + (2 * delta) * uu;
            const double t1 = xn - kPyTiny, t2 = 0.9999 * xn;
            xn = t2 > t1 ? t2 : t1;
            const double m1 = xn > k0 ? xn : k0;
            x = m1 < k1 ? m1 : k1;
            sq = root(x);
            any_nan |= !(x >= 0.0);
        } else {
            x = qnan();
            sq = qnan();
        }
#pragma unroll
        for (int k = 0; k < D; ++k) { S.rc1[k] = nx1[k]; S.rc2[k] = nx2[k]; }
    }
    if (alive) {
        xs[N] = x;
        if (WANT_SD) sdv[N] = sq;
        A.status[bb] = dead ? TPR_STATUS_FAIL_UNCONTROLLABLE : (any_nan ? TPR_STATUS_ERR_UNKNOWN : TPR_STATUS_OK);
    }
}


// ---- compute_feasible_sets on the certified lane design (reachability_algorithm.py:131-164) -------------------------
// Per stage i = 0..N two 2-D LPs -- min x (objective (-1e-9, -1), warm-start state active_c_up) and max x ((1e-9, 1),
// active_c_down; cy_seidel_solverwrapper.pyx:660-695) -- with x and x_next boxed to +-CVXPY_MAXX, in ascending stage
// order with the reference's warm-start state carried along.  These are the backward scan's LPs with the x_next rows
// pushed out to +-1e4 and the tilt in u reversed, so the stage block is the one of cert_solve_kernel: proposal +
// certificate for the max-x LP, the mirrored lower certificate for the min-x LP (cert_lower<UMAX = false>), the
// cooperative batches (walk, then the reference's full iteration) for what does not certify.  The LAST gridpoint has its
// own row set (MODE 2 of cert_needy_batch) and runs the full iteration for every lane.
// 65536 x 7 x 200: 9.9 ms on the rows-across-lanes kernel (group_feasible_kernel, full iteration for every LP).
template <int D, int BS, bool GRID_LDS, bool INTERP = true, bool SOUND = false>
__global__ void __launch_bounds__(BS) cert_feasible_kernel(GroupArgs A, double *X) {
    using C = CertStage<D, BS>;
#ifndef TPR_SIGNBITS_FEAS_DOFS   // (the slides' verdicts as sign bits, per dof: see cert_solve_kernel)
#define TPR_SIGNBITS_FEAS_DOFS 0x31feu  /* 1..8, 12, 13 (running minimum / sign bits: 2.53 / 3.37 ms at 9 dof, 3.31 / 5.25 at 10, 3.91 / 4.72 at 11, 6.77 / 6.67 at 12, 9.19 / 8.59 at 13) */
#endif
    constexpr bool kSignBitsF = (TPR_SIGNBITS_FEAS_DOFS >> D) & 1u;
    constexpr int kColDoubles = (4 * D + C::kLimCols) * BS;
    constexpr int kRing = C::kRing, kRingTraj = BS / kRing;
    __shared__ double cols[kColDoubles];
    double *qt = cols, *lim = cols + 4 * D * BS;
    __shared__ double scratch[(kCertXch - 1) * BS + cert_batch_groups<D>() * GroupCfg<D, kCertBatchLanes>::kRowBuf];
    __shared__ int needy_queue[2 * BS];
    constexpr bool kDirectK = C::kDirectK;
    __shared__ double kst[kDirectK ? 1 : kRing * 2 * BS];  // feasible sets of kRing stages, written out transposed
    double *xch = scratch, *rowbufs = scratch + (kCertXch - 1) * BS;
    extern __shared__ double grid_lds[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x * BS + tid;
    const bool alive = b < A.B;
    const int bb = alive ? b : A.B - 1;  // idle lanes shadow the last trajectory (computing, never storing)
    const int N = A.N, nseg = A.nseg;
    const double *gcf = A.coef + (size_t)bb * 4 * nseg * D;
    const double *brk = A.breaks + ((A.flags & TPR_BREAKS_PER_TRAJ) ? (size_t)bb * (nseg + 1) : 0);
    const double *ggrid = A.grid + ((A.flags & TPR_GRID_PER_TRAJ) ? (size_t)bb * (N + 1) : 0);
    if (GRID_LDS) {
        for (int e = tid; e <= N; e += BS) grid_lds[e] = A.grid[e];
        __syncthreads();
    }
    auto grid = [&](int i) -> double { return GRID_LDS ? grid_lds[i] : ggrid[i]; };
    const bool has_vel = A.flags & TPR_HAS_VELOCITY;

    // Slim blocks (above 8 dof) re-read limits and, from TPR_LEAN_COEF_FROM dof on, the spline coefficients at every stage.  From the
    // caller's trajectory-major arrays that is one cache line per lane and load (round 5, 12 dof: 9.8 GB fetched per launch for
    // 0.55 GB of algorithmic traffic, half the kernel's time waiting); each block therefore transposes its 64 trajectories' values
    // ONCE into its slice of GroupArgs::tws as [field][lane], and a wave's re-read is 512 contiguous bytes.  A lane only ever
    // re-reads its own column, except in the cooperative batches, which run behind wave-level hand-offs (TPR_WAVE_SYNC).
    const double *tw = nullptr, *tw_blk = nullptr;  // this lane's column / the block's slice
    const double *cbase = gcf;                      // c0, c1, c2 of this trajectory: [3][nseg][D] at stride cstride
    int cstride = 1;
    if constexpr (C::kSlim) {
        const size_t fields = cert_tws_fields(D, nseg);
        double *wb = A.tws + (size_t)blockIdx.x * fields * BS, *w = wb + tid;
        const double *al = A.alim + (size_t)bb * 2 * D;
#pragma unroll
        for (int j = 0; j < 2 * D; ++j) w[j * BS] = al[j];
        const double *vl = has_vel ? A.vlim + (size_t)bb * 2 * D : nullptr;
#pragma unroll
        for (int j = 0; j < 2 * D; ++j) w[(2 * D + j) * BS] = has_vel ? vl[j] : 0.0;
        if constexpr (D >= TPR_LEAN_COEF_FROM) {  // (below, the coefficients live in registers: nothing would read a copy)
            if (nseg <= kTwsMaxSeg) {
                for (int e = 0; e < 3 * nseg * D; ++e) w[(size_t)(4 * D + e) * BS] = gcf[e];
                cbase = w + (size_t)4 * D * BS;
                cstride = BS;
            }
        }
        tw = w; tw_blk = wb;
        TPR_WAVE_SYNC();  // (the cooperative batches read other lanes' columns)
    }
    C S;
    if constexpr (C::kPairFetch) {  // rows 0..5 as (q1, q2) pairs for CertStage::fetch: (1, 0), (+0, 1), (-0, 1)
        __shared__ double spec_rows[C::kSpecDoubles];
        if (tid < C::kSpecDoubles) spec_rows[tid] = (tid == 0 || (tid & 1)) ? (tid == 1 ? 0.0 : 1.0) : (tid == 4 ? -0.0 : 0.0);
        S.spec = spec_rows;
        TPR_WAVE_SYNC();
    }
    double vlo[D], vhi[D];
    {
        const double *alim = A.alim + (size_t)bb * 2 * D;
#pragma unroll
        for (int k = 0; k < D; ++k) { S.cpos[k] = -alim[2 * k + 1]; S.cneg[k] = alim[2 * k]; }
        S.lim = lim + tid;
        S.alim_lane = C::kSlim ? tw : alim;
        lim[0 * BS + tid] = kVarMin; lim[1 * BS + tid] = -kVarMax;
        S.cmax = 0.0;
        S.min_range = 3.0e300;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (!C::kSlim) {
                lim[(6 + k) * BS + tid] = S.cpos[k];
                lim[(6 + D + k) * BS + tid] = S.cneg[k];
            }
            S.cmax = fmax(S.cmax, fmax(fabs(S.cpos[k]), fabs(S.cneg[k])));
            S.min_range = fmin(S.min_range, -S.cpos[k] - S.cneg[k]);
        }
        const double *vlim = has_vel ? A.vlim + (size_t)bb * 2 * D : nullptr;
#pragma unroll
        for (int k = 0; k < D; ++k) { vlo[k] = has_vel ? vlim[2 * k] : 0.0; vhi[k] = has_vel ? vlim[2 * k + 1] : 0.0; }
    }
    // From 10 dof on the velocity limits, from 11 dof on the spline segment's coefficients too, are re-read from global memory
    // where they are used (once per stage, L2-hot) instead of living in 4 D + 6 D registers: the trace-following certificates
    // need those registers -- 0.2 - 0.7 KB of scratch per lane at 10..13 dof otherwise (65536 x d x 200: 4.6 / 7.8 / 7.7 /
    // 10.9 ms at 10..13 dof with everything in registers, 3.8 / 5.0 / 6.1 / 9.2 ms like this;
    // profiles/r04_family3_lean_rereads.log.  At 7 dof, where nothing spills, the re-read costs 15 %: DESIGN 4.1.)
    constexpr bool kLean = D >= TPR_LEAN_VEL_FROM, kLeanCoef = D >= TPR_LEAN_COEF_FROM;
    static_assert(!(kLean || kLeanCoef) || C::kSlim, "the lean re-reads go to the slim blocks' transposed workspace");
    auto vsel = [&](int k, bool upper) -> double {  // one load whichever side is asked for (a select between two loads gets sunk)
        if constexpr (kLean) return tw[(2 * D + 2 * k + (upper ? 1 : 0)) * BS];
        else return upper ? vhi[k] : vlo[k];
    };
    double c0[D], c1[D], c2[D];
    int jcur = -1;
    double seg_lo = 1.0, seg_hi = 0.0, seg_b = 0.0;
    double *col = qt + tid;
    // q', q'' at s into (o1, o2) and LDS parity slot par, and the x box from the velocity limits (as cert_solve_kernel)
    auto eval = [&](double s, int par, double (&o1)[D], double (&o2)[D], double &low1, double &high1) {
        if (!(s >= seg_lo && s < seg_hi)) {
            const int j = find_segment(brk, nseg, s);
            if (j != jcur) {
                if constexpr (!kLeanCoef) {
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        c0[k] = gcf[(0 * nseg + j) * D + k] * 3.0;
                        c1[k] = gcf[(1 * nseg + j) * D + k] * 2.0;
                        c2[k] = gcf[(2 * nseg + j) * D + k];
                    }
                }
                jcur = j;
            }
            seg_b = brk[j];
            seg_lo = j == 0 ? -3.0e300 : seg_b;
            seg_hi = j == nseg - 1 ? 3.0e300 : brk[j + 1];
        }
        const double t = s - seg_b;
        double *d1 = col + (par * 2 + 0) * D * BS, *d2 = col + (par * 2 + 1) * D * BS;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            double q1, q2;
            if constexpr (kLeanCoef) {
                cubic_d1_d2_scaled(cbase[(size_t)(((0 * nseg + jcur) * D + k) * cstride)] * 3.0, cbase[(size_t)(((1 * nseg + jcur) * D + k) * cstride)] * 2.0,
                                   cbase[(size_t)(((2 * nseg + jcur) * D + k) * cstride)], t, q1, q2);
            } else {
                cubic_d1_d2_scaled(c0[k], c1[k], c2[k], t, q1, q2);
            }
            o1[k] = q1; o2[k] = q2;
            d1[k * BS] = q1;
            d2[k * BS] = q2;
        }
        low1 = kVarMin; high1 = kVarMax;
        if (has_vel) {
            double mmax = (double)kJvelMaxSd;
            bool pos_lower = false;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double q1 = o1[k];
                const bool valid = (q1 != 0) & !isnan(q1);
                const double rmax = vsel(k, q1 > 0) / q1;
                mmax = (valid & (rmax <= mmax)) ? rmax : mmax;
                { const double vv = vsel(k, !(q1 > 0)); pos_lower |= (q1 > 0) ? vv > 0 : ((q1 < 0) & (vv < 0)); }
            }
            const float sdmax = (float)mmax;
            double xlo = 0.0;
            if (pos_lower) {
                float sdmin = -kJvelMaxSd;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double q1 = o1[k];
                    const double rmin = vsel(k, !(q1 > 0)) / q1;
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
        // x_min / x_max of solve_stagewise_optim intersect the box (cy_seidel_solverwrapper.pyx:598-601)
        low1 = low1 > -kFeasMaxX ? low1 : -kFeasMaxX;
        high1 = high1 < kFeasMaxX ? high1 : kFeasMaxX;
    };
    auto bind = [&](int i) {  // stage i: cur = parity of i, nxt = parity of i+1
        const int pc = i & 1, pn = pc ^ 1;
        S.cur1 = col + (pc * 2 + 0) * D * BS; S.cur2 = col + (pc * 2 + 1) * D * BS;
        S.nxt1 = col + (pn * 2 + 0) * D * BS; S.nxt2 = col + (pn * 2 + 1) * D * BS;
    };
    const size_t b0 = (size_t)blockIdx.x * BS;
    const int ntraj = A.B - (int)b0 < BS ? A.B - (int)b0 : BS;
    double *X0 = X + b0 * 2 * (N + 1);
    const double *alim_blk = tw_blk;
    auto x_put = [&](int i, double lo_, double hi_) {
        if constexpr (kDirectK) {
            if (tid < ntraj) *reinterpret_cast<double2 *>(X0 + (size_t)tid * 2 * (size_t)(N + 1) + (size_t)i * 2) = make_double2(lo_, hi_);
        } else {
            kst[((i & (kRing - 1)) * 2 + 0) * BS + tid] = lo_;
            kst[((i & (kRing - 1)) * 2 + 1) * BS + tid] = hi_;
        }
    };
    auto x_flush = [&](int base, int cnt) {  // stages [base, base + cnt), cnt <= kRing, base % kRing == 0
        if constexpr (kDirectK) return;
        TPR_WAVE_SYNC();
        const int pst = tid & (kRing - 1), slot = (base + pst) & (kRing - 1);
        double2 v[kRing];
#pragma unroll
        for (int k = 0; k < kRing; ++k) v[k] = make_double2(kst[(slot * 2) * BS + kRingTraj * k + (tid / kRing)], kst[(slot * 2 + 1) * BS + kRingTraj * k + (tid / kRing)]);
#pragma unroll
        for (int k = 0; k < kRing; ++k) {
            const int t = kRingTraj * k + (tid / kRing);
            if (pst < cnt && t < ntraj) *reinterpret_cast<double2 *>(X0 + (size_t)t * 2 * (size_t)(N + 1) + (size_t)(base + pst) * 2) = v[k];
        }
        TPR_WAVE_SYNC();
    };

    int up0 = 4, up1 = 4, dn0 = 4, dn1 = 4;  // a fresh wrapper object's state, internal row numbering

    double low1, high1;
    double s_i = grid(0);
    eval(s_i, 0, S.rc1, S.rc2, low1, high1);
    for (int i = 0; i < N; ++i) {
        const double s_n = grid(i + 1);
        double nx1[D], nx2[D], low1_n, high1_n;
        eval(s_n, (i + 1) & 1, nx1, nx2, low1_n, high1_n);
#pragma unroll
        for (int k = 0; k < D; ++k) { S.rn1[k] = INTERP ? nx1[k] : 0.0; S.rn2[k] = INTERP ? nx2[k] : 0.0; }
        bind(i);
        S.two_delta = 2 * (s_n - s_i); S.n0 = -kFeasMaxX; S.n1 = kFeasMaxX; S.low1 = low1; S.high1 = high1;
        S.publish_special(lim + tid);
        double nmax;
        const bool nok = S.norms(nmax);
        Lp2dOut su, sl;
        int up_p, up_q;
        bool up_ok;
        double up_prow[3], up_qrow[3];
        if constexpr (SOUND) cert_propose_sound<D, BS, 0, kSignBitsF>(S, 1e-9, 1.0, dn0, dn1, dn0 != dn1, nmax, up_p, up_q, up_ok, up_prow, up_qrow);
        else cert_propose2<D, BS>(S, 1e-9, 1.0, dn0, dn1, dn0 != dn1, false, nmax, up_p, up_q, up_ok, up_prow, up_qrow);
        bool need_u = !cert_pair_rows<D, BS, false, SOUND>(S, 1e-9, 1.0, up_p, up_q, nok & up_ok, up_prow[0], up_prow[1], up_prow[2],
                                                    up_qrow[0], up_qrow[1], up_qrow[2], dn0, dn1, nmax, su);
        bool need_l;
        if constexpr (SOUND) need_l = !cert_lower_sound<D, BS, false, kSignBitsF>(S, nok, nmax, up0, up1, sl);
        else need_l = !cert_lower<D, BS, false>(S, nok, nmax, sl);
        if (__builtin_amdgcn_ballot_w64(need_u | need_l) != 0)
            cert_needy_batch<D, BS, INTERP, 1, SOUND>(S, qt, i & 1, lim, alim_blk, ntraj, xch, needy_queue, rowbufs, need_u, need_l, dn0, dn1, up0, up1, su, sl);
        if (su.ok) { dn0 = su.ac0; dn1 = su.ac1; } else su.x = qnan();
        if (sl.ok) { up0 = sl.ac0; up1 = sl.ac1; } else sl.x = qnan();
        double lo = sl.x;
        if (lo < 0) lo = 0;
        x_put(i, lo, su.x);
        if ((i & (kRing - 1)) == kRing - 1) x_flush(i - (kRing - 1), kRing);
#pragma unroll
        for (int k = 0; k < D; ++k) { S.rc1[k] = nx1[k]; S.rc2[k] = nx2[k]; }
        low1 = low1_n; high1 = high1_n;
        s_i = s_n;
    }
    {   // the last gridpoint: x_next pair disabled, interpolation block = the stage's own rows, two_delta = 0
        bind(N);
        S.two_delta = 0.0; S.n0 = -kFeasMaxX; S.n1 = kFeasMaxX; S.low1 = low1; S.high1 = high1;
        S.publish_special(lim + tid);
        Lp2dOut su, sl;
        su.ok = sl.ok = false; su.u = sl.u = su.x = sl.x = qnan(); su.ac0 = su.ac1 = sl.ac0 = sl.ac1 = 4;
        cert_needy_batch<D, BS, INTERP, 2, SOUND>(S, qt, N & 1, lim, alim_blk, ntraj, xch, needy_queue, rowbufs, true, true, dn0, dn1, up0, up1, su, sl);
        if (!su.ok) su.x = qnan();
        if (!sl.ok) sl.x = qnan();
        double lo = sl.x;
        if (lo < 0) lo = 0;
        x_put(N, lo, su.x);
        x_flush(N & ~(kRing - 1), (N & (kRing - 1)) + 1);
    }
}

}  // namespace tpr

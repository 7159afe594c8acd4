// tpr_mount.hip.inc -- the base reaction of a rigid-body tree: the wrench its mount (a pedestal's flange, a cart's footprint, a
// ceiling plate) exerts ON the robot, at every gridpoint of every trajectory.  The model is the tree kernels' (tpr_chain with a
// parent table; a serial chain is the tree parent = -1, 0, 1, ...), the recursion is tpr_chain_rnea.hip.inc's -- chain_link,
// chain_joint and chain_forward<Level> are used as they are -- and the walk is the tree kernels' way up only.
//
// The wrench.  It is linear in gravity, and at rest the net force on link i is its weight's support whatever the pose: so the
// weight's part is summed in BASE coordinates and only the rest goes through the recursion, started from a base at rest (as the
// tool-acceleration kernels start it).  With W_i the link frame's rotation and p_i its origin in base coordinates
//   (W_i = W E_i,  p_i = p + W r_i  from the parent's W, p; the base: W = 1, p = 0),  m_i and c_i the link's mass and centre of mass,
// and F_i, N_i of chain_forward WITHOUT gravity (the net force on link i and its net moment about c_i, link axes):
//   weight    fg = sum_i -m_i gravity,          ng = sum_i (p_i + W_i c_i) x (-m_i gravity)
//   dynamic   fd = sum_i W_i F_i,               nd = sum_i [ W_i (N_i + c_i x F_i) + p_i x (W_i F_i) ]
// f = fg + fd, n = ng + nd is what the base must supply: force and moment about the base origin, base axes.  A platform of mass
// mb at cb, fixed to the base, adds -mb gravity and cb x (-mb gravity) to the weight's part.  In the mount frame (axes Rm, origin
// pm, both in base coordinates):  f' = Rm' f,  n' = Rm' (n - pm x f).
// Why the weight apart: carried through the recursion, gravity is turned into every link's frame and back -- 2 i rotations for link
// i -- and the static force comes out with an error of about d roundings of the weight, where the textbook recursion in base
// coordinates (tests/base_wrench_ref.py) never turns it at all: at 15 and 17 dof that is 1.0 - 1.7 x the accuracy bound.  Apart, it
// is a sum of products, w(q, 0, 0) needs no recursion at all, and the three evaluations share it.
// No backward pass and no per-link state: a point's state is registers at any dof -- W, p, the weight's sums, the running
// (w, wd, a) per level and the dynamic sums (f, n) per level.
//
// THE SUMMATION ORDER, fixed: links in ascending number, the sum on the left, (((0 + t_0) + t_1) + ...), the platform last in the
// weight's part; then weight + dynamic; then the mount frame.  The levels share W, p, E_i, r_i and the weight's part; level 1
// drops the products by an exact zero as chain_forward does, level 0 has no dynamic part, and every output passes through
// "+ 0.0": each output of the fused kernel equals the single evaluation on the same arguments in every bit, and without gravity
// w0 is +0.  A chain-shaped tree never touches a bank, so it evaluates what a chain would.
//
// Forks.  A fork (TreeTables) stores W, p and its (w, wd, a) per level in its bank once they are computed: [fork][slot][lane]
// behind the staging area, 21 doubles (27 fused: level 1 has no w).  A link whose parent is not the link before it loads them from the parent's
// bank, or restarts from the base (a further root).  Every decision reads the tables by the loop index: wave-uniform branches
// around LDS accesses, never around arithmetic.
//
// Shape: the tool-wrench kernels'.  One wave of 64 points per block; q, q', q'' [64][d] pass through LDS (chain_rows_load, read
// back one row per lane at the odd pitch d | 1) and the 6-wide outputs leave through the same LDS at pitch 7
// (chain_accel_rows_store).  Lanes past the last point of the batch work on the last point's row again and rewrite its LDS row
// with its values (no lane is masked out); only npts rows leave.  Dynamic LDS: mount_lds_bytes.
#pragma once
#define TPR_CHAIN_STAGING_ONLY  // (chain_accel_lds_bytes, chain_stage, chain_accel_rows_store; none of the chain kernels)
#include "tpr_chain.hip.inc"
#include "tpr_mount_args.hpp"

namespace tpr {

// Staging (chain_accel_lds_bytes) plus one bank per fork: at most 50 688 + 4 * 27 * 512 = 105 984 bytes.
__host__ __device__ constexpr size_t mount_lds_bytes(int d, int forks, bool fused) {
    return chain_accel_lds_bytes(d, fused ? 3 : 1) + (size_t)forks * (size_t)(fused ? kMountBankFused : kMountBankSingle) * kChainBlock * sizeof(double);
}
static_assert(mount_lds_bytes(kTreeMaxDof, kTreeMaxForks, true) == 50688 + 4 * 27 * 512 && mount_lds_bytes(kTreeMaxDof, kTreeMaxForks, true) == 105984 &&
                  mount_lds_bytes(kTreeMaxDof, kTreeMaxForks, true) <= (size_t)kChainLdsBytes,
              "staging plus four fused banks fit the LDS at 32 dof");
static_assert(mount_lds_bytes(kTreeMaxDof, kTreeMaxForks, false) == 50688 + 4 * 21 * 512, "... and the single evaluation's");

// What is read from the kernel's argument block where it is needed, behind an offset the compiler cannot see through, as the
// tool-wrench kernels read their payload: fetched up front (where the compiler moves loads of arguments to by itself) it would sit
// in scalar registers across the loop, beside a link's parameters, and spill.
//   the mount's 16 doubles, after the loop: rot[9], origin[3], mass, com[3] in this order;
//   the byte tables of the walk (which parent, which bank), where a branch begins or ends -- as 32-bit words, the byte taken out
//   by scalar shifts: there is no scalar load of a byte, and a vector load would make the walk's branches divergent in the
//   compiler's eyes.  The masks stay in scalar registers.
// The asm is NOT volatile: it hides a number and touches no memory.  A volatile one ahead of the loop counts as a possible store,
// and the links' parameters would then be loaded per lane into 56 vector registers instead of by scalar loads.
typedef const __attribute__((address_space(4))) char *MountArgBytes;
typedef const __attribute__((address_space(4))) double *MountWords;
typedef const __attribute__((address_space(4))) uint32_t *MountTable;
__device__ __forceinline__ MountArgBytes mount_arg_bytes() {
    unsigned off = 0;
    asm("" : "+s"(off));
    return (MountArgBytes)__builtin_amdgcn_kernarg_segment_ptr() + off;
}
template <class Args>
__device__ __forceinline__ MountWords mount_words() {
    static_assert(sizeof(MountFrame) == 16 * sizeof(double) && offsetof(Args, P) % 8 == 0, "the mount is 16 packed doubles");
    return (MountWords)(mount_arg_bytes() + offsetof(Args, P));
}
template <class Args>
__device__ __forceinline__ MountTable mount_parents() { return (MountTable)(mount_arg_bytes() + offsetof(Args, T) + offsetof(TreeTables, parent)); }
template <class Args>
__device__ __forceinline__ MountTable mount_fork_slots() { return (MountTable)(mount_arg_bytes() + offsetof(Args, T) + offsetof(TreeTables, fork_slot)); }
__device__ __forceinline__ int mount_table_at(MountTable t, int i) { return (int)(int8_t)(t[i >> 2] >> ((i & 3) * 8)); }
static_assert(offsetof(MountWrenchArgs, T) % 4 == 0 && offsetof(MountWrenchTermsArgs, T) % 4 == 0 && offsetof(TreeTables, parent) % 4 == 0 &&
                  offsetof(TreeTables, fork_slot) % 4 == 0, "the tables start on a word");

// This lane's banks: [fork][slot][lane].
template <int Doubles>
struct MountBanks : ChainLaneBanks<Doubles> {
    using ChainLaneBanks<Doubles>::at;
    __device__ __forceinline__ M3 frame(int b) {
        M3 W;
#pragma unroll
        for (int k = 0; k < 9; ++k) W.m[k] = at(b, k);
        return W;
    }
    __device__ __forceinline__ void put_frame(int b, const M3 &W) {
#pragma unroll
        for (int k = 0; k < 9; ++k) at(b, k) = W.m[k];
    }
};

struct MountSum { V3 f, n; };  // the links' wrench so far: base axes, the moment about the base origin

// Link i's dynamic share, added on the right of the sums.
__device__ __forceinline__ void mount_add(const ChainLink &L, const M3 &W, V3 p, V3 F, V3 Nm, MountSum &S) {
    const V3 t = Nm + cross(L.com, F), Wf = mul(W, F);
    S.f = S.f + Wf;
    S.n = S.n + (mul(W, t) + cross(p, Wf));
}

// The weight's part plus a level's dynamic part, in the mount frame; o[6].  (cross(f, pm) is -pm x f in every bit.)
__device__ __forceinline__ void mount_put(MountWords P, const MountSum &G, const MountSum &S, double *o) {
    const V3 f = G.f + S.f, n = G.n + S.n;
    M3 Rm;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rm.m[k] = P[k];
    chain_put6(mul_t(Rm, f), mul_t(Rm, n + cross(f, V3{P[9], P[10], P[11]})), o);
}

// This lane's walk over the links.  G: the weight's part, platform included.  Fused: S1, S2 = the dynamic parts of w(q, 0, v1) and
// w(q, v1, v2) (that of w(q, 0, 0) is an exact zero and is not computed); otherwise S2 alone.  bq, b1, b2 are this lane's rows
// in the staging area, banks this lane's first bank slot.
// Bank slots: W at 0, p at 9; then fused wd1 a1 | w2 wd2 a2 at 12, 18; single w wd a at 12.
template <bool Fused, class Args>
__device__ __forceinline__ void mount_walk(const ChainModel &M, const TreeTables &T, double *banks, const double *bq, const double *b1,
                                           const double *b2, MountSum &G, MountSum &S1, MountSum &S2) {
    constexpr int kBank2 = Fused ? 18 : 12;  // first bank slot of the level-2 evaluation
    MountBanks<Fused ? kMountBankFused : kMountBankSingle> Bk{banks};
    const MountTable parents = mount_parents<Args>(), slots = mount_fork_slots<Args>();
    const int d = M.d;
    const V3 zero{0.0, 0.0, 0.0};
    const M3 one{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
    const ChainKin base{zero, zero, zero};  // (the base at rest: gravity is not in the recursion)
    ChainKin K1 = base, K2 = base;
    M3 W = one;
    V3 p = zero;
    G = S1 = S2 = MountSum{zero, zero};
#pragma nounroll
    for (int i = 0; i < d; ++i) {
        if (!((T.running >> i) & 1u)) {  // (the same for every lane)
            const int par = mount_table_at(parents, i);
            if (par < 0) {
                W = one; p = zero;
                K1 = base; K2 = base;
            } else {
                const int b = mount_table_at(slots, par);
                W = Bk.frame(b);
                p = Bk.get(b, 9);
                if (Fused) K1 = ChainKin{zero, Bk.get(b, 12), Bk.get(b, 15)};
                K2 = ChainKin{Bk.get(b, kBank2), Bk.get(b, kBank2 + 3), Bk.get(b, kBank2 + 6)};
            }
        }
        const ChainLink L = chain_link(M, i);
        const double qi = bq[i], v1 = b1[i], v2 = b2[i];
        double sq, cq;
        sincos(qi, &sq, &cq);
        ChainJoint J = chain_joint(L, L.prismatic ? qi : sq, cq);
        // A link's 50 doubles of parameters in scalar registers at once, beside what the walk carries, are more than there are.
        // The joint's part (rot, trans, axis: 30) is dead once J stands; what the recursion reads (axis, mass, com, inertia: 26) is
        // fetched only then -- by a link number the compiler cannot tell from i, that waits for J.
        int ib = i;
        asm("" : "+s"(ib), "+v"(J.r.x));
        const ChainLink Lb = chain_link(M, ib);
        p = p + mul(W, J.r);
        W = mul(W, J.E);
        const V3 g = load3(M.gravity), fg = V3{-g.x, -g.y, -g.z} * Lb.mass;  // (gravity is fetched where it is needed, not held across the loop)
        G.f = G.f + fg;
        G.n = G.n + cross(p + mul(W, Lb.com), fg);
        V3 F, Nm;
        if (Fused) {
            chain_forward<1>(Lb, J, K1, 0.0, v1, F, Nm);
            mount_add(Lb, W, p, F, Nm, S1);
        }
        chain_forward<2>(Lb, J, K2, v1, v2, F, Nm);
        mount_add(Lb, W, p, F, Nm, S2);
        if ((T.forks >> i) & 1u) {  // (the same for every lane)
            const int own = mount_table_at(slots, i);
            Bk.put_frame(own, W); Bk.put(own, 9, p);
            if (Fused) {
                Bk.put(own, 12, K1.wd); Bk.put(own, 15, K1.a);
            }
            Bk.put(own, kBank2, K2.w); Bk.put(own, kBank2 + 3, K2.wd); Bk.put(own, kBank2 + 6, K2.a);
        }
    }
    // the platform: its weight's support at its centre of mass
    const MountWords P = mount_words<Args>();
    const V3 g = load3(M.gravity), fp = V3{-g.x, -g.y, -g.z} * P[12];
    G.f = G.f + fp;
    G.n = G.n + cross(V3{P[13], P[14], P[15]}, fp);
}

static __global__ void __launch_bounds__(kChainBlock) mount_wrench_kernel(MountWrenchArgs A) {
    extern __shared__ double chain_lds[];
    const ChainModel &M = A.M;
    const int d = M.d;
    const ChainStage B = chain_stage(chain_lds, A.q, A.qd, A.qdd, A.npoints, d);
    double *banks = chain_lds + chain_accel_lds_bytes(d, 1) / sizeof(double) + threadIdx.x;
    MountSum G, S1, S2;
    mount_walk<false, MountWrenchArgs>(M, A.T, banks, B.bq + B.row, B.b1 + B.row, B.b2 + B.row, G, S1, S2);
    __syncthreads();
    mount_put(mount_words<MountWrenchArgs>(), G, S2, chain_lds + B.lane * 7);
    __syncthreads();
    chain_accel_rows_store(chain_lds, A.wrench, B.g0, B.npts);
}

// w0 = w(q, 0, 0), wa = w(q, 0, qs), wb = w(q, qs, qss) in one pass over the links.
static __global__ void __launch_bounds__(kChainBlock) mount_wrench_terms_kernel(MountWrenchTermsArgs A) {
    extern __shared__ double chain_lds[];
    const ChainModel &M = A.M;
    const int d = M.d;
    const ChainStage B = chain_stage(chain_lds, A.q, A.qs, A.qss, A.npoints, d);
    double *banks = chain_lds + chain_accel_lds_bytes(d, 3) / sizeof(double) + threadIdx.x;
    MountSum G, S1, S2;
    mount_walk<true, MountWrenchTermsArgs>(M, A.T, banks, B.bq + B.row, B.b1 + B.row, B.b2 + B.row, G, S1, S2);
    double *o0 = chain_lds, *oa = o0 + kChainBlock * 7, *ob = oa + kChainBlock * 7;
    __syncthreads();
    const MountWords P = mount_words<MountWrenchTermsArgs>();
    const V3 zero{0.0, 0.0, 0.0};
    mount_put(P, G, MountSum{zero, zero}, o0 + B.lane * 7);
    mount_put(P, G, S1, oa + B.lane * 7);
    mount_put(P, G, S2, ob + B.lane * 7);
    __syncthreads();
    chain_accel_rows_store(o0, A.w0, B.g0, B.npts);
    chain_accel_rows_store(oa, A.wa, B.g0, B.npts);
    chain_accel_rows_store(ob, A.wb, B.g0, B.npts);
}

}  // namespace tpr

// tpr_momentum.hip.inc -- how much motion a rigid-body tree carries: the linear and angular momentum and twice the kinetic energy
// of a set of its links per unit of path velocity, at every gridpoint of every trajectory, and the bound on x = sd^2 that limits on
// them imply.  The model is the tree kernels' (tpr_chain with a parent table; a serial chain is the tree parent = -1, 0, 1, ...);
// the walk is the base-reaction kernels' (tpr_mount.hip.inc: frames W, origins p, banks at forks, tables read from the argument
// block), with the velocity recursion of the tool-velocity kernel in place of the second-order one: its first-order sibling.
//
// The quantities.  qd = q'.  With W_i the link frame's rotation and p_i its origin in base coordinates
//   (W_i = W E_i,  p_i = p + W r_i  from the parent's W, p; the base: W = 1, p = 0),
// v_i, w_i the velocity of the link frame's origin and the angular velocity, in link axes
//   (v_i = E_i' (v + w x r_i) + [prismatic] z qd_i,  w_i = E_i' w + [revolute] z qd_i  from the parent's v, w; the base: 0, 0),
// m_i, c_i, I_i the link's mass, centre of mass and inertia about it, and  vc_i = v_i + w_i x c_i:
//   h_i = (W_i vc_i) m_i
//   P   = sum_i h_i                                              linear momentum, base axes
//   L   = sum_i [ W_i (I_i w_i) + (p_i + W_i c_i) x h_i ]        angular momentum about the base origin, base axes
//   T2  = sum_i [ m_i (vc_i . vc_i) + w_i . (I_i w_i) ]          = q'' M(q) q', twice the kinetic energy per sd^2
// In the mount frame (axes Rm, origin o, both in base coordinates):  P' = Rm' P,  L' = Rm' (L - o x P).  The mount's platform is
// fixed to the base: it does not move and is not read.
// The bound.  With limit = (p_max^2, L_max^2, 2 E_max) of the point's trajectory:
//   xbound = (0, min(limit_0 / |P'|^2, limit_1 / |L'|^2, limit_2 / T2)),   |a|^2 = (a_x a_x + a_y a_y) + a_z a_z
// IEEE divisions of the outputs as they leave: +inf switches a term off, and a standstill gives +inf.
//
// THE SUMMATION ORDER, fixed: links of the set in ascending number, the sum on the left, (((0 + t_0) + t_1) + ...); then the mount
// frame; every output passes through "+ 0.0", so a robot at a standstill gives +0.  Links outside the set are skipped -- the same
// decision for every lane -- not multiplied by zero, and the walk ends after the highest link of the set (the numbering is
// topological: its ancestors have all been visited by then).  Each output is computed whichever of the others is asked for.
//
// Forks.  A fork (TreeTables) stores W, p, v, w in its bank once they are computed: [fork][slot][lane] behind the staging area, 18
// doubles.  A link whose parent is not the link before it loads them from the parent's bank, or restarts from the base (a further
// root).  Every decision reads the tables by the loop index: wave-uniform branches.
//
// Shape: the base-reaction kernels'.  One wave of 64 points per block; q, q' [64][d] pass through LDS (consecutive lanes on
// consecutive doubles, read back one row per lane at the odd pitch d | 1) and the nine outputs of a point leave through the same
// LDS as one row at pitch 9.  Lanes past the last point of the batch work on the last point's row again and rewrite its LDS row
// with its values (no lane is masked out); only npts rows leave.  A point's state -- W, p, v, w, P, L, T2 -- is registers at any
// dof; a link's parameters come from scalar loads by the loop index.  Dynamic LDS: momentum_lds_bytes.
#pragma once
#include "tpr_chain_rnea.hip.inc"
#include "tpr_momentum_args.hpp"

namespace tpr {

// The walk's byte tables and the mount's frame are read from the kernel's argument block where they are needed, behind an offset
// the compiler cannot see through (as the base-reaction kernels read theirs): fetched up front they would sit in scalar registers
// across the loop, beside a link's parameters.  The tables as 32-bit words, the byte taken out by scalar shifts.
typedef const __attribute__((address_space(4))) char *MomentumArgBytes;
typedef const __attribute__((address_space(4))) double *MomentumWords;
typedef const __attribute__((address_space(4))) uint32_t *MomentumTable;
typedef const __attribute__((address_space(4))) MomentumArgs MomentumLate;
__device__ __forceinline__ MomentumArgBytes momentum_arg_bytes() {
    unsigned off = 0;
    asm("" : "+s"(off));
    return (MomentumArgBytes)__builtin_amdgcn_kernarg_segment_ptr() + off;
}
__device__ __forceinline__ int momentum_table_at(MomentumTable t, int i) { return (int)(int8_t)(t[i >> 2] >> ((i & 3) * 8)); }
static_assert(offsetof(MomentumArgs, T) % 4 == 0 && offsetof(TreeTables, parent) % 4 == 0 && offsetof(TreeTables, fork_slot) % 4 == 0,
              "the tables start on a word");
static_assert(offsetof(MomentumArgs, P) % 8 == 0 && offsetof(MountFrame, rot) == 0 && offsetof(MountFrame, origin) == 9 * sizeof(double),
              "the mount's frame is 12 packed doubles: rot, origin");

// The block's rows [npts][d] of two arrays into LDS at `pitch`: (row, column) of element k advance without a division.
__device__ __forceinline__ void momentum_rows_load(double *b0, double *b1, const double *s0, const double *s1, size_t g0, int npts, int d, int pitch) {
    const size_t base = g0 * (size_t)d;
    const int step_r = kChainBlock / d, step_c = kChainBlock % d;
    int r = (int)threadIdx.x / d, c = (int)threadIdx.x % d;
    for (int k = threadIdx.x; k < npts * d; k += kChainBlock) {
        const int at = r * pitch + c;
        b0[at] = s0[base + k]; b1[at] = s1[base + k];
        r += step_r; c += step_c;
        if (c >= d) { c -= d; ++r; }
    }
}
// ... and `width` columns from column `c0` of a block's output rows (pitch kMomentumOut) to dst [npts][width].
__device__ __forceinline__ void momentum_rows_store(const double *buf, double *dst, size_t g0, int npts, int c0, int width) {
    for (int k = threadIdx.x; k < npts * width; k += kChainBlock) dst[g0 * (size_t)width + k] = buf[(k / width) * kMomentumOut + c0 + (k % width)];
}

static __global__ void __launch_bounds__(kChainBlock) momentum_kernel(MomentumArgs A) {
    extern __shared__ double momentum_lds[];
    const ChainModel &M = A.M;
    const int d = M.d, pitch = d | 1;
    const size_t g0 = (size_t)blockIdx.x * kChainBlock;
    const int left = A.npoints - (int)g0, npts = left < kChainBlock ? left : kChainBlock;
    double *bq = momentum_lds, *b1 = bq + kChainBlock * pitch;
    momentum_rows_load(bq, b1, A.q, A.qs, g0, npts, d, pitch);
    __syncthreads();
    const int lane = (int)threadIdx.x < npts ? (int)threadIdx.x : npts - 1, row = lane * pitch;
    ChainLaneBanks<kMomentumBank> Bk{momentum_lds + momentum_stage_doubles(d) + threadIdx.x};
    const MomentumTable parents = (MomentumTable)(momentum_arg_bytes() + offsetof(MomentumArgs, T) + offsetof(TreeTables, parent));
    const MomentumTable slots = (MomentumTable)(momentum_arg_bytes() + offsetof(MomentumArgs, T) + offsetof(TreeTables, fork_slot));
    const V3 zero{0.0, 0.0, 0.0};
    const M3 one{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
    M3 W = one;
    V3 p = zero, v = zero, w = zero, Ps = zero, Ls = zero;
    double T2 = 0.0;
#pragma nounroll
    for (int i = 0; i < A.nlinks; ++i) {
        if (!((A.T.running >> i) & 1u)) {  // (the same for every lane)
            const int par = momentum_table_at(parents, i);
            if (par < 0) {
                W = one; p = zero; v = zero; w = zero;
            } else {
                const int b = momentum_table_at(slots, par);
#pragma unroll
                for (int k = 0; k < 9; ++k) W.m[k] = Bk.at(b, k);
                p = Bk.get(b, 9); v = Bk.get(b, 12); w = Bk.get(b, 15);
            }
        }
        const ChainLink L = chain_link(M, i);  // (of it the joint's part alone is read: rot, trans, axis)
        const double qi = bq[row + i], qd = b1[row + i];
        double sq, cq;
        sincos(qi, &sq, &cq);
        const ChainJoint J = chain_joint(L, L.prismatic ? qi : sq, cq);
        const V3 zr = L.prismatic ? zero : L.axis, zp = L.prismatic ? L.axis : zero;
        v = mul_t(J.E, v + cross(w, J.r)) + zp * qd;
        w = mul_t(J.E, w) + zr * qd;
        p = p + mul(W, J.r);
        W = mul(W, J.E);
        if ((A.mask >> i) & 1u) {  // (the same for every lane)
            // The body's part of the link's parameters (mass, com, inertia: 10 doubles) is fetched only now, by a link number the
            // compiler cannot tell from i, that waits for the joint's part (rot, trans, axis: 15) to be dead: both in scalar
            // registers at once, beside what the walk carries, are more than there are.
            int ib = i;
            asm("" : "+s"(ib), "+v"(w.x));
            const double mass = M.mass[ib];
            const V3 c = load3(M.com + 3 * ib);
            ChainLink Lb;  // (the inertia alone)
#pragma unroll
            for (int k = 0; k < 6; ++k) Lb.I[k] = M.inertia[6 * ib + k];
            const V3 vc = v + cross(w, c), Iw = inertia_mul(Lb, w);
            const V3 h = mul(W, vc) * mass;
            Ps = Ps + h;
            Ls = Ls + (mul(W, Iw) + cross(p + mul(W, c), h));
            T2 = T2 + (mass * dot(vc, vc) + dot(w, Iw));
        }
        if ((A.T.forks >> i) & 1u) {  // (the same for every lane)
            const int own = momentum_table_at(slots, i);
#pragma unroll
            for (int k = 0; k < 9; ++k) Bk.at(own, k) = W.m[k];
            Bk.put(own, 9, p); Bk.put(own, 12, v); Bk.put(own, 15, w);
        }
    }
    // the mount frame (cross(P, o) is -o x P in every bit)
    const MomentumWords F = (MomentumWords)(momentum_arg_bytes() + offsetof(MomentumArgs, P));
    M3 Rm;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rm.m[k] = F[k];
    __syncthreads();  // every lane has read its rows: the outputs take their place
    double *o = momentum_lds + lane * kMomentumOut;
    const V3 z{0.0, 0.0, 0.0};
    const V3 Pm = mul_t(Rm, Ps) + z, Lm = mul_t(Rm, Ls + cross(Ps, V3{F[9], F[10], F[11]})) + z;  // ("+ 0.0")
    const double E2 = T2 + 0.0;
    o[0] = Pm.x; o[1] = Pm.y; o[2] = Pm.z;
    o[3] = Lm.x; o[4] = Lm.y; o[5] = Lm.z;
    o[6] = E2;
    // (where the outputs go is read from the argument block here, as the mount is: held across the loop, six pointers are twelve
    // scalar registers)
    const MomentumLate *out = (const MomentumLate *)momentum_arg_bytes();
    double *const o_momentum = out->momentum, *const o_energy2 = out->energy2, *const o_xbound = out->xbound;
    if (o_xbound) {  // (the same for every lane)
        const double *lim = out->limit + 3 * ((g0 + (size_t)lane) / (size_t)out->n1);
        double best = lim[0] / dot(Pm, Pm);
        const double xl = lim[1] / dot(Lm, Lm), xe = lim[2] / E2;
        best = xl < best ? xl : best;
        best = xe < best ? xe : best;
        o[7] = 0.0; o[8] = best;
    }
    __syncthreads();
    if (o_momentum) momentum_rows_store(momentum_lds, o_momentum, g0, npts, 0, 6);
    if (o_energy2) momentum_rows_store(momentum_lds, o_energy2, g0, npts, 6, 1);
    if (o_xbound) momentum_rows_store(momentum_lds, o_xbound, g0, npts, 7, 2);
}

}  // namespace tpr

// tpr_effmass.hip.inc -- what a contact at a point of a rigid-body tree meets: the point's squared speed per unit of path velocity,
// s2, and the mobility g = tau' M(q)^-1 tau of the robot along the contact force (tau = J_p' f), at every gridpoint of every
// trajectory, and the bound on x = sd^2 that a cap on the energy a contact can transfer implies.  The model is the tree kernels'
// (tpr_chain with a parent table; a serial chain is the tree parent = -1, 0, 1, ...), the points are the control-point kernels'
// (tpr_chain_points: up to 16 points fixed on any links).  M^-1 is never formed: one walk from the tips to the roots gives every g
// (the articulated-body factorisation M^-1 = (1 - H psi K)' D^-1 (1 - H psi K)), O(d) per gridpoint.
//
// The quantities, per gridpoint, qd = q'; all in link axes.  Spatial vectors are (angular; linear), a wrench's moment about its
// link's origin.  E_i, r_i: the link frame in its parent's (tpr_chain_rnea.hip.inc); z_i the joint axis; S_i = (z; 0) revolute,
// (0; z) prismatic.
//   way up     v_i = E_i' (v + w x r_i) + [prismatic] z qd_i,  w_i = E_i' w + [revolute] z qd_i        (the momentum kernel's)
//              point p at offset o_p on link k:  n_p = v_k + w_k x o_p
//              velocity mode   f = n_p,  s2_p = n_p . n_p          direction mode (u_p given, link axes)   f = u_p,  s2_p = (n_p . u_p)^2
//   way down   IA_i = I_i + sum over children c of X*(IA_c - U_c U_c' / D_c),   U_i = IA_i S_i,   D_i = S_i' U_i
//              I_i = [Ic + m (c.c 1 - c c'), m [c]x; (m [c]x)', m 1];   X* moves a spatial inertia into the parent's frame:
//              rotation by E_c, then the shift by r_c:  H + [r]x M,  J + [r]x H' + ([r]x H')' + ([r]x M) [r]x'
//              a point's bias wrench starts on its own link as b_p = (o_p x (-f); -f), g_p = 0; at every link i on its path to the root
//                u = -(S_i . b_p),  t = u (1 / D_i),  g_p = g_p + u t,  b_p = b_p + U_i t,  then b_p := (E b_ang + r x (E b_lin); E b_lin)
// so that g_p = sum over the path of u^2 / D_i.  One reciprocal per link (IEEE division), products by it elsewhere.  A robot whose
// mass matrix is singular (a weightless leaf: D = 0) gives non-finite results by IEEE rules: the caller's responsibility.
// The bound.  With limit = (2 E_max, 1 / m_body) of the point's trajectory and point:
//   winv = g_p / s2_p (velocity mode) | g_p (direction mode),   x_p = (limit_0 (limit_1 + winv)) / s2_p,   +inf where s2_p == 0
//   xbound = (0, min_p x_p):  best = +inf, then best = x_p < best ? x_p : best in the set's order.
//
// THE SUMMATION ORDER, fixed.  dot(a, b) = (a_x b_x + a_y b_y) + a_z b_z.  At link i, IA = ((carried + I_i) + bank): `carried` is
// what link i + 1 handed down when its parent is i (zero otherwise), `bank` the sum of the other children's, formed in the order the
// way down meets them -- descending link number, the first stored, each later one added with the bank on the left.  Links go in
// descending number.  A point's sums are its own: its bits depend neither on the other points of the set nor on its place in it.
// Every output passes through "+ 0.0".  Each output is computed whichever of the others is asked for.
//
// What is skipped, the same decision for every lane: a root's whole tree when it carries no point (both ways); on the way up the
// velocity of a link that no point hangs on (its sine and cosine are still kept: the way down needs every link of a walked tree).
// Which points are live at a link is a 16-bit word per link from the host, read by the loop index: wave-uniform branches.
//
// Shape: the family's.  One wave of 64 gridpoints per block; q, q' [64][d] pass through LDS (consecutive lanes on consecutive
// doubles, read back one row per lane at the odd pitch d | 1); a link's parameters come from scalar loads by the loop index, in two
// parts (the body's on the way down first, then the joint's); the joint type is a select.  IA is 21 doubles in registers.
// LDS, [slot][lane] (tpr_effmass_args.hpp): per link (sin q | q, cos q); per point its own 4 slots -- b_lin and s2 -- and 4 way-down
// slots -- b_ang and g -- that lie over the staged rows; per fork a bank of 21 (v, w on the way up).  Lanes past the last gridpoint
// of the batch work on the last one's row again; only npts rows leave.
#pragma once
#include "tpr_chain_rnea.hip.inc"
#include "tpr_effmass_args.hpp"

namespace tpr {

// The walk's tables, the points and the output pointers are read from the kernel's argument block where they are needed, behind an
// offset the compiler cannot see through (as the momentum kernel reads its): fetched up front they would sit in scalar registers
// across the loops, beside a link's parameters.
typedef const __attribute__((address_space(4))) char *EffMassArgBytes;
typedef const __attribute__((address_space(4))) double *EffMassWords;
typedef const __attribute__((address_space(4))) uint32_t *EffMassTable;
typedef const __attribute__((address_space(4))) EffMassArgs EffMassLate;
__device__ __forceinline__ EffMassArgBytes effmass_arg_bytes() {
    unsigned off = 0;
    asm("" : "+s"(off));
    return (EffMassArgBytes)__builtin_amdgcn_kernarg_segment_ptr() + off;
}
__device__ __forceinline__ int effmass_byte_at(EffMassTable t, int i) { return (int)(int8_t)(t[i >> 2] >> ((i & 3) * 8)); }
__device__ __forceinline__ unsigned effmass_half_at(EffMassTable t, int i) { return (t[i >> 1] >> ((i & 1) * 16)) & 0xffffu; }
// (a link mask is read as a table of one word, i < 32: the load stays where the bit is asked for)
__device__ __forceinline__ bool effmass_bit_at(EffMassTable t, int i) { return (t[i >> 5] >> (i & 31)) & 1u; }
static_assert(offsetof(EffMassArgs, T) % 4 == 0 && offsetof(TreeTables, parent) % 4 == 0 && offsetof(TreeTables, fork_slot) % 4 == 0 &&
                  offsetof(EffMassArgs, active) % 4 == 0 && offsetof(EffMassArgs, own) % 4 == 0 && offsetof(EffMassArgs, walk) % 4 == 0 &&
                  offsetof(TreeTables, running) % 4 == 0,
              "the tables start on a word");
static_assert(offsetof(EffMassArgs, P) % 8 == 0 && offsetof(ChainPoints, offset) % 8 == 0 && offsetof(EffMassArgs, direction) % 8 == 0,
              "the points' doubles are aligned");

// A symmetric 3 x 3 block and the spatial inertia [J, H; H', Mm] of an articulated body about its link's origin: 21 doubles.
struct EffSym { double xx, yy, zz, xy, xz, yz; };
struct EffInertia {
    EffSym J;
    M3 H;
    EffSym Mm;
};
__device__ __forceinline__ V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ V3 eff_row(const M3 &A, int r) { return {A.m[3 * r], A.m[3 * r + 1], A.m[3 * r + 2]}; }
__device__ __forceinline__ V3 eff_col(const EffSym &S, int c) {
    return c == 0 ? V3{S.xx, S.xy, S.xz} : c == 1 ? V3{S.xy, S.yy, S.yz} : V3{S.xz, S.yz, S.zz};
}
__device__ __forceinline__ double eff_at(V3 a, int k) { return k == 0 ? a.x : k == 1 ? a.y : a.z; }
__device__ __forceinline__ V3 eff_mul(const EffSym &S, V3 v) {
    return {S.xx * v.x + S.xy * v.y + S.xz * v.z, S.xy * v.x + S.yy * v.y + S.yz * v.z, S.xz * v.x + S.yz * v.y + S.zz * v.z};
}
__device__ __forceinline__ void eff_add(EffSym &a, const EffSym &b) {
    a.xx = a.xx + b.xx; a.yy = a.yy + b.yy; a.zz = a.zz + b.zz; a.xy = a.xy + b.xy; a.xz = a.xz + b.xz; a.yz = a.yz + b.yz;
}
// a - u w' on the upper triangle
__device__ __forceinline__ void eff_downdate(EffSym &a, V3 u, V3 w) {
    a.xx = a.xx - u.x * w.x; a.yy = a.yy - u.y * w.y; a.zz = a.zz - u.z * w.z;
    a.xy = a.xy - u.x * w.y; a.xz = a.xz - u.x * w.z; a.yz = a.yz - u.y * w.z;
}
// E S E': T = E S by rows (row r of T = S e_r, e_r = row r of E, S symmetric), then T E' on the upper triangle
__device__ __forceinline__ EffSym eff_rotate(const M3 &E, const EffSym &S) {
    const V3 e0 = eff_row(E, 0), e1 = eff_row(E, 1), e2 = eff_row(E, 2);
    const V3 t0 = eff_mul(S, e0), t1 = eff_mul(S, e1), t2 = eff_mul(S, e2);
    return {dot(t0, e0), dot(t1, e1), dot(t2, e2), dot(t0, e1), dot(t0, e2), dot(t1, e2)};
}
// E H E' for a general H: T = E H, then T E'
__device__ __forceinline__ M3 eff_rotate(const M3 &E, const M3 &H) {
    const M3 T = mul(E, H);
    M3 C;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C.m[3 * r + c] = dot(eff_row(T, r), eff_row(E, c));
    return C;
}
// X*: the spatial inertia `A` of a link, in its axes about its origin, as its parent sees it (the link frame: E, r).
__device__ __forceinline__ EffInertia eff_to_parent(const EffInertia &A, const M3 &E, V3 r) {
    const EffSym J = eff_rotate(E, A.J), Mm = eff_rotate(E, A.Mm);
    const M3 H = eff_rotate(E, A.H);
    // Q = [r]x Mm by columns, K = [r]x H' by columns (column c of H' is row c of H), and rows of Q [r]x' = r x (row j of Q)
    const V3 q0 = cross(r, eff_col(Mm, 0)), q1 = cross(r, eff_col(Mm, 1)), q2 = cross(r, eff_col(Mm, 2));
    const V3 k0 = cross(r, eff_row(H, 0)), k1 = cross(r, eff_row(H, 1)), k2 = cross(r, eff_row(H, 2));
    const V3 m0 = cross(r, V3{q0.x, q1.x, q2.x}), m1 = cross(r, V3{q0.y, q1.y, q2.y}), m2 = cross(r, V3{q0.z, q1.z, q2.z});
    EffInertia C;
    C.Mm = Mm;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        C.H.m[3 * j] = H.m[3 * j] + eff_at(q0, j); C.H.m[3 * j + 1] = H.m[3 * j + 1] + eff_at(q1, j); C.H.m[3 * j + 2] = H.m[3 * j + 2] + eff_at(q2, j);
    }
    // J_jk + K_jk + K_kj + (Q [r]x')_jk,  K_jk = k_k[j]
    C.J.xx = ((J.xx + k0.x) + k0.x) + m0.x;
    C.J.yy = ((J.yy + k1.y) + k1.y) + m1.y;
    C.J.zz = ((J.zz + k2.z) + k2.z) + m2.z;
    C.J.xy = ((J.xy + k1.x) + k0.y) + m0.y;
    C.J.xz = ((J.xz + k2.x) + k0.z) + m0.z;
    C.J.yz = ((J.yz + k2.y) + k1.z) + m1.z;
    return C;
}

// The block's rows [npts][d] of two arrays into LDS at `pitch`: (row, column) of element k advance without a division.
__device__ __forceinline__ void effmass_rows_load(double *b0, double *b1, const double *s0, const double *s1, size_t g0, int npts, int d, int pitch) {
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
// Slot `slot` of every point's group of four (`area`: [point][4][lane], lane 0) to dst [npts][count].
__device__ __forceinline__ void effmass_rows_store(const double *area, int slot, double *dst, size_t g0, int npts, int count) {
    for (int k = threadIdx.x; k < npts * count; k += kChainBlock) {
        const int r = k / count, p = k - r * count;
        dst[g0 * (size_t)count + k] = area[(4 * p + slot) * kChainBlock + r];
    }
}

static __global__ void __launch_bounds__(kChainBlock) effective_mass_kernel(EffMassArgs A) {
    extern __shared__ double effmass_lds[];
    const ChainModel &M = A.M;
    const int d = M.d, pitch = d | 1, count = A.P.count;
    const size_t g0 = (size_t)blockIdx.x * kChainBlock;
    const int left = A.npoints - (int)g0, npts = left < kChainBlock ? left : kChainBlock;
    // [link][2][lane] | [point][4][lane] own | [point][4][lane] way down, over the staged rows | [fork][21][lane]
    double *const own0 = effmass_lds + kEffMassLink * d * kChainBlock, *const down0 = own0 + kEffMassOwn * count * kChainBlock;
    double *const links = effmass_lds + threadIdx.x, *const own = own0 + threadIdx.x, *const down = down0 + threadIdx.x;
    double *const bq = down0, *const b1 = bq + kChainBlock * pitch;
    effmass_rows_load(bq, b1, A.q, A.qs, g0, npts, d, pitch);
    __syncthreads();
    const int lane = (int)threadIdx.x < npts ? (int)threadIdx.x : npts - 1, row = lane * pitch;
    ChainLaneBanks<kEffMassBank> Bk{down + effmass_shared_slots(d, count) * kChainBlock};
    const EffMassArgBytes late = effmass_arg_bytes();  // (one base for every late read: the offsets are immediates)
    const EffMassTable parents = (EffMassTable)(late + offsetof(EffMassArgs, T) + offsetof(TreeTables, parent));
    const EffMassTable slots = (EffMassTable)(late + offsetof(EffMassArgs, T) + offsetof(TreeTables, fork_slot));
    const EffMassTable actives = (EffMassTable)(late + offsetof(EffMassArgs, active));
    const EffMassTable owns = (EffMassTable)(late + offsetof(EffMassArgs, own));
    const EffMassWords offsets = (EffMassWords)(late + offsetof(EffMassArgs, P) + offsetof(ChainPoints, offset));
    const EffMassWords directions = (EffMassWords)(late + offsetof(EffMassArgs, direction));
    const EffMassTable walk = (EffMassTable)(late + offsetof(EffMassArgs, walk));
    const EffMassTable running = (EffMassTable)(late + offsetof(EffMassArgs, T) + offsetof(TreeTables, running));
    const EffMassTable forks = (EffMassTable)(late + offsetof(EffMassArgs, T) + offsetof(TreeTables, forks));
    const EffMassTable first = (EffMassTable)(late + offsetof(EffMassArgs, T) + offsetof(TreeTables, first));
    const bool directed = A.directed != 0;
    const V3 zero{0.0, 0.0, 0.0};

    // ---- the way up: (sin q | q, cos q) of every walked link; v, w along the paths to the points; the points' f and s2
    {
        V3 v = zero, w = zero;
#pragma nounroll
        for (int i = 0; i < d; ++i) {
            if (!effmass_bit_at(walk, i)) continue;  // (the same for every lane, as every branch of this loop)
            const ChainLink L = chain_link(M, i);  // (of it the joint's part alone is read: rot, trans, axis)
            const double qi = bq[row + i], qd = b1[row + i];
            double sq, cq;
            sincos(qi, &sq, &cq);
            const double sv = L.prismatic ? qi : sq;
            links[(kEffMassLink * i) * kChainBlock] = sv; links[(kEffMassLink * i + 1) * kChainBlock] = cq;
            if (effmass_half_at(actives, i) == 0) continue;
            if (!effmass_bit_at(running, i)) {
                const int par = effmass_byte_at(parents, i);
                if (par < 0) {
                    v = zero; w = zero;
                } else {
                    const int b = effmass_byte_at(slots, par);
                    v = Bk.get(b, 0); w = Bk.get(b, 3);
                }
            }
            const ChainJoint J = chain_joint(L, sv, cq);
            const V3 zr = L.prismatic ? zero : L.axis, zp = L.prismatic ? L.axis : zero;
            v = mul_t(J.E, v + cross(w, J.r)) + zp * qd;
            w = mul_t(J.E, w) + zr * qd;
            if (effmass_bit_at(forks, i)) {
                const int b = effmass_byte_at(slots, i);
                Bk.put(b, 0, v); Bk.put(b, 3, w);
            }
            const unsigned mine = effmass_half_at(owns, i);
#pragma nounroll
            for (int p = 0; p < count; ++p) {
                if (!((mine >> p) & 1u)) continue;
                const V3 o{offsets[3 * p], offsets[3 * p + 1], offsets[3 * p + 2]};
                const V3 u{directions[3 * p], directions[3 * p + 1], directions[3 * p + 2]};
                const V3 n = v + cross(w, o);
                const double along = dot(n, u);
                const V3 f = directed ? u : n;
                const double s2 = directed ? along * along : dot(n, n);
                double *const mo = own + (kEffMassOwn * p) * kChainBlock;
                mo[0] = -f.x; mo[kChainBlock] = -f.y; mo[2 * kChainBlock] = -f.z;
                mo[3 * kChainBlock] = s2 + 0.0;
            }
        }
    }
    __syncthreads();  // every lane has read its rows: the points' way-down slots take their place

    // ---- the way down: articulated inertias towards the roots, every live point's bias wrench and g along with them
    {
        EffInertia IA;
#pragma nounroll
        for (int i = d - 1; i >= 0; --i) {
            if (!effmass_bit_at(walk, i)) continue;
            if (!(i + 1 < d && effmass_bit_at(running, i + 1))) {  // link i + 1 is not this link's child: nothing is carried
                IA.J = EffSym{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; IA.Mm = IA.J;
#pragma unroll
                for (int k = 0; k < 9; ++k) IA.H.m[k] = 0.0;
            }
            {
                // The body's part of the link's parameters (mass, com, inertia: 10 doubles), by a link number the compiler cannot
                // tell from i: it is dead before the joint's part (rot, trans, axis: 15) is fetched.
                int ib = i;
                asm("" : "+s"(ib));
                const double mass = M.mass[ib];
                const V3 c = load3(M.com + 3 * ib);
                const double *const Ic = M.inertia + 6 * ib;
                const V3 mc = c * mass;
                IA.J.xx = IA.J.xx + (Ic[0] + (mc.y * c.y + mc.z * c.z));
                IA.J.yy = IA.J.yy + (Ic[1] + (mc.x * c.x + mc.z * c.z));
                IA.J.zz = IA.J.zz + (Ic[2] + (mc.x * c.x + mc.y * c.y));
                IA.J.xy = IA.J.xy + (Ic[3] - mc.x * c.y);
                IA.J.xz = IA.J.xz + (Ic[4] - mc.x * c.z);
                IA.J.yz = IA.J.yz + (Ic[5] - mc.y * c.z);
                // H = m [c]x
                IA.H.m[1] = IA.H.m[1] - mc.z; IA.H.m[2] = IA.H.m[2] + mc.y;
                IA.H.m[3] = IA.H.m[3] + mc.z; IA.H.m[5] = IA.H.m[5] - mc.x;
                IA.H.m[6] = IA.H.m[6] - mc.y; IA.H.m[7] = IA.H.m[7] + mc.x;
                IA.Mm.xx = IA.Mm.xx + mass; IA.Mm.yy = IA.Mm.yy + mass; IA.Mm.zz = IA.Mm.zz + mass;
            }
            if (effmass_bit_at(forks, i)) {
                const int b = effmass_byte_at(slots, i);
                EffInertia K;
                K.J = EffSym{Bk.at(b, 0), Bk.at(b, 1), Bk.at(b, 2), Bk.at(b, 3), Bk.at(b, 4), Bk.at(b, 5)};
#pragma unroll
                for (int k = 0; k < 9; ++k) K.H.m[k] = Bk.at(b, 6 + k);
                K.Mm = EffSym{Bk.at(b, 15), Bk.at(b, 16), Bk.at(b, 17), Bk.at(b, 18), Bk.at(b, 19), Bk.at(b, 20)};
                eff_add(IA.J, K.J); eff_add(IA.Mm, K.Mm);
#pragma unroll
                for (int k = 0; k < 9; ++k) IA.H.m[k] = IA.H.m[k] + K.H.m[k];
            }
            int ij = i;
            asm("" : "+s"(ij), "+v"(IA.Mm.xx));
            const ChainLink L = chain_link(M, ij);  // (the joint's part)
            const ChainJoint J = chain_joint(L, links[(kEffMassLink * i) * kChainBlock], links[(kEffMassLink * i + 1) * kChainBlock]);
            const V3 z = L.axis;
            // U = IA S: a column of IA weighted by z -- (J; H') z for a revolute joint, (H; Mm) z for a prismatic one
            const V3 Ua = L.prismatic ? mul(IA.H, z) : eff_mul(IA.J, z);
            const V3 Ul = L.prismatic ? eff_mul(IA.Mm, z) : mul_t(IA.H, z);
            const double D = dot(z, L.prismatic ? Ul : Ua), rinv = 1.0 / D;
            const unsigned act = effmass_half_at(actives, i), mine = effmass_half_at(owns, i);
#pragma nounroll
            for (int p = 0; p < count; ++p) {
                if (!((act >> p) & 1u)) continue;
                double *const mo = own + (kEffMassOwn * p) * kChainBlock, *const md = down + (kEffMassDown * p) * kChainBlock;
                V3 bl{mo[0], mo[kChainBlock], mo[2 * kChainBlock]}, ba;
                double g;
                if ((mine >> p) & 1u) {  // the point's own link: its wrench starts here
                    const V3 o{offsets[3 * p], offsets[3 * p + 1], offsets[3 * p + 2]};
                    ba = cross(o, bl);
                    g = 0.0;
                } else {
                    ba = V3{md[0], md[kChainBlock], md[2 * kChainBlock]};
                    g = md[3 * kChainBlock];
                }
                const double u = -dot(z, L.prismatic ? bl : ba), t = u * rinv;
                g = g + u * t;
                ba = ba + Ua * t; bl = bl + Ul * t;
                const V3 fl = mul(J.E, bl), fa = mul(J.E, ba) + cross(J.r, fl);
                mo[0] = fl.x; mo[kChainBlock] = fl.y; mo[2 * kChainBlock] = fl.z;
                md[0] = fa.x; md[kChainBlock] = fa.y; md[2 * kChainBlock] = fa.z;
                md[3 * kChainBlock] = g;
            }
            const int par = effmass_byte_at(parents, i);
            if (par < 0) continue;  // a root hands nothing down
            eff_downdate(IA.J, Ua, Ua * rinv); eff_downdate(IA.Mm, Ul, Ul * rinv);
            {
                const V3 w = Ul * rinv;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    IA.H.m[3 * r] = IA.H.m[3 * r] - eff_at(Ua, r) * w.x; IA.H.m[3 * r + 1] = IA.H.m[3 * r + 1] - eff_at(Ua, r) * w.y;
                    IA.H.m[3 * r + 2] = IA.H.m[3 * r + 2] - eff_at(Ua, r) * w.z;
                }
            }
            IA = eff_to_parent(IA, J.E, J.r);
            if (effmass_bit_at(running, i)) continue;  // the parent is the next link of the walk: carried in registers
            const int b = effmass_byte_at(slots, par);
            const double give[kEffMassBank] = {IA.J.xx, IA.J.yy, IA.J.zz, IA.J.xy, IA.J.xz, IA.J.yz, IA.H.m[0], IA.H.m[1], IA.H.m[2], IA.H.m[3],
                                               IA.H.m[4], IA.H.m[5], IA.H.m[6], IA.H.m[7], IA.H.m[8], IA.Mm.xx, IA.Mm.yy, IA.Mm.zz, IA.Mm.xy,
                                               IA.Mm.xz, IA.Mm.yz};
            if (effmass_bit_at(first, i)) {
#pragma unroll
                for (int k = 0; k < kEffMassBank; ++k) Bk.at(b, k) = give[k];
            } else {
#pragma unroll
                for (int k = 0; k < kEffMassBank; ++k) Bk.at(b, k) = Bk.at(b, k) + give[k];
            }
        }
    }

    // ---- the outputs.  Where they go, and the block's place in the batch and in the LDS, are read from the argument block and worked
    // out again here: held across the loops they are scalar registers the walks have no room for.
    const EffMassLate *out = (const EffMassLate *)late;
    double *const o_speed2 = out->speed2, *const o_mobility = out->mobility, *const o_xbound = out->xbound;
    unsigned block = blockIdx.x;
    asm("" : "+s"(block));
    const int dl = out->M.d, cl = out->P.count;
    const size_t gl = (size_t)block * kChainBlock;
    const int leftl = out->npoints - (int)gl, nl = leftl < kChainBlock ? leftl : kChainBlock;
    const int lanel = (int)threadIdx.x < nl ? (int)threadIdx.x : nl - 1;
    double *const ownl = effmass_lds + kEffMassLink * dl * kChainBlock, *const downl = ownl + kEffMassOwn * cl * kChainBlock;
    const double *lim = out->limit;
    if (o_xbound) lim += 2 * (size_t)cl * ((gl + (size_t)lanel) / (size_t)out->n1);
    double best = __builtin_inf();
#pragma nounroll
    for (int p = 0; p < cl; ++p) {
        double *const gs = downl + (kEffMassDown * p + 3) * kChainBlock + threadIdx.x;
        const double s2 = ownl[(kEffMassOwn * p + 3) * kChainBlock + threadIdx.x], g = *gs + 0.0;
        *gs = g;
        if (o_xbound) {  // (the same for every lane)
            const double winv = directed ? g : g / s2;
            const double x = (lim[2 * p] * (lim[2 * p + 1] + winv)) / s2;
            const double xs = s2 == 0.0 ? __builtin_inf() : x;
            best = xs < best ? xs : best;
        }
    }
    downl[threadIdx.x] = best;  // (point 0's first moment slot: dead)
    __syncthreads();
    if (o_speed2) effmass_rows_store(ownl, 3, o_speed2, gl, nl, cl);
    if (o_mobility) effmass_rows_store(downl, 3, o_mobility, gl, nl, cl);
    if (o_xbound)
        for (int k = threadIdx.x; k < 2 * nl; k += kChainBlock) o_xbound[2 * gl + k] = (k & 1) ? downl[k >> 1] : 0.0;
}

}  // namespace tpr

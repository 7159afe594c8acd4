// tpr_chain.hip.inc -- the kernels of a serial rigid-body chain evaluated at every gridpoint of every trajectory: inverse
// dynamics and the three evaluations of a torque constraint in one pass (the recursion is tpr_chain_rnea.hip.inc's), the tool
// point's velocity (CartesianVelocityNorm, constraint/cartesian_velocity_norm/pinocchio.hpp of the reference's C++ twin) and
// acceleration, the wrench on a carried body, speed and acceleration of control points on any link.
//
// Where the state lives.  1 .. 8 dof: the dof is a template parameter, both loops unroll, and a point's state is registers
// (327 registers at 7 dof for the fused kernel, 371 at 8: one wave per SIMD, no scratch).  A block is ONE wave of 64 consecutive
// points; their q, q', q'' [64][d] are contiguous in memory and pass through LDS -- loaded with consecutive lanes on
// consecutive doubles, read back one row per lane at pitch d | 1 -- and so do the outputs.  9 .. 32 dof: runtime dof, the
// state in LDS as [link][slot][lane] (conflict-free), d * slots * 512 bytes per block; the fused state fits 160 KB up to 18
// dof, above that the three evaluations run one after another in one launch.  Chain parameters are addressed by the loop
// index only: uniform loads.  The tool point's velocity and acceleration and the wrench on a carried body (at the end of this
// file) keep nothing per link: runtime dof, registers only, at any dof.
#pragma once
#include "tpr_chain_rnea.hip.inc"

namespace tpr {

// ---- staging a block's rows through LDS: the tool kernels below, and the base-reaction kernels (tpr_mount.hip.inc), which take
// this part of the file alone (TPR_CHAIN_STAGING_ONLY: a unit that saw the kernels below would carry a second copy of each) -----
// A block is one wave of 64 consecutive points.  Their q, q', q'' [64][d] are contiguous in memory and pass through LDS, as
// in the 1 .. 8-dof torque kernels but with a runtime d: loaded with consecutive lanes on consecutive doubles, read back one
// row per lane at the odd pitch d | 1 (conflict-free).  Read in place instead, a wave's rows -- 64 lanes x 3 arrays x d doubles,
// re-read link after link -- outgrow the caches from about 12 dof on and the lines come from memory again and again.  The
// 6-wide outputs leave through the same LDS at pitch 7.  Dynamic LDS: chain_accel_lds_bytes.
__host__ __device__ constexpr size_t chain_accel_lds_bytes(int d, int outputs) {
    const size_t in = 3 * (size_t)kChainBlock * (size_t)(d | 1), out = (size_t)outputs * kChainBlock * 7;
    return (in > out ? in : out) * sizeof(double);
}

// The block's rows [npts][d] of three arrays into LDS at `pitch`: (row, column) of element k advance without a division.
__device__ __forceinline__ void chain_rows_load(double *b0, double *b1, double *b2, const double *s0, const double *s1, const double *s2,
                                                size_t g0, int npts, int d, int pitch) {
    const size_t base = g0 * (size_t)d;
    const int step_r = kChainBlock / d, step_c = kChainBlock % d;
    int r = (int)threadIdx.x / d, c = (int)threadIdx.x % d;
    for (int k = threadIdx.x; k < npts * d; k += kChainBlock) {
        const int at = r * pitch + c;
        b0[at] = s0[base + k]; b1[at] = s1[base + k]; b2[at] = s2[base + k];
        r += step_r; c += step_c;
        if (c >= d) { c -= d; ++r; }
    }
}
// A block's q, q', q'' staged at the head of its LDS, and where this lane reads them: g0 = the block's first point, npts = its
// points, bq / b1 / b2 = the three areas, row = where this lane's row begins in each; lanes past the last point of the batch take
// the last point's lane.  Ends with the block in step: every row is in place.
struct ChainStage {
    size_t g0;
    int npts, lane, row;
    const double *bq, *b1, *b2;
};
__device__ __forceinline__ ChainStage chain_stage(double *lds, const double *s0, const double *s1, const double *s2, int npoints, int d) {
    const int pitch = d | 1;
    const size_t g0 = (size_t)blockIdx.x * kChainBlock;
    const int left = npoints - (int)g0, npts = left < kChainBlock ? left : kChainBlock;
    double *bq = lds, *b1 = bq + kChainBlock * pitch, *b2 = b1 + kChainBlock * pitch;
    chain_rows_load(bq, b1, b2, s0, s1, s2, g0, npts, d, pitch);
    __syncthreads();
    const int lane = (int)threadIdx.x < npts ? (int)threadIdx.x : npts - 1, row = lane * pitch;
    return {g0, npts, lane, row, bq, b1, b2};
}
// ... and a block's outputs [npts][6] from LDS at pitch 7.
__device__ __forceinline__ void chain_accel_rows_store(const double *buf, double *dst, size_t g0, int npts) {
    for (int k = threadIdx.x; k < npts * 6; k += kChainBlock) dst[g0 * 6 + k] = buf[(k / 6) * 7 + (k % 6)];
}

#ifndef TPR_CHAIN_STAGING_ONLY
// ---- 1 .. 8 dof: a block's 64 points through LDS, a point's state in registers ------------------------------------------
template <int D>
struct ChainTile {
    static constexpr int kPitch = D | 1;
    // consecutive lanes on consecutive doubles of the block's [npts][D] run
    static __device__ __forceinline__ void load(double *buf, const double *src, size_t g0, int npts) {
        for (int k = threadIdx.x; k < npts * D; k += kChainBlock) buf[(k / D) * kPitch + (k % D)] = src[g0 * D + k];
    }
    static __device__ __forceinline__ void store(const double *buf, double *dst, size_t g0, int npts) {
        for (int k = threadIdx.x; k < npts * D; k += kChainBlock) dst[g0 * D + k] = buf[(k / D) * kPitch + (k % D)];
    }
};

// Lanes past the last point of the batch work on the last point's row again (no divergence); only npts rows leave.
template <int D>
static __global__ void __launch_bounds__(kChainBlock) chain_inverse_dynamics_kernel(ChainDynArgs A) {
    using T = ChainTile<D>;
    __shared__ double buf[3][kChainBlock * T::kPitch];
    const size_t g0 = (size_t)blockIdx.x * kChainBlock;
    const int left = A.npoints - (int)g0, npts = left < kChainBlock ? left : kChainBlock;
    T::load(buf[0], A.q, g0, npts); T::load(buf[1], A.qd, g0, npts); T::load(buf[2], A.qdd, g0, npts);
    __syncthreads();
    const int row = ((int)threadIdx.x < npts ? (int)threadIdx.x : npts - 1) * T::kPitch;
    ChainRegState<D, kChainSlotsSingle> St;
    double tau[D];
    chain_rnea<D, false>(A.M, St, buf[0] + row, buf[1] + row, buf[2] + row, nullptr, nullptr, tau);
    __syncthreads();
    // (a lane past the end rewrites the last point's row with the last point's values: a store under a condition would draw
    // the whole backward pass into its branch, past the fences between the links)
#pragma unroll
    for (int i = 0; i < D; ++i) buf[0][row + i] = tau[i];
    __syncthreads();
    T::store(buf[0], A.tau, g0, npts);
}

template <int D>
static __global__ void __launch_bounds__(kChainBlock) chain_torque_terms_kernel(ChainTermsArgs A) {
    using T = ChainTile<D>;
    __shared__ double buf[3][kChainBlock * T::kPitch];
    const size_t g0 = (size_t)blockIdx.x * kChainBlock;
    const int left = A.npoints - (int)g0, npts = left < kChainBlock ? left : kChainBlock;
    T::load(buf[0], A.q, g0, npts); T::load(buf[1], A.qs, g0, npts); T::load(buf[2], A.qss, g0, npts);
    __syncthreads();
    const int row = ((int)threadIdx.x < npts ? (int)threadIdx.x : npts - 1) * T::kPitch;
    ChainRegState<D, kChainSlotsFused> St;
    double w0[D], wa[D], wb[D];
    chain_rnea<D, true>(A.M, St, buf[0] + row, buf[1] + row, buf[2] + row, w0, wa, wb);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < D; ++i) { buf[0][row + i] = w0[i]; buf[1][row + i] = wa[i]; buf[2][row + i] = wb[i]; }  // (as above)
    __syncthreads();
    T::store(buf[0], A.w0, g0, npts); T::store(buf[1], A.wa, g0, npts); T::store(buf[2], A.wb, g0, npts);
}

// ---- 9 .. 32 dof: runtime dof, a point's state in LDS, its rows read and written in place ----------------------------------
static __global__ void __launch_bounds__(kChainBlock) chain_inverse_dynamics_lds_kernel(ChainDynArgs A) {
    extern __shared__ double chain_lds[];
    const size_t at = chain_row(A.npoints, A.M.d);
    ChainLdsState<kChainSlotsSingle> St{chain_lds + threadIdx.x};
    chain_rnea<0, false>(A.M, St, A.q + at, A.qd + at, A.qdd + at, nullptr, nullptr, A.tau + at);
}

// FusedState: the 17 doubles per link fit the LDS (up to 18 dof); otherwise one evaluation after the other on 8.
template <bool FusedState>
static __global__ void __launch_bounds__(kChainBlock) chain_torque_terms_lds_kernel(ChainTermsArgs A) {
    extern __shared__ double chain_lds[];
    const size_t at = chain_row(A.npoints, A.M.d);
    if constexpr (FusedState) {
        ChainLdsState<kChainSlotsFused> St{chain_lds + threadIdx.x};
        chain_rnea<0, true>(A.M, St, A.q + at, A.qs + at, A.qss + at, A.w0 + at, A.wa + at, A.wb + at);
    } else {
        ChainLdsState<kChainSlotsSingle> St{chain_lds + threadIdx.x};
        chain_rnea<0, false>(A.M, St, A.q + at, nullptr, nullptr, nullptr, nullptr, A.w0 + at);
        chain_rnea<0, false>(A.M, St, A.q + at, nullptr, A.qs + at, nullptr, nullptr, A.wa + at);
        chain_rnea<0, false>(A.M, St, A.q + at, A.qs + at, A.qss + at, nullptr, nullptr, A.wb + at);
    }
}

// ---- the tool point's velocity: the forward recursion on velocities alone, any dof, registers only ---------------------
//   v_i = E_i' (v + w x r_i) + [prismatic] z qd_i,  w_i = E_i' w + [revolute] z qd_i,  W_i = W E_i (link axes in the world)
//   tool: W_d (v_d + w_d x tool), W_d w_d;  vSv = x' S x summed as sum_i x_i (sum_j S_ij x_j), or v . v without S.
static __global__ void __launch_bounds__(kChainBlock) chain_tool_velocity_kernel(ChainToolArgs A) {
    const ChainModel &M = A.M;
    const size_t g = (size_t)blockIdx.x * kChainBlock + threadIdx.x;
    const size_t p = g < (size_t)A.npoints ? g : (size_t)A.npoints - 1, at = p * (size_t)M.d;
    const V3 zero{0.0, 0.0, 0.0};
    V3 v = zero, w = zero;
    M3 W{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
#pragma nounroll
    for (int i = 0; i < M.d; ++i) {
        const ChainLink L = chain_link(M, i);
        const double qi = A.q[at + i], qd = A.qs[at + i];
        const ChainJoint J = chain_joint(L, L.prismatic ? qi : sin(qi), cos(qi));
        const V3 zr = L.prismatic ? zero : L.axis, zp = L.prismatic ? L.axis : zero;
        v = mul_t(J.E, v + cross(w, J.r)) + zp * qd;
        w = mul_t(J.E, w) + zr * qd;
        W = mul(W, J.E);
    }
    const V3 vw = mul(W, v + cross(w, load3(M.tool))), ww = mul(W, w);
    double vSv;
    if (A.S) {  // (the same for every lane)
        const double x[6] = {vw.x, vw.y, vw.z, ww.x, ww.y, ww.z};
        vSv = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double row = 0.0;
#pragma unroll
            for (int c = 0; c < 6; ++c) row = row + A.S[6 * r + c] * x[c];
            vSv = vSv + x[r] * row;
        }
    } else {
        vSv = dot(vw, vw);
    }
    // (a lane past the end repeats the last point's stores with the last point's values)
    if (A.vSv) A.vSv[p] = vSv;
    if (A.xbound) {
        A.xbound[2 * p] = 0.0;
        A.xbound[2 * p + 1] = A.limit[p / (size_t)A.n1] / vSv;
    }
}

// ---- the tool point's acceleration: the kinematic recursion with the base at rest, any dof, state in registers ------------
//   acc(q, qd, qdd) = [W_d (a_d + wd_d x tool + w_d x (w_d x tool)); W_d wd_d]: the classical (point) acceleration and the
//   angular acceleration, world axes; no gravity.  Per evaluation the state is (w, wd, a) of the current link, W is shared.
// Every output passes through "+ 0.0": a zero leaves as +0 whatever the signs of the vanishing products were, so the fused
// outputs equal the single evaluation's in every bit and acc(q, 0, 0) is the +0 a constraint's w0 is given as.
// How a block's rows pass through LDS (chain_accel_lds_bytes, chain_stage, chain_accel_rows_store) is at the head of this file.
template <int Level>
__device__ __forceinline__ void chain_tool_accel_put(const M3 &W, const ChainKin &K, V3 tool, double *o) {
    V3 al = K.a + cross(K.wd, tool);
    if (Level >= 2) al = al + cross(K.w, cross(K.w, tool));
    chain_put6(mul(W, al), mul(W, K.wd), o);
}

// Lanes past the last point of the batch work on the last point's row again and rewrite its LDS row with its values (no lane is
// masked out); only npts rows leave.
static __global__ void __launch_bounds__(kChainBlock) chain_tool_accel_kernel(ChainAccelArgs A) {
    extern __shared__ double chain_lds[];
    const ChainModel &M = A.M;
    const int d = M.d;
    const ChainStage B = chain_stage(chain_lds, A.q, A.qd, A.qdd, A.npoints, d);
    const V3 zero{0.0, 0.0, 0.0};
    ChainKin K{zero, zero, zero};
    M3 W{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
#pragma nounroll
    for (int i = 0; i < d; ++i) {
        const ChainLink L = chain_link(M, i);
        const double qi = B.bq[B.row + i];
        const ChainJoint J = chain_joint(L, L.prismatic ? qi : sin(qi), cos(qi));
        chain_kinematics<2>(L, J, K, B.b1[B.row + i], B.b2[B.row + i]);
        W = mul(W, J.E);
    }
    __syncthreads();
    chain_tool_accel_put<2>(W, K, load3(M.tool), chain_lds + B.lane * 7);
    __syncthreads();
    chain_accel_rows_store(chain_lds, A.acc, B.g0, B.npts);
}

// wa = acc(q, 0, qs), wb = acc(q, qs, qss) in one pass: level 1 leaves out the products with the zero velocity.
static __global__ void __launch_bounds__(kChainBlock) chain_tool_accel_terms_kernel(ChainAccelTermsArgs A) {
    extern __shared__ double chain_lds[];
    const ChainModel &M = A.M;
    const int d = M.d;
    const ChainStage B = chain_stage(chain_lds, A.q, A.qs, A.qss, A.npoints, d);
    const V3 zero{0.0, 0.0, 0.0};
    ChainKin K1{zero, zero, zero}, K2 = K1;
    M3 W{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
#pragma nounroll
    for (int i = 0; i < d; ++i) {
        const ChainLink L = chain_link(M, i);
        const double qi = B.bq[B.row + i], v1 = B.b1[B.row + i], v2 = B.b2[B.row + i];
        const ChainJoint J = chain_joint(L, L.prismatic ? qi : sin(qi), cos(qi));
        chain_kinematics<1>(L, J, K1, 0.0, v1);
        chain_kinematics<2>(L, J, K2, v1, v2);
        W = mul(W, J.E);
    }
    const V3 tool = load3(M.tool);
    double *oa = chain_lds, *ob = chain_lds + kChainBlock * 7;
    __syncthreads();
    chain_tool_accel_put<1>(W, K1, tool, oa + B.lane * 7);
    chain_tool_accel_put<2>(W, K2, tool, ob + B.lane * 7);
    __syncthreads();
    chain_accel_rows_store(oa, A.wa, B.g0, B.npts);
    chain_accel_rows_store(ob, A.wb, B.g0, B.npts);
}

// ---- the wrench at the tool: what the last link transmits to a body it carries, any dof, state in registers -------------------
//   With (w, wd, a) of the last link in its own frame, from the recursion started at a = -gravity (as chain_rnea starts it), the
//   payload's mass m, centre of mass c, inertia I about c (link axes), contact frame Rc (columns: its axes in link coordinates)
//   and that frame's origin p:
//     Fl = m (a + wd x c + w x (w x c)),  Nl = I wd + w x (I w),  wrench = [Rc' Fl; Rc' (Nl + (c - p) x Fl)]
//   the force on the body and its moment about p, contact-frame axes; gravity included.  The result is in link axes, so the
//   accumulated world rotation W is never formed.  The levels drop the products with an exact zero as chain_forward does and
//   every output passes through "+ 0.0", so the fused outputs equal the single evaluation's in every bit, and a massless,
//   inertia-less payload gives +0.  Staging and launch shape are the tool-acceleration kernels'; the payload comes by value.
// The payload's 22 doubles are read from the kernel's argument block AFTER the loop over the links, behind an offset the
// compiler cannot see through: fetched up front (where it moves loads of arguments to by itself) they sit in 44 scalar
// registers across the loop, beside a link's parameters, and spill.  mass, com[3], inertia[6], rot[9], origin[3] in this order.
typedef const __attribute__((address_space(4))) double *ChainPayloadWords;
template <class Args>
__device__ __forceinline__ ChainPayloadWords chain_payload_words() {
    static_assert(sizeof(ChainPayload) == 22 * sizeof(double), "the payload is 22 packed doubles");
    unsigned off = (unsigned)offsetof(Args, P);
    asm volatile("" : "+s"(off));
    return (ChainPayloadWords)((const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() + off);
}
__device__ __forceinline__ V3 payload_inertia_mul(ChainPayloadWords I, V3 w) {  // I = xx, yy, zz, xy, xz, yz
    return {I[0] * w.x + I[3] * w.y + I[4] * w.z, I[3] * w.x + I[1] * w.y + I[5] * w.z, I[4] * w.x + I[5] * w.y + I[2] * w.z};
}

template <int Level>
__device__ __forceinline__ void chain_tool_wrench_put(ChainPayloadWords P, const ChainKin &K, double *o) {
    const double mass = P[0];
    const V3 c{P[1], P[2], P[3]}, arm{P[1] - P[19], P[2] - P[20], P[3] - P[21]};
    M3 Rc;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rc.m[k] = P[10 + k];
    V3 ac = K.a;
    if (Level >= 1) ac = ac + cross(K.wd, c);
    if (Level >= 2) ac = ac + cross(K.w, cross(K.w, c));
    const V3 Fl = ac * mass;
    V3 n = cross(arm, Fl);
    if (Level >= 1) {
        V3 Nl = payload_inertia_mul(P + 4, K.wd);
        if (Level >= 2) Nl = Nl + cross(K.w, payload_inertia_mul(P + 4, K.w));
        n = Nl + n;
    }
    chain_put6(mul_t(Rc, Fl), mul_t(Rc, n), o);
}

// Lanes past the last point of the batch work on the last point's row again and rewrite its LDS row with its values (no lane is
// masked out); only npts rows leave.
static __global__ void __launch_bounds__(kChainBlock) chain_tool_wrench_kernel(ChainWrenchArgs A) {
    extern __shared__ double chain_lds[];
    const ChainModel &M = A.M;
    const int d = M.d;
    const ChainStage B = chain_stage(chain_lds, A.q, A.qd, A.qdd, A.npoints, d);
    const V3 g = load3(M.gravity), zero{0.0, 0.0, 0.0};
    ChainKin K{zero, zero, {-g.x, -g.y, -g.z}};
#pragma nounroll
    for (int i = 0; i < d; ++i) {
        const ChainLink L = chain_link(M, i);
        const double qi = B.bq[B.row + i];
        const ChainJoint J = chain_joint(L, L.prismatic ? qi : sin(qi), cos(qi));
        chain_kinematics<2>(L, J, K, B.b1[B.row + i], B.b2[B.row + i]);
    }
    __syncthreads();
    chain_tool_wrench_put<2>(chain_payload_words<ChainWrenchArgs>(), K, chain_lds + B.lane * 7);
    __syncthreads();
    chain_accel_rows_store(chain_lds, A.wrench, B.g0, B.npts);
}

// w0 = wrench(q, 0, 0), wa = wrench(q, 0, qs), wb = wrench(q, qs, qss) in one pass over the links.
static __global__ void __launch_bounds__(kChainBlock) chain_tool_wrench_terms_kernel(ChainWrenchTermsArgs A) {
    extern __shared__ double chain_lds[];
    const ChainModel &M = A.M;
    const int d = M.d;
    const ChainStage B = chain_stage(chain_lds, A.q, A.qs, A.qss, A.npoints, d);
    const V3 g = load3(M.gravity), zero{0.0, 0.0, 0.0};
    ChainKin K0{zero, zero, {-g.x, -g.y, -g.z}}, K1 = K0, K2 = K0;
#pragma nounroll
    for (int i = 0; i < d; ++i) {
        const ChainLink L = chain_link(M, i);
        const double qi = B.bq[B.row + i], v1 = B.b1[B.row + i], v2 = B.b2[B.row + i];
        const ChainJoint J = chain_joint(L, L.prismatic ? qi : sin(qi), cos(qi));
        chain_kinematics<0>(L, J, K0, 0.0, 0.0);
        chain_kinematics<1>(L, J, K1, 0.0, v1);
        chain_kinematics<2>(L, J, K2, v1, v2);
    }
    double *o0 = chain_lds, *oa = o0 + kChainBlock * 7, *ob = oa + kChainBlock * 7;
    __syncthreads();
    const ChainPayloadWords P = chain_payload_words<ChainWrenchTermsArgs>();
    chain_tool_wrench_put<0>(P, K0, o0 + B.lane * 7);
    chain_tool_wrench_put<1>(P, K1, oa + B.lane * 7);
    chain_tool_wrench_put<2>(P, K2, ob + B.lane * 7);
    __syncthreads();
    chain_accel_rows_store(o0, A.w0, B.g0, B.npts);
    chain_accel_rows_store(oa, A.wa, B.g0, B.npts);
    chain_accel_rows_store(ob, A.wb, B.g0, B.npts);
}

// ---- control points on any link: speed and linear acceleration of up to 16 points in one pass over the links -------------------
//   A point p is fixed in the frame of link[p] at offset[p].  The recursions are the tool kernels' (velocity: v, w, W; acceleration:
//   chain_kinematics<Level>, base at rest, no gravity); after link i is updated every point that sits on it reads the link's state
//   with the tool kernels' own expressions in their order, so a point (k, r) gives the bits of the tool kernel on the chain cut
//   after link k with tool = r.  The loop over the links ends after the deepest link that carries a point (nlinks, found by the
//   host).  The set comes by value and is the same for every lane: "does point p sit on link i" is a scalar compare.  Its words are
//   read from the kernel's argument block behind an offset the compiler cannot see through (as the payload's are), by the running
//   index p: nothing of the set is held in registers across the links.
typedef const __attribute__((address_space(4))) int32_t *ChainPointLinks;
template <class Args>
__device__ __forceinline__ ChainPointLinks chain_point_links() {
    unsigned off = (unsigned)(offsetof(Args, P) + offsetof(ChainPoints, link));
    asm volatile("" : "+s"(off));
    return (ChainPointLinks)((const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() + off);
}
template <class Args>
__device__ __forceinline__ ChainPayloadWords chain_point_offsets() {
    unsigned off = (unsigned)(offsetof(Args, P) + offsetof(ChainPoints, offset));
    asm volatile("" : "+s"(off));
    return (ChainPayloadWords)((const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr() + off);
}

// speed2 [npoints][count] = |velocity of point p|^2 for qd = qs; xbound [npoints][2] = (0, min_p limit[b][p] / speed2_p): an IEEE
// division, so a point that stands still gives +inf and drops out of the minimum.  q, qs are read in place, as the tool kernel reads.
static __global__ void __launch_bounds__(kChainBlock) chain_points_speed_kernel(ChainPointsSpeedArgs A) {
    const ChainModel &M = A.M;
    const ChainPointLinks links = chain_point_links<ChainPointsSpeedArgs>();
    const ChainPayloadWords offsets = chain_point_offsets<ChainPointsSpeedArgs>();
    const int count = A.P.count;
    const size_t g = (size_t)blockIdx.x * kChainBlock + threadIdx.x;
    const size_t pt = g < (size_t)A.npoints ? g : (size_t)A.npoints - 1, at = pt * (size_t)M.d;
    const size_t out = pt * (size_t)count, lim = (pt / (size_t)A.n1) * (size_t)count;
    const V3 zero{0.0, 0.0, 0.0};
    V3 v = zero, w = zero;
    M3 W{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
    double best = __builtin_huge_val();
#pragma nounroll
    for (int i = 0; i < A.nlinks; ++i) {
        const ChainLink L = chain_link(M, i);
        const double qi = A.q[at + i], qd = A.qs[at + i];
        const ChainJoint J = chain_joint(L, L.prismatic ? qi : sin(qi), cos(qi));
        const V3 zr = L.prismatic ? zero : L.axis, zp = L.prismatic ? L.axis : zero;
        v = mul_t(J.E, v + cross(w, J.r)) + zp * qd;
        w = mul_t(J.E, w) + zr * qd;
        W = mul(W, J.E);
#pragma nounroll
        for (int p = 0; p < count; ++p) {
            if (links[p] != i) continue;  // (the same for every lane)
            const V3 vw = mul(W, v + cross(w, V3{offsets[3 * p], offsets[3 * p + 1], offsets[3 * p + 2]}));
            const double s = dot(vw, vw);
            // (a lane past the end repeats the last point's stores with the last point's values)
            if (A.speed2) A.speed2[out + p] = s;
            if (A.xbound) {
                const double x = A.limit[lim + p] / s;
                best = x < best ? x : best;
            }
        }
    }
    if (A.xbound) {
        A.xbound[2 * pt] = 0.0;
        A.xbound[2 * pt + 1] = best;
    }
}

// The acceleration kernels stage a block's q, q', q'' through LDS as the tool kernels do -- loaded with consecutive lanes on
// consecutive doubles of a row's part, read back one row per lane -- but kChainPointsChunk = 3 links at a time, at pitch 3 (odd:
// conflict-free), and keep the block's outputs [64][3 count] in LDS at the odd pitch 3 count | 1 BESIDE them until the links are
// done, so that the global stores are contiguous.  The two areas cannot share their space as the tool kernels' do: a point's
// output exists from its link on, while the inputs of the deeper links are still to be read -- with 16 points on link 0 of a
// 32-dof chain that is 96 + 93 columns of 64 doubles at once, more than either area.  Staging few links at a time keeps the sum
// small, and that is what the kernels' speed hangs on: a block's LDS bounds the waves a CU holds, and the recursion's latencies
// want many.  Measured (65 536 x 201 points, 4 points, 7 / 12 / 20 dof, fused kernel): every link staged at once 2.70 / 5.55 /
// 10.9 ms, 7 links 2.73 / 4.24 / 6.43, 5 links 2.46 / 3.79 / 6.10, 3 links 2.16 / 3.46 / 6.02, 1 link 2.17 / 5.23 / 13.6 (8-byte
// pieces of a row per load).  At most 4 608 + 2 * 64 * 49 * 8 = 54 784 bytes: under the 64 KB any launch may take.
__host__ __device__ constexpr size_t chain_points_lds_bytes(int count, int outputs) {
    return (3 * (size_t)kChainBlock * (size_t)kChainPointsChunk + (size_t)outputs * kChainBlock * (size_t)(3 * count | 1)) * sizeof(double);
}
static_assert(kChainPointsChunk % 2 == 1, "the staging pitch is the chunk itself: odd, or the rows' reads conflict");

// Columns [c0, c0 + nc) of the block's rows [npts][d] of three arrays into LDS at `pitch`: chain_rows_load for a part of the row.
__device__ __forceinline__ void chain_cols_load(double *b0, double *b1, double *b2, const double *s0, const double *s1, const double *s2,
                                                size_t g0, int npts, int d, int c0, int nc, int pitch) {
    const size_t base = g0 * (size_t)d + (size_t)c0;
    const int step_r = kChainBlock / nc, step_c = kChainBlock % nc;
    int r = (int)threadIdx.x / nc, c = (int)threadIdx.x % nc;
    for (int k = threadIdx.x; k < npts * nc; k += kChainBlock) {
        const int at = r * pitch + c;
        const size_t from = base + (size_t)r * (size_t)d + (size_t)c;
        b0[at] = s0[from]; b1[at] = s1[from]; b2[at] = s2[from];
        r += step_r; c += step_c;
        if (c >= nc) { c -= nc; ++r; }
    }
}
// ... and a block's outputs [npts][n] from LDS at `pitch`.
__device__ __forceinline__ void chain_points_rows_store(const double *buf, double *dst, size_t g0, int npts, int n, int pitch) {
    const size_t base = g0 * (size_t)n;
    const int step_r = kChainBlock / n, step_c = kChainBlock % n;
    int r = (int)threadIdx.x / n, c = (int)threadIdx.x % n;
    for (int k = threadIdx.x; k < npts * n; k += kChainBlock) {
        dst[base + k] = buf[r * pitch + c];
        r += step_r; c += step_c;
        if (c >= n) { c -= n; ++r; }
    }
}

// The linear three of chain_tool_accel_put, in its order.
template <int Level>
__device__ __forceinline__ void chain_point_accel_put(const M3 &W, const ChainKin &K, V3 at, double *o) {
    V3 al = K.a + cross(K.wd, at);
    if (Level >= 2) al = al + cross(K.w, cross(K.w, at));
    const V3 lin = mul(W, al);
    o[0] = lin.x + 0.0; o[1] = lin.y + 0.0; o[2] = lin.z + 0.0;
}

// Terms: wa = acc(q, 0, v1) and acc = acc(q, v1, v2) in one pass; otherwise acc alone.  Lanes past the last point of the batch work
// on the last point's row again and rewrite its LDS row with its values (no lane is masked out); only npts rows leave.
template <bool Terms>
__device__ __forceinline__ void chain_points_accel(const ChainPointsAccelArgs &A) {
    extern __shared__ double chain_lds[];
    const ChainModel &M = A.M;
    const ChainPointLinks links = chain_point_links<ChainPointsAccelArgs>();
    const ChainPayloadWords offsets = chain_point_offsets<ChainPointsAccelArgs>();
    constexpr int chunk = kChainPointsChunk, pitch = kChainPointsChunk;
    const int d = M.d, count = A.P.count, width = 3 * count, opitch = width | 1;
    const size_t g0 = (size_t)blockIdx.x * kChainBlock;
    const int left = A.npoints - (int)g0, npts = left < kChainBlock ? left : kChainBlock;
    double *bq = chain_lds, *b1 = bq + kChainBlock * pitch, *b2 = b1 + kChainBlock * pitch;
    double *ob = b2 + kChainBlock * pitch, *oa = ob + kChainBlock * opitch;  // (oa: Terms only)
    const int lane = (int)threadIdx.x < npts ? (int)threadIdx.x : npts - 1, row = lane * pitch, orow = lane * opitch;
    const V3 zero{0.0, 0.0, 0.0};
    ChainKin K1{zero, zero, zero}, K2 = K1;
    M3 W{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
#pragma nounroll
    for (int c0 = 0; c0 < A.nlinks; c0 += chunk) {
        const int nc = A.nlinks - c0 < chunk ? A.nlinks - c0 : chunk;
        if (c0 > 0) __syncthreads();  // every lane has read its row of the links before
        chain_cols_load(bq, b1, b2, A.q, A.v1, A.v2, g0, npts, d, c0, nc, pitch);
        __syncthreads();
#pragma nounroll
        for (int j = 0; j < nc; ++j) {
            const int i = c0 + j;
            const ChainLink L = chain_link(M, i);
            const double qi = bq[row + j], v1 = b1[row + j], v2 = b2[row + j];
            const ChainJoint J = chain_joint(L, L.prismatic ? qi : sin(qi), cos(qi));
            if (Terms) chain_kinematics<1>(L, J, K1, 0.0, v1);
            chain_kinematics<2>(L, J, K2, v1, v2);
            W = mul(W, J.E);
#pragma nounroll
            for (int p = 0; p < count; ++p) {
                if (links[p] != i) continue;  // (the same for every lane)
                const V3 at{offsets[3 * p], offsets[3 * p + 1], offsets[3 * p + 2]};
                if (Terms) chain_point_accel_put<1>(W, K1, at, oa + orow + 3 * p);
                chain_point_accel_put<2>(W, K2, at, ob + orow + 3 * p);
            }
        }
    }
    __syncthreads();
    if (Terms) chain_points_rows_store(oa, A.wa, g0, npts, width, opitch);
    chain_points_rows_store(ob, A.acc, g0, npts, width, opitch);
}

static __global__ void __launch_bounds__(kChainBlock) chain_points_accel_kernel(ChainPointsAccelArgs A) { chain_points_accel<false>(A); }
static __global__ void __launch_bounds__(kChainBlock) chain_points_accel_terms_kernel(ChainPointsAccelArgs A) { chain_points_accel<true>(A); }

#endif  // TPR_CHAIN_STAGING_ONLY

}  // namespace tpr

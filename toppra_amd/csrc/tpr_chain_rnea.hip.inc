// tpr_chain_rnea.hip.inc -- the recursive Newton-Euler recursion of a rigid-body chain, one link at a time: what the chain
// kernels (tpr_chain.hip.inc) and the tree kernels (tpr_tree.hip.inc) are both written on.  Device functions only, no kernel:
// recursive Newton-Euler inverse dynamics is what JointTorqueConstraint's inv_dyn callback computes, and what the reference's
// C++ twin takes from pinocchio (cpp/src/toppra/constraint/joint_torque/pinocchio.hpp).  The model is the one of
// include/toppra_hip.h (tpr_chain).
//
// The recursion, in link-local frames.  E_i = rot_i R(axis_i, q_i) (R = identity for a prismatic joint) has the link frame's
// axes in parent coordinates as columns, r_i = trans_i + rot_i axis_i q_i [prismatic] is its origin there.  With the
// parent's angular velocity w, angular acceleration wd and origin acceleration a (base: 0, 0, -gravity), z = axis_i:
//   forward    a_i  = E_i' (a + wd x r_i + w x (w x r_i))                 + [prismatic] (z qdd_i + 2 (E_i' w) x z qd_i)
//              w_i  = E_i' w                                              + [revolute]  z qd_i
//              wd_i = E_i' wd                                             + [revolute]  (z qdd_i + (E_i' w) x z qd_i)
//              F_i  = m_i (a_i + wd_i x c_i + w_i x (w_i x c_i)),  N_i = I_i wd_i + w_i x (I_i w_i)
//   backward   f_i  = F_i + fc,  n_i = N_i + c_i x F_i + nc   with the child's  fc = E f,  nc = E n + r x fc  (0 at the tip)
//              tau_i = z . n_i [revolute],  z . f_i [prismatic]
// The joint type enters as selects on a wave-uniform bit, never as a branch around arithmetic.  The backward pass needs F_i,
// N_i of every link and rebuilds E_i, r_i from the kept (sin q_i | q_i, cos q_i): 8 doubles per link and evaluation.
//
// Three evaluations in one pass (chain_rnea<D, true>): tau(q, 0, 0), tau(q, 0, q'), tau(q, q', q'') share the sines,
// cosines, E_i and r_i.  The first two are the same recursion with the products by an exact zero left out (level 0: no
// velocity, no acceleration -- N_i = 0 is not even kept; level 1: no velocity); every remaining sum keeps its order, so each
// output equals the single evaluation of level 2 on the same arguments (a zero's sign apart).  17 doubles per link.
#pragma once
#include "tpr_device.hpp"
#include "tpr_chain_args.hpp"

namespace tpr {

struct V3 { double x, y, z; };
struct M3 { double m[9]; };  // row-major

__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 mul(const M3 &A, V3 v) {
    return {A.m[0] * v.x + A.m[1] * v.y + A.m[2] * v.z, A.m[3] * v.x + A.m[4] * v.y + A.m[5] * v.z, A.m[6] * v.x + A.m[7] * v.y + A.m[8] * v.z};
}
__device__ __forceinline__ V3 mul_t(const M3 &A, V3 v) {  // A' v
    return {A.m[0] * v.x + A.m[3] * v.y + A.m[6] * v.z, A.m[1] * v.x + A.m[4] * v.y + A.m[7] * v.z, A.m[2] * v.x + A.m[5] * v.y + A.m[8] * v.z};
}
__device__ __forceinline__ M3 mul(const M3 &A, const M3 &B) {
    M3 C;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C.m[3 * r + c] = A.m[3 * r] * B.m[c] + A.m[3 * r + 1] * B.m[3 + c] + A.m[3 * r + 2] * B.m[6 + c];
    return C;
}

// One link's parameters: the same for every lane.
struct ChainLink {
    M3 rot;
    V3 trans, axis, com;
    double mass, I[6];
    bool prismatic;
};
__device__ __forceinline__ V3 load3(const double *p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ ChainLink chain_link(const ChainModel &M, int i) {
    ChainLink L;
#pragma unroll
    for (int k = 0; k < 9; ++k) L.rot.m[k] = M.rot[9 * i + k];
    L.trans = load3(M.trans + 3 * i); L.axis = load3(M.axis + 3 * i); L.com = load3(M.com + 3 * i);
    L.mass = M.mass[i];
#pragma unroll
    for (int k = 0; k < 6; ++k) L.I[k] = M.inertia[6 * i + k];
    L.prismatic = (M.prismatic >> i) & 1u;
    return L;
}
__device__ __forceinline__ V3 inertia_mul(const ChainLink &L, V3 w) {  // I = xx, yy, zz, xy, xz, yz
    return {L.I[0] * w.x + L.I[3] * w.y + L.I[4] * w.z, L.I[3] * w.x + L.I[1] * w.y + L.I[5] * w.z, L.I[4] * w.x + L.I[5] * w.y + L.I[2] * w.z};
}

// The link frame in its parent's, from the kept pair sv = sin q (revolute) | q (prismatic), cv = cos q.
struct ChainJoint {
    M3 E;
    V3 r;
};
__device__ __forceinline__ ChainJoint chain_joint(const ChainLink &L, double sv, double cv) {
    const double s = L.prismatic ? 0.0 : sv, c = L.prismatic ? 1.0 : cv, t = 1.0 - c, slide = L.prismatic ? sv : 0.0;
    const V3 k = L.axis;
    const double txy = t * k.x * k.y, txz = t * k.x * k.z, tyz = t * k.y * k.z;
    M3 R;  // Rodrigues: c I + s [k]x + (1 - c) k k'
    R.m[0] = t * k.x * k.x + c; R.m[1] = txy - s * k.z;     R.m[2] = txz + s * k.y;
    R.m[3] = txy + s * k.z;     R.m[4] = t * k.y * k.y + c; R.m[5] = tyz - s * k.x;
    R.m[6] = txz - s * k.y;     R.m[7] = tyz + s * k.x;     R.m[8] = t * k.z * k.z + c;
    ChainJoint J;
    J.E = mul(L.rot, R);
    J.r = L.trans + mul(L.rot, k * slide);
    return J;
}

struct ChainKin { V3 w, wd, a; };  // a link's angular velocity, angular acceleration, origin acceleration, in its own frame

// Level 2: the recursion.  Level 1: velocity zero, its products left out.  Level 0: acceleration zero as well.
// The kinematic part (the tool point's acceleration needs nothing else): the parent's K becomes this link's.
template <int Level>
__device__ __forceinline__ void chain_kinematics(const ChainLink &L, const ChainJoint &J, ChainKin &K, double qd, double qdd) {
    const V3 zero{0.0, 0.0, 0.0};
    const V3 zr = L.prismatic ? zero : L.axis, zp = L.prismatic ? L.axis : zero;
    V3 ar = K.a;
    if (Level >= 1) ar = ar + cross(K.wd, J.r);
    if (Level >= 2) ar = ar + cross(K.w, cross(K.w, J.r));
    V3 a = mul_t(J.E, ar), w = zero, wd = zero;
    if (Level >= 1) {
        wd = mul_t(J.E, K.wd) + zr * qdd;
        a = a + zp * qdd;
    }
    if (Level >= 2) {
        const V3 wl = mul_t(J.E, K.w);
        w = wl + zr * qd;
        wd = wd + cross(wl, zr) * qd;
        a = a + cross(wl, zp) * (2.0 * qd);
    }
    K.w = w; K.wd = wd; K.a = a;
}

template <int Level>
__device__ __forceinline__ void chain_forward(const ChainLink &L, const ChainJoint &J, ChainKin &K, double qd, double qdd, V3 &F, V3 &Nm) {
    const V3 zero{0.0, 0.0, 0.0};
    chain_kinematics<Level>(L, J, K, qd, qdd);
    const V3 w = K.w, wd = K.wd, a = K.a;
    V3 ac = a;
    if (Level >= 1) ac = ac + cross(wd, L.com);
    if (Level >= 2) ac = ac + cross(w, cross(w, L.com));
    F = ac * L.mass;
    Nm = zero;
    if (Level >= 1) Nm = inertia_mul(L, wd);
    if (Level >= 2) Nm = Nm + cross(w, inertia_mul(L, w));
}

struct ChainWrench { V3 f, n; };  // the child's force and moment in this link's frame, the moment about this link's origin

template <int Level>
__device__ __forceinline__ double chain_backward(const ChainLink &L, const ChainJoint &J, V3 F, V3 Nm, ChainWrench &C) {
    const V3 f = F + C.f;
    V3 n = cross(L.com, F);
    if (Level >= 1) n = Nm + n;
    n = n + C.n;
    const double tr = dot(L.axis, n), tp = dot(L.axis, f);
    C.f = mul(J.E, f);
    C.n = mul(J.E, n) + cross(J.r, C.f);
    return L.prismatic ? tp : tr;
}

// chain_backward's sibling for what wants the whole wrench and not its projection on the joint axis (tpr_joint.hip.inc): f, n =
// the force ON link i through joint i and its moment about link i's origin, link axes -- the very sums chain_backward forms, in
// its order; C becomes what link i hands to its parent, as there.
template <int Level>
__device__ __forceinline__ void chain_backward_wrench(const ChainLink &L, const ChainJoint &J, V3 F, V3 Nm, ChainWrench &C, V3 &f, V3 &n) {
    f = F + C.f;
    n = cross(L.com, F);
    if (Level >= 1) n = Nm + n;
    n = n + C.n;
    C.f = mul(J.E, f);
    C.n = mul(J.E, n) + cross(J.r, C.f);
}

// A point's per-link state: registers (compile-time dof, constant indices after unrolling) or LDS [link][slot][lane].
template <int D, int Slots>
struct ChainRegState {
    double v[D][Slots];
    __device__ __forceinline__ double &at(int i, int s) { return v[i][s]; }
};
template <int Slots>
struct ChainLdsState {
    double *base;  // this lane's first slot
    __device__ __forceinline__ double &at(int i, int s) { return base[(i * Slots + s) * kChainBlock]; }
};
__device__ __forceinline__ void chain_put(V3 v, double &a, double &b, double &c) { a = v.x; b = v.y; c = v.z; }
// A lane's banks in LDS, [bank][slot][lane] -- ChainLdsState's layout -- read and written three doubles at a time: what the tree and
// joint-load kernels (TreeBanks) and the base-reaction kernels (MountBanks) keep a fork's state in.
template <int Doubles>
struct ChainLaneBanks : ChainLdsState<Doubles> {
    using ChainLdsState<Doubles>::at;
    __device__ __forceinline__ V3 get(int b, int s) { return {at(b, s), at(b, s + 1), at(b, s + 2)}; }
    __device__ __forceinline__ void put(int b, int s, V3 v) { at(b, s) = v.x; at(b, s + 1) = v.y; at(b, s + 2) = v.z; }
};
// Six outputs, each through "+ 0.0": a zero leaves as +0 whatever the signs of the vanishing products were.
__device__ __forceinline__ void chain_put6(V3 a, V3 b, double *o) {
    o[0] = a.x + 0.0; o[1] = a.y + 0.0; o[2] = a.z + 0.0;
    o[3] = b.x + 0.0; o[4] = b.y + 0.0; o[5] = b.z + 0.0;
}

// One point.  Fused: o0 = tau(q, 0, 0), o1 = tau(q, 0, v1), o2 = tau(q, v1, v2).  Otherwise o2 = tau(q, v1, v2) alone, where a
// null v1 / v2 stands for zeros.  q, v1, v2, o* are this point's rows.  D = 0: runtime dof M.d.
template <int D, bool Fused, class State>
__device__ __forceinline__ void chain_rnea(const ChainModel &M, State &St, const double *q, const double *v1, const double *v2,
                                           double *o0, double *o1, double *o2) {
    constexpr int kFull = Fused ? 11 : 2;  // first slot of the level-2 evaluation's F, N
    const int d = D ? D : M.d;
    const V3 g = load3(M.gravity), zero{0.0, 0.0, 0.0};
    ChainKin K0{zero, zero, {-g.x, -g.y, -g.z}}, K1 = K0, K2 = K0;
    auto forward = [&](int i) {
        const ChainLink L = chain_link(M, i);
        const double qi = q[i], cv = cos(qi), sv = L.prismatic ? qi : sin(qi);
        St.at(i, 0) = sv; St.at(i, 1) = cv;
        const ChainJoint J = chain_joint(L, sv, cv);
        const double a1 = v1 ? v1[i] : 0.0, a2 = v2 ? v2[i] : 0.0;
        V3 F, Nm;
        if (Fused) {
            chain_forward<0>(L, J, K0, 0.0, 0.0, F, Nm);
            chain_put(F, St.at(i, 2), St.at(i, 3), St.at(i, 4));
            chain_forward<1>(L, J, K1, 0.0, a1, F, Nm);
            chain_put(F, St.at(i, 5), St.at(i, 6), St.at(i, 7));
            chain_put(Nm, St.at(i, 8), St.at(i, 9), St.at(i, 10));
        }
        chain_forward<2>(L, J, K2, a1, a2, F, Nm);
        chain_put(F, St.at(i, kFull), St.at(i, kFull + 1), St.at(i, kFull + 2));
        chain_put(Nm, St.at(i, kFull + 3), St.at(i, kFull + 4), St.at(i, kFull + 5));
        // unrolled, the links are one basic block: without a fence the scheduler starts every link's sine, cosine and
        // parameter loads at once and the live values overflow the register file (452 bytes of scratch at 8 dof)
        if (D > 0) __builtin_amdgcn_sched_barrier(0);
    };
    ChainWrench C0{zero, zero}, C1 = C0, C2 = C0;
    auto backward = [&](int i) {
        const ChainLink L = chain_link(M, i);
        const ChainJoint J = chain_joint(L, St.at(i, 0), St.at(i, 1));
        if (Fused) {
            o0[i] = chain_backward<0>(L, J, V3{St.at(i, 2), St.at(i, 3), St.at(i, 4)}, zero, C0);
            o1[i] = chain_backward<1>(L, J, V3{St.at(i, 5), St.at(i, 6), St.at(i, 7)}, V3{St.at(i, 8), St.at(i, 9), St.at(i, 10)}, C1);
        }
        o2[i] = chain_backward<2>(L, J, V3{St.at(i, kFull), St.at(i, kFull + 1), St.at(i, kFull + 2)},
                                  V3{St.at(i, kFull + 3), St.at(i, kFull + 4), St.at(i, kFull + 5)}, C2);
        if (D > 0) __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (D > 0) {
#pragma unroll
        for (int i = 0; i < D; ++i) forward(i);
#pragma unroll
        for (int i = D - 1; i >= 0; --i) backward(i);
    } else {
#pragma nounroll
        for (int i = 0; i < d; ++i) forward(i);
#pragma nounroll
        for (int i = d - 1; i >= 0; --i) backward(i);
    }
}

// Lanes past the last point of the batch evaluate the last point again and store the very same values where its own lane
// does: no lane is ever masked out, nothing is written outside [npoints][d].
__device__ __forceinline__ size_t chain_point(int npoints) {
    const size_t g = (size_t)blockIdx.x * kChainBlock + threadIdx.x;
    return g < (size_t)npoints ? g : (size_t)npoints - 1;
}
__device__ __forceinline__ size_t chain_row(int npoints, int d) { return chain_point(npoints) * (size_t)d; }

}  // namespace tpr

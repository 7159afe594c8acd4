// tpr_joint.hip.inc -- the wrench ACROSS any joint of a rigid-body tree: what a gearbox's output bearing, a linear guide's
// carriage or a slender link's flange carries beside the joint's own torque -- tilting moment, axial and radial force -- at every
// gridpoint of every trajectory, for a set of up to 8 sections in one launch.  The model and the walk are the tree kernels'
// (tpr_tree.hip.inc: a serial chain is the tree parent = -1, 0, 1, ...), on the banks and slots of tpr_tree_walk.hip.inc;
// chain_link, chain_joint and chain_forward<Level> are used as they are, and the way down uses chain_backward_wrench<Level>,
// chain_backward's sibling that hands out the pair (f, n) the torque kernels project on the joint axis and drop.  joint_rnea repeats
// tree_rnea's walk in its own text: written on walk functions shared with tree_rnea the single kernel was 2 % slower on the MI355X
// (profiles/rigid_body_kernel_refactor.md).
//
// The quantity.  (f_i, n_i) of the recursion: the force the parent side exerts ON link i through joint i and its moment about
// link i's origin, in link i's axes, gravity included (at rest f is the support of the weight of everything that hangs on the
// joint -- for a fork, every child branch).  A section k = (link i, origin o in link coordinates, rot R with the section's axes in
// link coordinates as columns) reports
//   w_k = [ R' f_i ;  R' (n_i + f_i x o) ]            (f x o = -o x f in every bit)
// the force and its moment about o in section axes, each output passed through "+ 0.0".  With o = 0, R = 1, axis_i . n (revolute)
// or axis_i . f (prismatic) is the joint's torque as the tree kernels form it, on the same operands.
//
// The recipe: the plain link-local recursion, tree_rnea's with (f, n) kept (DESIGN.md 3.5 has the measurement behind it).  THE
// SUMMATION ORDER is tree_rnea's: at a fork the children i != j + 1 in descending link number into the bank, then carry + bank.
//
// Sections.  They travel by value in the argument block.  S.mask (bit i: a section sits on link i) stays in a scalar register:
// a link without a section pays one scalar bit test on the way down; a link with one scans the (at most 8) section links, all
// wave-uniform.  The way down stops once the lowest-numbered section link has been served (S.lowest): nothing below it is
// needed.  The way up is the tree kernels' over all links (no cut by subtree: a link's F, N are needed by every section above it,
// and the set's subtrees cover most links in practice).
//
// Each section's output depends on its own (link, R, o) alone -- the walk does not know the set beyond where it stops --, so a
// section gives the same bits from a set of one and from any larger or permuted set.  Each output of the fused kernel equals the
// single evaluation on the same arguments in every bit (-ffp-contract=off; products by an exact zero dropped, no sum reordered).
//
// Shape: the tree kernels'.  One wave of 64 points per block, runtime dof 1 .. 32, at most 4 forks, per-link state and banks in
// dynamic LDS (joint_lds_bytes = tree_lds_bytes).  The 6 S-wide outputs leave by direct stores, six consecutive doubles per lane
// and section: no staging, no LDS of their own.  Lanes past the last point of the batch evaluate the last point again and store
// the very same values where its own lane does.
#pragma once
#include "tpr_tree_walk.hip.inc"
#include "tpr_joint_args.hpp"

namespace tpr {

// Section k's six outputs of a link's (f, n).
__device__ __forceinline__ void joint_put(const JointSections &S, int k, V3 f, V3 n, double *o) {
    M3 R;
#pragma unroll
    for (int j = 0; j < 9; ++j) R.m[j] = S.rot[k][j];
    chain_put6(mul_t(R, f), mul_t(R, n + cross(f, V3{S.origin[k][0], S.origin[k][1], S.origin[k][2]})), o);
}

// One point, as tree_rnea<Fused>: o0 = w(q, 0, 0), o1 = w(q, 0, v1), o2 = w(q, v1, v2), or o2 alone; o* = this point's [count][6].
// State and bank slots are tree_rnea's.
template <bool Fused, class State>
__device__ __forceinline__ void joint_rnea(const ChainModel &M, const TreeTables &T, const JointSections &S, State &St, double *banks,
                                           const double *q, const double *v1, const double *v2, double *o0, double *o1, double *o2) {
    constexpr int kFull = TreeSlots<Fused>::kFull, kBank2 = TreeSlots<Fused>::kBank2, kWrench2 = TreeSlots<Fused>::kWrench2;
    typename TreeSlots<Fused>::Banks Bk{banks};
    const int d = M.d;
    const V3 g = load3(M.gravity), zero{0.0, 0.0, 0.0};
    const ChainKin base{zero, zero, {-g.x, -g.y, -g.z}};
    ChainKin K0 = base, K1 = base, K2 = base;
#pragma nounroll
    for (int i = 0; i < d; ++i) {
        if (!((T.running >> i) & 1u)) {  // (the same for every lane)
            const int p = T.parent[i];
            if (p < 0) {
                K0 = base; K1 = base; K2 = base;
            } else {
                const int b = T.fork_slot[p];
                if (Fused) {
                    K0 = ChainKin{zero, zero, Bk.get(b, 0)};
                    K1 = ChainKin{zero, Bk.get(b, 3), Bk.get(b, 6)};
                }
                K2 = ChainKin{Bk.get(b, kBank2), Bk.get(b, kBank2 + 3), Bk.get(b, kBank2 + 6)};
            }
        }
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
        if ((T.forks >> i) & 1u) {  // (the same for every lane)
            const int own = T.fork_slot[i];
            if (Fused) {
                Bk.put(own, 0, K0.a);
                Bk.put(own, 3, K1.wd); Bk.put(own, 6, K1.a);
            }
            Bk.put(own, kBank2, K2.w); Bk.put(own, kBank2 + 3, K2.wd); Bk.put(own, kBank2 + 6, K2.a);
        }
    }
    const ChainWrench none{zero, zero};
    ChainWrench C0 = none, C1 = none, C2 = none;  // the carry: link i + 1's wrench when it is link i's child, else zero
    const int lowest = S.lowest;
#pragma nounroll
    for (int i = d - 1; i >= lowest; --i) {
        if ((T.forks >> i) & 1u) {  // (the same for every lane)
            const int own = T.fork_slot[i];
            const bool carried = i + 1 < d && ((T.running >> (i + 1)) & 1u);
            if (Fused) {
                const ChainWrench W0 = Bk.wrench(own, 0), W1 = Bk.wrench(own, 6);
                C0 = carried ? ChainWrench{C0.f + W0.f, C0.n + W0.n} : W0;
                C1 = carried ? ChainWrench{C1.f + W1.f, C1.n + W1.n} : W1;
            }
            const ChainWrench W2 = Bk.wrench(own, kWrench2);
            C2 = carried ? ChainWrench{C2.f + W2.f, C2.n + W2.n} : W2;
        }
        const ChainLink L = chain_link(M, i);
        const ChainJoint J = chain_joint(L, St.at(i, 0), St.at(i, 1));
        V3 f0 = zero, n0 = zero, f1 = zero, n1 = zero, f2, n2;
        if (Fused) {
            chain_backward_wrench<0>(L, J, V3{St.at(i, 2), St.at(i, 3), St.at(i, 4)}, zero, C0, f0, n0);
            chain_backward_wrench<1>(L, J, V3{St.at(i, 5), St.at(i, 6), St.at(i, 7)}, V3{St.at(i, 8), St.at(i, 9), St.at(i, 10)}, C1, f1, n1);
        }
        chain_backward_wrench<2>(L, J, V3{St.at(i, kFull), St.at(i, kFull + 1), St.at(i, kFull + 2)},
                                 V3{St.at(i, kFull + 3), St.at(i, kFull + 4), St.at(i, kFull + 5)}, C2, f2, n2);
        if ((S.mask >> i) & 1u) {  // (the same for every lane)
#pragma nounroll
            for (int k = 0; k < S.count; ++k) {
                if (S.link[k] != i) continue;
                if (Fused) {
                    joint_put(S, k, f0, n0, o0 + 6 * k);
                    joint_put(S, k, f1, n1, o1 + 6 * k);
                }
                joint_put(S, k, f2, n2, o2 + 6 * k);
            }
        }
        if (!((T.running >> i) & 1u)) {  // (the same for every lane)
            const int p = T.parent[i];
            if (p >= 0) {
                const int b = T.fork_slot[p];
                const bool first = (T.first >> i) & 1u;
                if (Fused) {
                    Bk.hand_up(b, 0, C0, first); Bk.hand_up(b, 6, C1, first);
                }
                Bk.hand_up(b, kWrench2, C2, first);
            }
            C0 = none; C1 = none; C2 = none;
        }
    }
}

static __global__ void __launch_bounds__(kChainBlock) joint_wrench_kernel(JointWrenchArgs A) {
    extern __shared__ double chain_lds[];
    const size_t pt = chain_point(A.npoints), at = pt * (size_t)A.M.d, to = pt * (size_t)(6 * A.S.count);
    ChainLdsState<kChainSlotsSingle> St{chain_lds + threadIdx.x};
    double *banks = chain_lds + A.M.d * kChainSlotsSingle * kChainBlock + threadIdx.x;
    joint_rnea<false>(A.M, A.T, A.S, St, banks, A.q + at, A.qd + at, A.qdd + at, nullptr, nullptr, A.wrench + to);
}

// FusedState: the 17 doubles per link and 18 per fork fit the LDS (joint_terms_fused); otherwise one evaluation after the other
// on 8 and 9, as tree_torque_terms_kernel does.
template <bool FusedState>
static __global__ void __launch_bounds__(kChainBlock) joint_wrench_terms_kernel(JointWrenchTermsArgs A) {
    extern __shared__ double chain_lds[];
    const size_t pt = chain_point(A.npoints), at = pt * (size_t)A.M.d, to = pt * (size_t)(6 * A.S.count);
    if constexpr (FusedState) {
        ChainLdsState<kChainSlotsFused> St{chain_lds + threadIdx.x};
        double *banks = chain_lds + A.M.d * kChainSlotsFused * kChainBlock + threadIdx.x;
        joint_rnea<true>(A.M, A.T, A.S, St, banks, A.q + at, A.qs + at, A.qss + at, A.w0 + to, A.wa + to, A.wb + to);
    } else {
        ChainLdsState<kChainSlotsSingle> St{chain_lds + threadIdx.x};
        double *banks = chain_lds + A.M.d * kChainSlotsSingle * kChainBlock + threadIdx.x;
        joint_rnea<false>(A.M, A.T, A.S, St, banks, A.q + at, nullptr, nullptr, nullptr, nullptr, A.w0 + to);
        joint_rnea<false>(A.M, A.T, A.S, St, banks, A.q + at, nullptr, A.qs + at, nullptr, nullptr, A.wa + to);
        joint_rnea<false>(A.M, A.T, A.S, St, banks, A.q + at, A.qs + at, A.qss + at, nullptr, nullptr, A.wb + to);
    }
}

}  // namespace tpr

// tpr_tree.hip.inc -- recursive Newton-Euler inverse dynamics of a kinematic TREE (a branched robot: two arms on a torso, an arm
// beside a pan-tilt head, a forest of robots on one base) at every gridpoint of every trajectory.  The model is tpr_chain's with
// a parent table beside it; the recursion is tpr_chain_rnea.hip.inc's -- chain_link, chain_joint, chain_forward<Level> and
// chain_backward<Level> are used as they are -- and what is new is the walk around them.  The banks and the slots of state and banks
// are tpr_tree_walk.hip.inc's, shared with the joint-load kernels (tpr_joint.hip.inc), whose joint_rnea repeats tree_rnea's walk.
//
// The walk.  Links are numbered topologically (parent[i] < i), so one loop up and one loop down visit every link after (before)
// its parent.  Forward, link i takes the parent's (w, wd, a):
//   parent[i] == i - 1    the running state in registers, as in a chain (link 0 with the base as parent included)
//   parent[i] == -1       a further root: the base state again (w = wd = 0, a = -gravity)
//   otherwise             loaded from the parent's BANK: a FORK -- a link that is the parent of some link i != j + 1 -- stores its
//                         state there once it is computed, for the children that come after a whole sub-chain
// Backward (links d-1 .. 0), link i hands its wrench, transformed into the parent's frame by chain_backward, to the parent:
//   parent[i] == i - 1    it stays in registers as the carry
//   parent[i] == -1       dropped
//   otherwise             into the parent's bank -- the storage the forward pass used, dead by now: the first contribution a bank
//                         receives is stored (not added to a zero), every later one is added to what the bank holds
// and a fork starts from  C = carry + bank  (bank alone when link j + 1 is not its child); any other link from its carry, or from
// zero when it has no child, as a chain's tip does.
//
// THE SUMMATION ORDER of the children's wrenches at a fork j, fixed: the children i != j + 1 in DESCENDING link number, summed
// left to right into the bank, ((c_last + c_before) + ...); then carry + bank with the carry (child j + 1) on the left.  With one
// child only there is no sum at all, so a chain-shaped tree evaluates the chain's expressions one for one and gives the chain
// kernels' bits at every dof, and each output of the fused kernel equals the single evaluation's (-ffp-contract=off).
//
// Every decision of the walk reads the tables (TreeTables, by value in the argument block) by the loop index: wave-uniform
// branches around LDS accesses, never around arithmetic; the joint type stays a select.  "Is this link's parent the link before
// it" and "is this link a fork" are bits of two masks that stay in scalar registers, so a chain-shaped stretch pays two scalar bit
// tests per link and pass; the byte tables (which parent, which bank) are read only where a branch begins or ends.
//
// Shape: chain_inverse_dynamics_lds_kernel's and chain_torque_terms_lds_kernel's.  One wave of 64 points per block, runtime dof
// 1 .. 32, a point's per-link state in dynamic LDS as [link][slot][lane] (8 slots, 17 fused), the banks behind it as
// [fork][slot][lane] (9 doubles, 3 + 6 + 9 = 18 fused): d * 8 * 512 + forks * 9 * 512 bytes (149 504 at 32 dof with 4 forks), fused
// d * 17 * 512 + forks * 18 * 512.  Lanes past the last point of the batch evaluate the last point again and store the very same
// values where its own lane does.
#pragma once
#include "tpr_tree_walk.hip.inc"

namespace tpr {

// One point, as chain_rnea<0, Fused>: o0 = tau(q, 0, 0), o1 = tau(q, 0, v1), o2 = tau(q, v1, v2), or o2 alone.
template <bool Fused, class State>
__device__ __forceinline__ void tree_rnea(const ChainModel &M, const TreeTables &T, State &St, double *banks, const double *q,
                                          const double *v1, const double *v2, double *o0, double *o1, double *o2) {
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
#pragma nounroll
    for (int i = d - 1; i >= 0; --i) {
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
        if (Fused) {
            o0[i] = chain_backward<0>(L, J, V3{St.at(i, 2), St.at(i, 3), St.at(i, 4)}, zero, C0);
            o1[i] = chain_backward<1>(L, J, V3{St.at(i, 5), St.at(i, 6), St.at(i, 7)}, V3{St.at(i, 8), St.at(i, 9), St.at(i, 10)}, C1);
        }
        o2[i] = chain_backward<2>(L, J, V3{St.at(i, kFull), St.at(i, kFull + 1), St.at(i, kFull + 2)},
                                  V3{St.at(i, kFull + 3), St.at(i, kFull + 4), St.at(i, kFull + 5)}, C2);
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

static __global__ void __launch_bounds__(kChainBlock) tree_inverse_dynamics_kernel(TreeDynArgs A) {
    extern __shared__ double chain_lds[];
    const size_t at = chain_row(A.npoints, A.M.d);
    ChainLdsState<kChainSlotsSingle> St{chain_lds + threadIdx.x};
    double *banks = chain_lds + A.M.d * kChainSlotsSingle * kChainBlock + threadIdx.x;
    tree_rnea<false>(A.M, A.T, St, banks, A.q + at, A.qd + at, A.qdd + at, nullptr, nullptr, A.tau + at);
}

// FusedState: the 17 doubles per link and 18 per fork fit the LDS; otherwise one evaluation after the other on 8 and 9.
template <bool FusedState>
static __global__ void __launch_bounds__(kChainBlock) tree_torque_terms_kernel(TreeTermsArgs A) {
    extern __shared__ double chain_lds[];
    const size_t at = chain_row(A.npoints, A.M.d);
    if constexpr (FusedState) {
        ChainLdsState<kChainSlotsFused> St{chain_lds + threadIdx.x};
        double *banks = chain_lds + A.M.d * kChainSlotsFused * kChainBlock + threadIdx.x;
        tree_rnea<true>(A.M, A.T, St, banks, A.q + at, A.qs + at, A.qss + at, A.w0 + at, A.wa + at, A.wb + at);
    } else {
        ChainLdsState<kChainSlotsSingle> St{chain_lds + threadIdx.x};
        double *banks = chain_lds + A.M.d * kChainSlotsSingle * kChainBlock + threadIdx.x;
        tree_rnea<false>(A.M, A.T, St, banks, A.q + at, nullptr, nullptr, nullptr, nullptr, A.w0 + at);
        tree_rnea<false>(A.M, A.T, St, banks, A.q + at, nullptr, A.qs + at, nullptr, nullptr, A.wa + at);
        tree_rnea<false>(A.M, A.T, St, banks, A.q + at, A.qs + at, A.qss + at, nullptr, nullptr, A.wb + at);
    }
}

}  // namespace tpr

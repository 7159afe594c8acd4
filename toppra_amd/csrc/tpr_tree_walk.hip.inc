// tpr_tree_walk.hip.inc -- what the two walks over a kinematic tree, tree_rnea (tpr_tree.hip.inc) and joint_rnea (tpr_joint.hip.inc),
// agree on: the banks of the forks and the slots of state and banks.  Device code only, no kernel.  What the walk does, why, and THE
// SUMMATION ORDER at a fork are at the head of tpr_tree.hip.inc.
#pragma once
#include "tpr_chain_rnea.hip.inc"
#include "tpr_tree_args.hpp"

namespace tpr {

// This lane's banks: [fork][slot][lane].
template <int Doubles>
struct TreeBanks : ChainLaneBanks<Doubles> {
    using ChainLaneBanks<Doubles>::get;
    using ChainLaneBanks<Doubles>::put;
    __device__ __forceinline__ ChainWrench wrench(int b, int s) { return {get(b, s), get(b, s + 3)}; }
    // the first contribution is stored; a later one is added to what the bank holds (bank on the left)
    __device__ __forceinline__ void hand_up(int b, int s, const ChainWrench &C, bool first) {
        if (first) {
            put(b, s, C.f); put(b, s + 3, C.n);
        } else {
            put(b, s, get(b, s) + C.f); put(b, s + 3, get(b, s + 3) + C.n);
        }
    }
};

// State slots are chain_rnea's.  Bank slots, forward: fused a0 | wd1 a1 | w2 wd2 a2 at 0, 3, 9; single w wd a.  Backward: (f, n)
// per level at 0, 6, 12; single at 0.
template <bool Fused>
struct TreeSlots {
    static constexpr int kFull = Fused ? 11 : 2;     // first slot of the level-2 evaluation's F, N
    static constexpr int kBank2 = Fused ? 9 : 0;     // first bank slot of the level-2 evaluation, forward
    static constexpr int kWrench2 = Fused ? 12 : 0;  // ... and backward
    using Banks = TreeBanks<Fused ? kTreeBankFused : kTreeBankSingle>;
};

}  // namespace tpr

// tpr_tree_args.hpp -- argument blocks of the kinematic-tree kernels (tpr_tree.hip.inc), shared with the C-ABI entries, and the
// host function that turns a parent array into the tables the kernels walk by.
#pragma once
#include <cstddef>
#include <cstdint>

#include "tpr_chain_args.hpp"
namespace tpr {
constexpr int kTreeMaxDof = 32;    // TPR_MAX_DOF
constexpr int kTreeMaxForks = 4;   // TPR_TREE_MAX_FORKS
// Doubles of LDS one thread keeps per fork (its bank): forward, the fork's (w, wd, a) for its later children -- 9, or
// 3 (a) + 6 (wd, a) + 9 for the three levels of the fused kernel; backward, the same storage takes the summed wrenches
// (f, n) of those children, 6 per level.
constexpr int kTreeBankSingle = 9, kTreeBankFused = 3 + 6 + 9;

// The tree's structure by value: the same for every lane, every decision on it is wave-uniform.
//   parent[i]     the link joint i attaches link i to, -1 = the base; -1 <= parent[i] < i
//   fork_slot[j]  the bank of link j when it is a fork (the parent of some link i != j + 1), else -1
//   running       bit i: parent[i] == i - 1 -- the chain's case, told without a look at the tables (link 0 on the base included)
//   forks         bit j: link j is a fork
//   first         bit i: link i is the LAST-numbered child i != parent[i] + 1 of its parent, i.e. the first one the backward
//                 walk meets: its wrench is stored into the parent's bank, the others' are added
struct TreeTables {
    int8_t parent[kTreeMaxDof], fork_slot[kTreeMaxDof];
    uint32_t running, forks, first;
};

struct TreeDynArgs {
    ChainModel M;  // (M.tool is not read)
    TreeTables T;
    int npoints;
    const double *q, *qd, *qdd;  // [npoints][d]
    double *tau;
};

struct TreeTermsArgs {
    ChainModel M;
    TreeTables T;
    int npoints;
    const double *q, *qs, *qss;  // [npoints][d]
    double *w0, *wa, *wb;
};

// The tables of a host parent array [d]: returns the number of forks, or -1 - i for the first link i whose parent is outside
// -1 .. i-1 (-1 - d for a dof outside 1 .. 32).  More than kTreeMaxForks forks are counted, not refused: the caller refuses
// them (T then holds slots the kernels have no bank for and must not be launched with).
inline int tree_tables(const int32_t *parent, int d, TreeTables &T) {
    if (d < 1 || d > kTreeMaxDof) return -1 - d;
    for (int i = 0; i < kTreeMaxDof; ++i) T.parent[i] = T.fork_slot[i] = -1;
    T.running = T.forks = T.first = 0;
    for (int i = 0; i < d; ++i) {
        if (parent[i] < -1 || parent[i] >= i) return -1 - i;
        T.parent[i] = (int8_t)parent[i];
        if (parent[i] == i - 1) T.running |= 1u << i;
    }
    int forks = 0;
    for (int i = 0; i < d; ++i) {  // slots in the order in which the forks are numbered
        const int p = parent[i];
        if (p >= 0 && p != i - 1 && T.fork_slot[p] < 0) T.fork_slot[p] = -2;
    }
    for (int j = 0; j < d; ++j)
        if (T.fork_slot[j] == -2) {
            T.fork_slot[j] = (int8_t)forks++;
            T.forks |= 1u << j;
        }
    uint32_t seen = 0;
    for (int i = d - 1; i >= 0; --i) {
        const int p = parent[i];
        if (p >= 0 && p != i - 1 && !(seen >> p & 1u)) {
            T.first |= 1u << i;
            seen |= 1u << p;
        }
    }
    return forks;
}

// Dynamic LDS of a launch: the per-link state of the chain kernels plus one bank per fork.
constexpr size_t tree_lds_bytes(int d, int forks, bool fused) {
    return ((size_t)d * (size_t)(fused ? kChainSlotsFused : kChainSlotsSingle) + (size_t)forks * (size_t)(fused ? kTreeBankFused : kTreeBankSingle)) *
           (size_t)kChainBlock * sizeof(double);
}
static_assert(tree_lds_bytes(kTreeMaxDof, kTreeMaxForks, false) == 149504 && tree_lds_bytes(kTreeMaxDof, kTreeMaxForks, false) <= (size_t)kChainLdsBytes,
              "the single state fits the LDS at 32 dof with 4 forks");
static_assert(tree_lds_bytes(17, 1, true) <= (size_t)kChainLdsBytes && tree_lds_bytes(18, 1, true) > (size_t)kChainLdsBytes,
              "with one fork the fused state fits up to 17 dof");
}  // namespace tpr

// tpr_momentum_args.hpp -- argument block of the momentum kernel (tpr_momentum.hip.inc), shared with the C-ABI entry.
#pragma once
#include "tpr_mount_args.hpp"
namespace tpr {
// Doubles of LDS one thread keeps per fork (its bank): the fork's frame in base coordinates, W (9) and p (3), and its velocity
// state v, w (3 + 3) for its later children.  Forward only, first order: nothing comes back down and no acceleration is carried.
constexpr int kMomentumBank = 12 + 6;
// Doubles a point leaves through LDS: momentum (6), energy2 (1), xbound (2), one row at this (odd) pitch.
constexpr int kMomentumOut = 6 + 1 + 2;

// Dynamic LDS of a launch: q, q' [64][d | 1] staged (or the 64 output rows where that is more) plus one bank per fork.  Host and
// device: the launcher sizes the launch with it.
constexpr size_t momentum_stage_doubles(int d) {
    const size_t in = 2 * (size_t)kChainBlock * (size_t)(d | 1), out = (size_t)kChainBlock * kMomentumOut;
    return in > out ? in : out;
}
constexpr size_t momentum_lds_bytes(int d, int forks) {
    return (momentum_stage_doubles(d) + (size_t)forks * kMomentumBank * kChainBlock) * sizeof(double);
}
static_assert(kMomentumOut % 2 == 1, "the output pitch is odd: a wave's rows fall on different banks");
static_assert(momentum_lds_bytes(kTreeMaxDof, kTreeMaxForks) == 33792 + 4 * 18 * 512 && momentum_lds_bytes(kTreeMaxDof, kTreeMaxForks) == 70656 &&
                  momentum_lds_bytes(kTreeMaxDof, kTreeMaxForks) <= (size_t)kChainLdsBytes,
              "two staged rows plus four banks fit the LDS at 32 dof");
static_assert(momentum_lds_bytes(1, 0) == 64 * 9 * 8 && momentum_lds_bytes(4, 0) == 2 * 64 * 5 * 8, "below 4 dof the outputs size the staging area");

struct MomentumArgs {
    ChainModel M;  // (M.tool and M.gravity are not read)
    TreeTables T;
    MountFrame P;  // (rot and origin are read; the platform does not move)
    uint32_t mask;            // bit i: link i is in the sum
    int npoints, n1, nlinks;  // B (N + 1); N + 1; the highest link of the mask, plus one
    const double *q, *qs;     // [npoints][d]
    const double *limit;      // [B][3] = (p_max^2, L_max^2, 2 E_max), or null
    double *momentum;         // [npoints][6] or null
    double *energy2;          // [npoints] or null
    double *xbound;           // [npoints][2] or null
};
}  // namespace tpr

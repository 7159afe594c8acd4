// tpr_effmass_args.hpp -- argument block of the effective-mass kernel (tpr_effmass.hip.inc), shared with the C-ABI entry.
#pragma once
#include "tpr_tree_args.hpp"
namespace tpr {
// Slots of LDS (a slot = one double per lane of the block's wave: 512 bytes) the kernel keeps
//   per link   2: (sin q | q, cos q), written on the way up, read on the way down
//   per point  4 + 4: the force's linear part and s2, written on the way up when the point's link is reached (its "own" slots);
//                     the moment part of the bias wrench (3) and g, live on the way down only
//   per fork   21: v, w (6) on the way up; the summed articulated inertias of its later children (21) on the way down
// and the staged rows of q, q', 2 (d | 1) slots, live on the way up only: they share their slots with the points' way-down
// slots, which nothing writes before the way up has read its last row.
constexpr int kEffMassLink = 2, kEffMassOwn = 3 + 1, kEffMassDown = 3 + 1, kEffMassBank = 6 + 9 + 6;

// Dynamic LDS of a launch, in slots and bytes.  Host and device: the launcher sizes the launch with it.
constexpr size_t effmass_shared_slots(int d, int points) {
    const size_t stage = 2 * (size_t)(d | 1), down = (size_t)kEffMassDown * (size_t)points;
    return stage > down ? stage : down;
}
constexpr size_t effmass_lds_bytes(int d, int points, int forks) {
    return ((size_t)kEffMassLink * (size_t)d + (size_t)kEffMassOwn * (size_t)points + effmass_shared_slots(d, points) +
            (size_t)kEffMassBank * (size_t)forks) * (size_t)kChainBlock * sizeof(double);
}
static_assert(effmass_lds_bytes(kTreeMaxDof, kChainMaxPoints, kTreeMaxForks) == (64 + 64 + 66 + 84) * 512 &&
                  effmass_lds_bytes(kTreeMaxDof, kChainMaxPoints, kTreeMaxForks) == 142336 &&
                  effmass_lds_bytes(kTreeMaxDof, kChainMaxPoints, kTreeMaxForks) <= (size_t)kChainLdsBytes,
              "32 links, 16 points and 4 forks fit the LDS with the staged rows under the points' way-down slots");
static_assert((64 + 64 + 64 + 66 + 84) * 512 == 175104 && 175104 > kChainLdsBytes, "... and would not with slots of their own");
static_assert(effmass_lds_bytes(1, 1, 0) == (2 + 4 + 4) * 512 && effmass_lds_bytes(7, 1, 0) == (14 + 4 + 14) * 512, "the larger of the two shares");

struct EffMassArgs {
    ChainModel M;  // (M.tool and M.gravity are not read)
    TreeTables T;
    ChainPoints P;
    double direction[kChainMaxPoints][3];  // per point, link axes; read when `directed`
    uint16_t active[kTreeMaxDof];          // bit p of [i]: link i lies on the path from point p's link to its root
    uint16_t own[kTreeMaxDof];             // bit p of [i]: point p sits on link i
    uint32_t walk;                         // bit i: link i belongs to a root's tree that carries a point (the others are skipped)
    int directed;                          // 0: the force along the point's velocity; 1: along direction[p]
    int npoints, n1;                       // B (N + 1); N + 1
    const double *q, *qs;                  // [npoints][d]  (qs is q again where the caller gave none: s2 is not asked for then)
    const double *limit;                   // [B][count][2] = (2 E_max, 1 / m_body), or null
    double *speed2;                        // [npoints][count] or null
    double *mobility;                      // [npoints][count] or null
    double *xbound;                        // [npoints][2] or null
};
}  // namespace tpr

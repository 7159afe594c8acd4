// tpr_mount_args.hpp -- argument blocks of the base-reaction kernels (tpr_mount.hip.inc), shared with the C-ABI entries.
#pragma once
#include "tpr_tree_args.hpp"
namespace tpr {
// Doubles of LDS one thread keeps per fork (its bank): the fork's frame in base coordinates, W (9) and p (3), shared by the
// evaluations, and its (w, wd, a) for its later children -- 9, or 6 (wd, a) + 9 for the two levels the fused kernel runs a
// recursion for (gravity is not in it: w(q, 0, 0) has no recursion).  Forward only: nothing comes back down.
constexpr int kMountBankSingle = 12 + 9, kMountBankFused = 12 + 6 + 9;

// The mount (tpr_mount), by value: the same for every lane.  rot: columns = the mount frame's axes in base coordinates.
struct MountFrame {
    double rot[9], origin[3], mass, com[3];
};

struct MountWrenchArgs {
    ChainModel M;  // (M.tool is not read)
    TreeTables T;
    MountFrame P;
    int npoints;
    const double *q, *qd, *qdd;  // [npoints][d]
    double *wrench;              // [npoints][6]: force, moment about the mount frame's origin, mount-frame axes
};

struct MountWrenchTermsArgs {
    ChainModel M;
    TreeTables T;
    MountFrame P;
    int npoints;
    const double *q, *qs, *qss;  // [npoints][d]
    double *w0, *wa, *wb;        // [npoints][6]
};
}  // namespace tpr

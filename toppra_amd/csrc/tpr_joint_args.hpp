// tpr_joint_args.hpp -- argument blocks of the joint-wrench kernels (tpr_joint.hip.inc), shared with the C-ABI entries.
#pragma once
#include "tpr_tree_args.hpp"
namespace tpr {
constexpr int kJointMaxSections = 8;  // TPR_JOINT_MAX_SECTIONS

// The sections (tpr_joint_sections), by value: the same for every lane.  link[k] is resolved (0 .. d-1); rot[k]: row-major,
// columns = the section frame's axes in link coordinates; origin[k] in link coordinates.  Built by the C-ABI entry:
//   mask    bit i: some section sits on link i -- it stays in a scalar register, a link without one pays one bit test
//   lowest  the lowest-numbered section link: the way down stops once it has been served
struct JointSections {
    int32_t count, lowest;
    uint32_t mask;
    int32_t link[kJointMaxSections];
    double rot[kJointMaxSections][9], origin[kJointMaxSections][3];
};

struct JointWrenchArgs {
    ChainModel M;  // (M.tool is not read)
    TreeTables T;
    JointSections S;
    int npoints;
    const double *q, *qd, *qdd;  // [npoints][d]
    double *wrench;              // [npoints][count][6]: per section force, moment about its origin, section axes
};

struct JointWrenchTermsArgs {
    ChainModel M;
    TreeTables T;
    JointSections S;
    int npoints;
    const double *q, *qs, *qss;  // [npoints][d]
    double *w0, *wa, *wb;        // [npoints][count][6]
};

// Dynamic LDS of a launch: the tree kernels' (tree_lds_bytes) -- the per-link state plus one bank per fork.  The outputs leave by
// direct stores and take none.  Fused: the terms kernel's one-pass mode; it is chosen where this fits kChainLdsBytes, otherwise the
// three evaluations run one after another on the single state.
constexpr size_t joint_lds_bytes(int d, int forks, bool fused) { return tree_lds_bytes(d, forks, fused); }
constexpr bool joint_terms_fused(int d, int forks) { return joint_lds_bytes(d, forks, true) <= (size_t)kChainLdsBytes; }
static_assert(joint_lds_bytes(kTreeMaxDof, kTreeMaxForks, false) == (32 * 8 + 4 * 9) * 512 &&
                  joint_lds_bytes(kTreeMaxDof, kTreeMaxForks, false) <= (size_t)kChainLdsBytes && !joint_terms_fused(kTreeMaxDof, kTreeMaxForks),
              "32 dof with 4 forks is served by the sequential mode within the LDS");
static_assert(joint_lds_bytes(15, 1, true) == (15 * 17 + 18) * 512 && joint_terms_fused(15, 1) && joint_terms_fused(17, 1) && !joint_terms_fused(18, 1) &&
                  joint_terms_fused(18, 0) && !joint_terms_fused(19, 0),
              "fused: 17 doubles per link and 18 per fork; a chain to 18 dof, one fork to 17");
static_assert(sizeof(JointSections) == 12 + 4 * kJointMaxSections + 4 + 8 * 12 * kJointMaxSections && offsetof(JointSections, rot) % 8 == 0,
              "the sections are packed: three words, the links, one word of padding, then 12 doubles per section");
}  // namespace tpr

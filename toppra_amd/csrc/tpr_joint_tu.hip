// tpr_joint_tu.hip -- translation unit of the joint-wrench kernels (tpr_joint.hip.inc): the wrench across any joint of a chain or
// tree for a set of sections, and the three evaluations of a constraint on it in one launch.  build.py compiles it in parallel
// with the other units.  Two entry points, declared in tpr_kernels.hip; each takes the argument block with the kernels' tables
// and sections in it (A->T, A->S, built and validated by the C-ABI entry) and the fork count, and returns 0 = launched, -1 = a dof
// outside 1 .. 32, a fork count outside 0 .. 4 (they size the LDS) or a section count outside 1 .. 8, -3 = the LDS could not be
// reserved.
#include "tpr_chain_launch.hpp"
#include "tpr_joint.hip.inc"

static_assert(TPR_JOINT_MAX_SECTIONS == tpr::kJointMaxSections, "the header's limit is the kernels'");

using tpr::chain_allow_lds;
using tpr::chain_blocks;

namespace {
std::atomic<unsigned long long> g_wrench_lds{0}, g_terms_fused_lds{0}, g_terms_serial_lds{0};

inline bool joint_shape_ok(int d, int forks, const tpr::JointSections &S) {
    return tpr::chain_dof_ok(d) && forks >= 0 && forks <= tpr::kTreeMaxForks && S.count >= 1 && S.count <= tpr::kJointMaxSections &&
           S.lowest >= 0 && S.lowest < d;
}
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_joint_wrench_launch(const tpr::JointWrenchArgs *A, int forks, hipStream_t stream) {
    if (!joint_shape_ok(A->M.d, forks, A->S)) return -1;
    const size_t lds = tpr::joint_lds_bytes(A->M.d, forks, false);
    if (chain_allow_lds(tpr::joint_wrench_kernel, lds, g_wrench_lds) != 0) return -3;
    hipLaunchKernelGGL(tpr::joint_wrench_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), lds, stream, *A);
    return 0;
}

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_joint_wrench_terms_launch(const tpr::JointWrenchTermsArgs *A, int forks, hipStream_t stream) {
    if (!joint_shape_ok(A->M.d, forks, A->S)) return -1;
    const dim3 grid(chain_blocks(A->npoints)), block(tpr::kChainBlock);
    if (tpr::joint_terms_fused(A->M.d, forks)) {
        const size_t lds = tpr::joint_lds_bytes(A->M.d, forks, true);
        if (chain_allow_lds(tpr::joint_wrench_terms_kernel<true>, lds, g_terms_fused_lds) != 0) return -3;
        hipLaunchKernelGGL(tpr::joint_wrench_terms_kernel<true>, grid, block, lds, stream, *A);
    } else {
        const size_t lds = tpr::joint_lds_bytes(A->M.d, forks, false);
        if (chain_allow_lds(tpr::joint_wrench_terms_kernel<false>, lds, g_terms_serial_lds) != 0) return -3;
        hipLaunchKernelGGL(tpr::joint_wrench_terms_kernel<false>, grid, block, lds, stream, *A);
    }
    return 0;
}

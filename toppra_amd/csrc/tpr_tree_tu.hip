// tpr_tree_tu.hip -- translation unit of the kinematic-tree kernels (tpr_tree.hip.inc): inverse dynamics of a branched robot and
// the three evaluations of a torque constraint in one launch.  build.py compiles it in parallel with the other units.  Two entry
// points, declared in tpr_kernels.hip; each takes the argument block with the kernels' tables in it (A->T, built and validated
// by the C-ABI entry) and their fork count, and returns 0 = launched, -1 = a dof outside 1 .. 32 or a fork count outside
// 0 .. 4 (they size the LDS), -3 = the LDS could not be reserved.
#include "tpr_chain_launch.hpp"
#include "tpr_tree.hip.inc"

static_assert(TPR_TREE_MAX_FORKS == tpr::kTreeMaxForks && TPR_MAX_DOF == tpr::kTreeMaxDof, "the header's limits are the kernels'");

using tpr::chain_allow_lds;
using tpr::chain_blocks;

namespace {
std::atomic<unsigned long long> g_dyn_lds{0}, g_terms_fused_lds{0}, g_terms_serial_lds{0};

inline bool tree_shape_ok(int d, int forks) { return tpr::chain_dof_ok(d) && forks >= 0 && forks <= tpr::kTreeMaxForks; }
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_tree_dynamics_launch(const tpr::TreeDynArgs *A, int forks, hipStream_t stream) {
    if (!tree_shape_ok(A->M.d, forks)) return -1;
    const size_t lds = tpr::tree_lds_bytes(A->M.d, forks, false);
    if (chain_allow_lds(tpr::tree_inverse_dynamics_kernel, lds, g_dyn_lds) != 0) return -3;
    hipLaunchKernelGGL(tpr::tree_inverse_dynamics_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), lds, stream, *A);
    return 0;
}

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_tree_terms_launch(const tpr::TreeTermsArgs *A, int forks, hipStream_t stream) {
    if (!tree_shape_ok(A->M.d, forks)) return -1;
    const dim3 grid(chain_blocks(A->npoints)), block(tpr::kChainBlock);
    if (tpr::tree_lds_bytes(A->M.d, forks, true) <= (size_t)tpr::kChainLdsBytes) {
        const size_t lds = tpr::tree_lds_bytes(A->M.d, forks, true);
        if (chain_allow_lds(tpr::tree_torque_terms_kernel<true>, lds, g_terms_fused_lds) != 0) return -3;
        hipLaunchKernelGGL(tpr::tree_torque_terms_kernel<true>, grid, block, lds, stream, *A);
    } else {
        const size_t lds = tpr::tree_lds_bytes(A->M.d, forks, false);
        if (chain_allow_lds(tpr::tree_torque_terms_kernel<false>, lds, g_terms_serial_lds) != 0) return -3;
        hipLaunchKernelGGL(tpr::tree_torque_terms_kernel<false>, grid, block, lds, stream, *A);
    }
    return 0;
}

// tpr_tree_tu.hip -- translation unit of the kinematic-tree kernels (tpr_tree.hip.inc): inverse dynamics of a branched robot and
// the three evaluations of a torque constraint in one launch.  build.py compiles it in parallel with the other units.  Two entry
// points, declared in tpr_kernels.hip; each takes the HOST parent array, builds the kernels' tables from it and returns
// 0 = launched, -1 = a parent outside -1 .. i-1 or a dof outside 1 .. 32, -2 = more forks than banks, -3 = the LDS could not be
// reserved.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/toppra_hip.h"
#include "tpr_tree.hip.inc"

static_assert(TPR_TREE_MAX_FORKS == tpr::kTreeMaxForks && TPR_MAX_DOF == tpr::kTreeMaxDof, "the header's limits are the kernels'");

namespace {
inline unsigned tree_blocks(int npoints) { return (unsigned)(((long long)npoints + tpr::kChainBlock - 1) / tpr::kChainBlock); }

// Above 64 KB of dynamic LDS a kernel has to be told so, once per device (as the chain unit's chain_allow_lds does): `done` is
// the kernel's bit mask of the devices that have been told; the attribute is raised to the full 160 KB, so one call serves
// every dof and fork count.
template <class Kernel>
int tree_allow_lds(Kernel kernel, size_t lds, std::atomic<unsigned long long> &done) {
    if (lds > (size_t)tpr::kChainLdsBytes) return -1;
    if (lds <= 64 * 1024) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
    if (done.load(std::memory_order_relaxed) >> dev & 1ull) return 0;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, tpr::kChainLdsBytes) != hipSuccess) return -1;
    done.fetch_or(1ull << dev, std::memory_order_relaxed);
    return 0;
}
std::atomic<unsigned long long> g_dyn_lds{0}, g_terms_fused_lds{0}, g_terms_serial_lds{0};

// The tables of `parent` into T; the fork count, or the launchers' error code.
int tree_prepare(const int32_t *parent, int d, tpr::TreeTables &T) {
    if (!parent) return -1;
    const int forks = tpr::tree_tables(parent, d, T);
    if (forks < 0) return -1;
    return forks > tpr::kTreeMaxForks ? -2 : forks;
}
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_tree_dynamics_launch(const tpr::TreeDynArgs *A, const int32_t *parent, hipStream_t stream) {
    tpr::TreeDynArgs K = *A;
    const int forks = tree_prepare(parent, K.M.d, K.T);
    if (forks < 0) return forks;
    const size_t lds = tpr::tree_lds_bytes(K.M.d, forks, false);
    if (tree_allow_lds(tpr::tree_inverse_dynamics_kernel, lds, g_dyn_lds) != 0) return -3;
    hipLaunchKernelGGL(tpr::tree_inverse_dynamics_kernel, dim3(tree_blocks(K.npoints)), dim3(tpr::kChainBlock), lds, stream, K);
    return 0;
}

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_tree_terms_launch(const tpr::TreeTermsArgs *A, const int32_t *parent, hipStream_t stream) {
    tpr::TreeTermsArgs K = *A;
    const int forks = tree_prepare(parent, K.M.d, K.T);
    if (forks < 0) return forks;
    const dim3 grid(tree_blocks(K.npoints)), block(tpr::kChainBlock);
    if (tpr::tree_lds_bytes(K.M.d, forks, true) <= (size_t)tpr::kChainLdsBytes) {
        const size_t lds = tpr::tree_lds_bytes(K.M.d, forks, true);
        if (tree_allow_lds(tpr::tree_torque_terms_kernel<true>, lds, g_terms_fused_lds) != 0) return -3;
        hipLaunchKernelGGL(tpr::tree_torque_terms_kernel<true>, grid, block, lds, stream, K);
    } else {
        const size_t lds = tpr::tree_lds_bytes(K.M.d, forks, false);
        if (tree_allow_lds(tpr::tree_torque_terms_kernel<false>, lds, g_terms_serial_lds) != 0) return -3;
        hipLaunchKernelGGL(tpr::tree_torque_terms_kernel<false>, grid, block, lds, stream, K);
    }
    return 0;
}

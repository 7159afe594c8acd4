// tpr_mount_tu.hip -- translation unit of the base-reaction kernels (tpr_mount.hip.inc): the wrench a robot's mount exerts on it,
// and the three evaluations of a constraint on that wrench in one pass.  build.py compiles it in parallel with the other units.
// Two entry points, declared in tpr_kernels.hip; each takes the argument block with the kernels' tables in it (A->T, built and
// validated by the C-ABI entry) and their fork count, and returns 0 = launched, -1 = a dof outside 1 .. 32 or a fork count
// outside 0 .. 4 (they size the LDS), -3 = the LDS could not be reserved.
#include "tpr_chain_launch.hpp"
#include "tpr_mount.hip.inc"

static_assert(sizeof(tpr_mount) == sizeof(tpr::MountFrame) && offsetof(tpr_mount, mass) == offsetof(tpr::MountFrame, mass), "tpr_mount is MountFrame");

using tpr::chain_allow_lds;
using tpr::chain_blocks;

namespace {
std::atomic<unsigned long long> g_wrench_lds{0}, g_terms_lds{0};

inline bool mount_shape_ok(int d, int forks) { return tpr::chain_dof_ok(d) && forks >= 0 && forks <= tpr::kTreeMaxForks; }
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_mount_wrench_launch(const tpr::MountWrenchArgs *A, int forks, hipStream_t stream) {
    if (!mount_shape_ok(A->M.d, forks)) return -1;
    const size_t lds = tpr::mount_lds_bytes(A->M.d, forks, false);
    if (chain_allow_lds(tpr::mount_wrench_kernel, lds, g_wrench_lds) != 0) return -3;
    hipLaunchKernelGGL(tpr::mount_wrench_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), lds, stream, *A);
    return 0;
}

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_mount_wrench_terms_launch(const tpr::MountWrenchTermsArgs *A, int forks, hipStream_t stream) {
    if (!mount_shape_ok(A->M.d, forks)) return -1;
    const size_t lds = tpr::mount_lds_bytes(A->M.d, forks, true);
    if (chain_allow_lds(tpr::mount_wrench_terms_kernel, lds, g_terms_lds) != 0) return -3;
    hipLaunchKernelGGL(tpr::mount_wrench_terms_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), lds, stream, *A);
    return 0;
}

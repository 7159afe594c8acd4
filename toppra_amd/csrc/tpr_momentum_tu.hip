// tpr_momentum_tu.hip -- translation unit of the momentum kernel (tpr_momentum.hip.inc): the momentum and kinetic energy a set of
// a robot's links carries per unit of path velocity, and the bound on sd^2 that limits on them imply.  build.py compiles it in
// parallel with the other units.
// One entry point, declared in tpr_kernels.hip; it takes the argument block with the kernel's tables in it (A->T, built and
// validated by the C-ABI entry) and the number of forks the walk reaches, and returns 0 = launched, -1 = a dof outside 1 .. 32, a
// walk longer than the dof or a fork count outside 0 .. 4 (they size the LDS), -3 = the LDS could not be reserved.
#include "tpr_chain_launch.hpp"
#include "tpr_momentum.hip.inc"

using tpr::chain_allow_lds;
using tpr::chain_blocks;

namespace {
std::atomic<unsigned long long> g_momentum_lds{0};
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_momentum_launch(const tpr::MomentumArgs *A, int forks, hipStream_t stream) {
    if (!tpr::chain_dof_ok(A->M.d) || A->nlinks < 1 || A->nlinks > A->M.d || forks < 0 || forks > tpr::kTreeMaxForks) return -1;
    const size_t lds = tpr::momentum_lds_bytes(A->M.d, forks);
    if (chain_allow_lds(tpr::momentum_kernel, lds, g_momentum_lds) != 0) return -3;
    hipLaunchKernelGGL(tpr::momentum_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), lds, stream, *A);
    return 0;
}

// tpr_effmass_tu.hip -- translation unit of the effective-mass kernel (tpr_effmass.hip.inc): the squared speed of control points
// on a chain or tree, the robot's mobility along a contact force there, and the bound on sd^2 that a cap on the energy a contact can
// transfer implies.  build.py compiles it in parallel with the other units.
// One entry point, declared in tpr_kernels.hip; it takes the argument block with the kernel's tables in it (A->T, A->active, A->own,
// A->walk: built and validated by the C-ABI entry) and the tree's fork count, and returns 0 = launched, -1 = a dof outside 1 .. 32,
// a point count outside 1 .. 16 or a fork count outside 0 .. 4 (they size the LDS), -3 = the LDS could not be reserved.
#include "tpr_chain_launch.hpp"
#include "tpr_effmass.hip.inc"

using tpr::chain_allow_lds;
using tpr::chain_blocks;

namespace {
std::atomic<unsigned long long> g_effmass_lds{0};
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_effmass_launch(const tpr::EffMassArgs *A, int forks, hipStream_t stream) {
    if (!tpr::chain_dof_ok(A->M.d) || A->P.count < 1 || A->P.count > tpr::kChainMaxPoints || forks < 0 || forks > tpr::kTreeMaxForks) return -1;
    const size_t lds = tpr::effmass_lds_bytes(A->M.d, A->P.count, forks);
    if (chain_allow_lds(tpr::effective_mass_kernel, lds, g_effmass_lds) != 0) return -3;
    hipLaunchKernelGGL(tpr::effective_mass_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), lds, stream, *A);
    return 0;
}

// tpr_chain_tu.hip -- translation unit of the rigid-body chain kernels (tpr_chain.hip.inc): inverse dynamics, the three
// evaluations of a torque constraint in one pass, the tool point's velocity and acceleration, the wrench on a carried body,
// speed and acceleration of control points on any link.  build.py compiles it in parallel with the other units.  Nine entry
// points, declared in tpr_kernels.hip; each returns 0 = launched, -1 = no kernel for this dof (or this point set).
#include "tpr_chain_launch.hpp"
#include "tpr_chain.hip.inc"

using tpr::chain_allow_lds;
using tpr::chain_blocks;
using tpr::chain_launch;

namespace {
std::atomic<unsigned long long> g_dyn_lds{0}, g_terms_fused_lds{0}, g_terms_serial_lds{0};
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_chain_dynamics_launch(const tpr::ChainDynArgs *A, hipStream_t stream) {
    const dim3 grid(chain_blocks(A->npoints)), block(tpr::kChainBlock);
    switch (A->M.d) {
#define TPR_CHAIN_CASE(DD) case DD: hipLaunchKernelGGL(tpr::chain_inverse_dynamics_kernel<DD>, grid, block, 0, stream, *A); return 0
        TPR_CHAIN_CASE(1); TPR_CHAIN_CASE(2); TPR_CHAIN_CASE(3); TPR_CHAIN_CASE(4);
        TPR_CHAIN_CASE(5); TPR_CHAIN_CASE(6); TPR_CHAIN_CASE(7); TPR_CHAIN_CASE(8);
#undef TPR_CHAIN_CASE
    }
    if (!tpr::chain_dof_ok(A->M.d)) return -1;
    const size_t lds = (size_t)A->M.d * tpr::kChainSlotsSingle * tpr::kChainBlock * sizeof(double);
    if (chain_allow_lds(tpr::chain_inverse_dynamics_lds_kernel, lds, g_dyn_lds) != 0) return -1;
    hipLaunchKernelGGL(tpr::chain_inverse_dynamics_lds_kernel, grid, block, lds, stream, *A);
    return 0;
}

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_chain_terms_launch(const tpr::ChainTermsArgs *A, hipStream_t stream) {
    const dim3 grid(chain_blocks(A->npoints)), block(tpr::kChainBlock);
    switch (A->M.d) {
#define TPR_CHAIN_CASE(DD) case DD: hipLaunchKernelGGL(tpr::chain_torque_terms_kernel<DD>, grid, block, 0, stream, *A); return 0
        TPR_CHAIN_CASE(1); TPR_CHAIN_CASE(2); TPR_CHAIN_CASE(3); TPR_CHAIN_CASE(4);
        TPR_CHAIN_CASE(5); TPR_CHAIN_CASE(6); TPR_CHAIN_CASE(7); TPR_CHAIN_CASE(8);
#undef TPR_CHAIN_CASE
    }
    if (!tpr::chain_dof_ok(A->M.d)) return -1;
    const size_t per_slot = (size_t)A->M.d * tpr::kChainBlock * sizeof(double);
    if (per_slot * tpr::kChainSlotsFused <= (size_t)tpr::kChainLdsBytes) {
        const size_t lds = per_slot * tpr::kChainSlotsFused;
        if (chain_allow_lds(tpr::chain_torque_terms_lds_kernel<true>, lds, g_terms_fused_lds) != 0) return -1;
        hipLaunchKernelGGL(tpr::chain_torque_terms_lds_kernel<true>, grid, block, lds, stream, *A);
    } else {
        const size_t lds = per_slot * tpr::kChainSlotsSingle;
        if (chain_allow_lds(tpr::chain_torque_terms_lds_kernel<false>, lds, g_terms_serial_lds) != 0) return -1;
        hipLaunchKernelGGL(tpr::chain_torque_terms_lds_kernel<false>, grid, block, lds, stream, *A);
    }
    return 0;
}

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_chain_tool_launch(const tpr::ChainToolArgs *A, hipStream_t stream) {
    return chain_launch(tpr::chain_tool_velocity_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), 0, stream, *A);
}

// (the tool-acceleration kernels' staging area is at most 3 * 64 * 33 doubles = 50 688 bytes at 32 dof: under the 64 KB any kernel may take)
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_chain_accel_launch(const tpr::ChainAccelArgs *A, hipStream_t stream) {
    return chain_launch(tpr::chain_tool_accel_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), tpr::chain_accel_lds_bytes(A->M.d, 1), stream, *A);
}

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_chain_accel_terms_launch(const tpr::ChainAccelTermsArgs *A, hipStream_t stream) {
    return chain_launch(tpr::chain_tool_accel_terms_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), tpr::chain_accel_lds_bytes(A->M.d, 2), stream, *A);
}

// (the wrench kernels stage the same three inputs; their three 6-wide outputs take 10 752 bytes: the same 50 688 at 32 dof)
static_assert(tpr::chain_accel_lds_bytes(TPR_MAX_DOF, 3) <= 64 * 1024, "the wrench kernels' staging area fits an unattributed launch");

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_chain_wrench_launch(const tpr::ChainWrenchArgs *A, hipStream_t stream) {
    return chain_launch(tpr::chain_tool_wrench_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), tpr::chain_accel_lds_bytes(A->M.d, 1), stream, *A);
}

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_chain_wrench_terms_launch(const tpr::ChainWrenchTermsArgs *A, hipStream_t stream) {
    return chain_launch(tpr::chain_tool_wrench_terms_kernel, dim3(chain_blocks(A->npoints)), dim3(tpr::kChainBlock), tpr::chain_accel_lds_bytes(A->M.d, 3), stream, *A);
}

// ---- control points: the launchers find the deepest link that carries a point (the kernels' loops end there); the set is
// validated by the C-ABI entries, and once more here because the kernels index LDS and the outputs by it.
static_assert(TPR_CHAIN_MAX_POINTS == tpr::kChainMaxPoints && sizeof(tpr_chain_points) == sizeof(tpr::ChainPoints), "tpr_chain_points is ChainPoints");
static_assert(tpr::chain_points_lds_bytes(TPR_CHAIN_MAX_POINTS, 2) <= 64 * 1024, "the control-point kernels' LDS fits an unattributed launch");
namespace {
int chain_points_links(const tpr::ChainPoints &P, int d) {
    if (!tpr::chain_dof_ok(d) || P.count < 1 || P.count > tpr::kChainMaxPoints) return -1;
    int deepest = 0;
    for (int p = 0; p < P.count; ++p) {
        if (P.link[p] < 0 || P.link[p] >= d) return -1;
        if (P.link[p] > deepest) deepest = P.link[p];
    }
    return deepest + 1;
}
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_chain_points_speed_launch(const tpr::ChainPointsSpeedArgs *A, hipStream_t stream) {
    tpr::ChainPointsSpeedArgs K = *A;
    if ((K.nlinks = chain_points_links(K.P, K.M.d)) < 0) return -1;
    return chain_launch(tpr::chain_points_speed_kernel, dim3(chain_blocks(K.npoints)), dim3(tpr::kChainBlock), 0, stream, K);
}

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_chain_points_accel_launch(const tpr::ChainPointsAccelArgs *A, int terms, hipStream_t stream) {
    tpr::ChainPointsAccelArgs K = *A;
    if ((K.nlinks = chain_points_links(K.P, K.M.d)) < 0) return -1;
    return chain_launch(terms ? tpr::chain_points_accel_terms_kernel : tpr::chain_points_accel_kernel, dim3(chain_blocks(K.npoints)),
                        dim3(tpr::kChainBlock), tpr::chain_points_lds_bytes(K.P.count, terms ? 2 : 1), stream, K);
}

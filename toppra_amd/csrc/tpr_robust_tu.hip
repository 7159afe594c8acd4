// tpr_robust_tu.hip -- translation unit of the robust (conic) kernels (tpr_robust.hip.inc).
//
// build.py compiles this file twice (-DTPR_TU_HALF=0: the generic lane kernel and 1..8 dof on 8 lanes per trajectory;
// =1: 9..16 dof on 16 lanes), in parallel with the other units.  One entry point per half, declared in tpr_kernels.hip.
#include <hip/hip_runtime.h>

#include "../../include/toppra_hip.h"
#include "tpr_device.hpp"
#include "tpr_lane.hip.inc"
#include "tpr_group.hip.inc"
#include "tpr_robust.hip.inc"

#ifndef TPR_TU_HALF
#error "compile with -DTPR_TU_HALF=0|1"
#endif

namespace {
// 0 = launched; 1 = this shape needs the lane kernel (very long spline tables: this kernel has no table-in-global form)
template <int D, int L>
int robust_launch_group(const tpr::RobustArgs &P, hipStream_t stream) {
    const tpr::GroupLaunch g = tpr::group_launch_geometry<D, L>(P.A.B, P.A.nseg);
    if (!g.table_in_lds) return 1;
    hipLaunchKernelGGL((tpr::group_robust_kernel<D, L>), dim3(g.blocks), dim3(g.threads), g.lds, stream, P);
    return 0;
}
}  // namespace

// 0 = launched; 1 = this shape needs the lane kernel (tpr_tu_robust_lane_launch); -1 = dof not served by this half
#if TPR_TU_HALF == 0
#define TPR_TU_ROBUST_LAUNCH tpr_tu_robust_launch_lo
constexpr int kDofLo = 1, kDofHi = 8;
#else
#define TPR_TU_ROBUST_LAUNCH tpr_tu_robust_launch_hi
constexpr int kDofLo = 9, kDofHi = 16;
#endif
extern "C" __attribute__((visibility("hidden"))) int TPR_TU_ROBUST_LAUNCH(const tpr::RobustArgs *P, hipStream_t stream) {
    return tpr::for_dof<kDofLo, kDofHi>(P->A.d, -1, [&](auto D, auto L) { return robust_launch_group<D(), L()>(*P, stream); });
}
#if TPR_TU_HALF == 0
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_robust_lane_launch(const tpr::RobustArgs *P, hipStream_t stream) {
    hipLaunchKernelGGL(tpr::robust_solve_kernel, dim3((P->A.B + 63) / 64), dim3(64), 0, stream, *P);
    return 0;
}
#endif

// tpr_boxed_args.hpp -- argument blocks of the stage-box kernel (tpr_boxes.hip.inc) and of the dense-row passes on path
// samples + stage boxes (tpr_boxed_stage.hip.inc), shared with the C-ABI entries in tpr_kernels.hip.
#pragma once
#include <cstdint>
#include "tpr_dense_args.hpp"
namespace tpr {
constexpr int kBoxesMaxSources = 8;  // TPR_BOUND_MAX_SOURCES

// The sampled passes with the per-stage variable box read from arrays: low, high [B][N+1][2] set (what tpr_stage_boxes_batch
// writes), vlim null -- the box carries every first-order constraint.  A type of its own so that dense_launch and
// lane_dense_reachable_kernel dispatch on it.
struct BoxedArgs : SampledArgs {};

// One bound source of tpr_stage_boxes_batch with a device pointer.
struct BoxSource {
    int kind, flags;     // TPR_BOUND_*
    const double *data;
};

struct BoxesArgs {
    int B, N, d, nsrc;
    int tile;            // gridpoints per block
    int dp;              // d | 1: row pitch of a gridpoint's fp32 quotients in LDS
    const double *qs;    // [B][N+1][d] (null without a VLIM* source)
    double *low, *high;  // [B][N+1][2]
    BoxSource src[kBoxesMaxSources];
};
}  // namespace tpr

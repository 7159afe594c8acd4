// tpr_boxed_tu.hip -- translation unit of the stage-box kernel (tpr_boxes.hip.inc) and of the dense-row kernels instantiated
// with BoxedSampledStage (tpr_boxed_stage.hip.inc): the passes of tpr_*_sampled_boxed_batch, a stage's rows generated from
// path samples and its variable box read from arrays.  build.py compiles it in parallel with the other units.  Two entry
// points, declared in tpr_kernels.hip.
#include <hip/hip_runtime.h>

#include "../../include/toppra_hip.h"
#include "tpr_device.hpp"
#include "tpr_group.hip.inc"
#include "tpr_dense_args.hpp"
#include "tpr_dense.hip.inc"
#include "tpr_boxed_stage.hip.inc"
#include "tpr_boxes.hip.inc"

// The same passes with the rows generated from path samples and the stage boxes read (BoxedSampledStage).
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_boxed_launch(const tpr::BoxedArgs *A, int feasible, hipStream_t stream) {
    return tpr::dense_dispatch<tpr::BoxedSampledStage>(*A, feasible, stream);
}

// Tile and LDS of the box kernel: up to kBoxesTile gridpoints per block, halved until the two fp32 candidate arrays
// [tile][d | 1] stay within 48 KB.  0 = launched, -1 = one gridpoint's candidates do not fit, -2 = more than 2^31 - 1
// gridpoints in the batch.
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_stage_boxes_launch(tpr::BoxesArgs *A, hipStream_t stream) {
    const long long total = (long long)A->B * (A->N + 1);
    if (total > 0x7fffffffLL) return -2;
    A->dp = A->d | 1;
    int tile = tpr::kBoxesTile;
    bool vel = false;
    for (int j = 0; j < A->nsrc; ++j) vel |= A->src[j].kind == TPR_BOUND_VLIM || A->src[j].kind == TPR_BOUND_VLIM_GRID;
    if (!vel) A->dp = 1;  // (no candidates: the LDS stays unused)
    while (tile > 1 && (size_t)2 * tile * A->dp * sizeof(float) > 48 * 1024) tile /= 2;
    const size_t lds = (size_t)2 * tile * A->dp * sizeof(float);
    if (lds > 64 * 1024) return -1;
    A->tile = tile;
    hipLaunchKernelGGL(tpr::stage_boxes_kernel, dim3((unsigned)((total + tile - 1) / tile)), dim3(256), lds, stream, *A);
    return 0;
}

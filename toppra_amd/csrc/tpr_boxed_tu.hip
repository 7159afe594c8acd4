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

// The (D, L) table of tpr_sampled_tu.hip: nC = 2 + (4 | 2 | 0) d by the flags, same layouts.
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_boxed_launch(const tpr::BoxedArgs *A, int feasible, hipStream_t stream) {
    const int D = A->nC <= 6 ? 1 : (A->nC - 2 + 3) / 4;
    switch (D) {
#define TPR_BOXED_CASE(DD, LL) case DD: return tpr::dense_launch<DD, LL, tpr::BoxedSampledStage<DD, LL>>(*A, feasible, stream)
        TPR_BOXED_CASE(1, 8); TPR_BOXED_CASE(2, 8); TPR_BOXED_CASE(3, 8); TPR_BOXED_CASE(4, 8);
        TPR_BOXED_CASE(5, 8); TPR_BOXED_CASE(6, 8); TPR_BOXED_CASE(7, 8); TPR_BOXED_CASE(8, 8);
        TPR_BOXED_CASE(9, 16); TPR_BOXED_CASE(10, 16); TPR_BOXED_CASE(11, 16); TPR_BOXED_CASE(12, 16);
        TPR_BOXED_CASE(13, 16); TPR_BOXED_CASE(14, 16); TPR_BOXED_CASE(15, 16); TPR_BOXED_CASE(16, 16);
        TPR_BOXED_CASE(17, 32); TPR_BOXED_CASE(18, 32); TPR_BOXED_CASE(19, 32); TPR_BOXED_CASE(20, 32);
        TPR_BOXED_CASE(21, 32); TPR_BOXED_CASE(22, 32); TPR_BOXED_CASE(23, 32); TPR_BOXED_CASE(24, 32);
        TPR_BOXED_CASE(25, 32); TPR_BOXED_CASE(26, 32); TPR_BOXED_CASE(27, 32); TPR_BOXED_CASE(28, 32);
        TPR_BOXED_CASE(29, 32); TPR_BOXED_CASE(30, 32);
#undef TPR_BOXED_CASE
    }
    return -1;
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

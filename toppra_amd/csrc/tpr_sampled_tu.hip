// tpr_sampled_tu.hip -- translation unit of the dense-row kernels instantiated with SampledStage (tpr_dense.hip.inc): the
// passes of tpr_*_sampled_batch, a stage's rows generated from path samples.  build.py compiles it in parallel with the
// other units.  One entry point, declared in tpr_kernels.hip.
#include <hip/hip_runtime.h>

#include "../../include/toppra_hip.h"
#include "tpr_device.hpp"
#include "tpr_group.hip.inc"
#include "tpr_dense_args.hpp"
#include "tpr_dense.hip.inc"

// The same passes with the rows generated from path samples (SampledStage):
// nC = 2 + (4 | 2 | 0) d by the flags, same layouts.
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_sampled_launch(const tpr::SampledArgs *A, int feasible, hipStream_t stream) {
    const int D = A->nC <= 6 ? 1 : (A->nC - 2 + 3) / 4;
    switch (D) {
#define TPR_SAMPLED_CASE(DD, LL) case DD: return tpr::dense_launch<DD, LL, tpr::SampledStage<DD, LL>>(*A, feasible, stream)
        TPR_SAMPLED_CASE(1, 8); TPR_SAMPLED_CASE(2, 8); TPR_SAMPLED_CASE(3, 8); TPR_SAMPLED_CASE(4, 8);
        TPR_SAMPLED_CASE(5, 8); TPR_SAMPLED_CASE(6, 8); TPR_SAMPLED_CASE(7, 8); TPR_SAMPLED_CASE(8, 8);
        TPR_SAMPLED_CASE(9, 16); TPR_SAMPLED_CASE(10, 16); TPR_SAMPLED_CASE(11, 16); TPR_SAMPLED_CASE(12, 16);
        TPR_SAMPLED_CASE(13, 16); TPR_SAMPLED_CASE(14, 16); TPR_SAMPLED_CASE(15, 16); TPR_SAMPLED_CASE(16, 16);
        TPR_SAMPLED_CASE(17, 32); TPR_SAMPLED_CASE(18, 32); TPR_SAMPLED_CASE(19, 32); TPR_SAMPLED_CASE(20, 32);
        TPR_SAMPLED_CASE(21, 32); TPR_SAMPLED_CASE(22, 32); TPR_SAMPLED_CASE(23, 32); TPR_SAMPLED_CASE(24, 32);
        TPR_SAMPLED_CASE(25, 32); TPR_SAMPLED_CASE(26, 32); TPR_SAMPLED_CASE(27, 32); TPR_SAMPLED_CASE(28, 32);
        TPR_SAMPLED_CASE(29, 32); TPR_SAMPLED_CASE(30, 32);
#undef TPR_SAMPLED_CASE
    }
    return -1;
}

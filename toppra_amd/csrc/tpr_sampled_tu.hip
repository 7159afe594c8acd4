// tpr_sampled_tu.hip -- translation unit of the dense-row kernels instantiated with SampledStage (tpr_dense.hip.inc): the
// passes of tpr_*_sampled_batch, a stage's rows generated from path samples.  build.py compiles it in parallel with the
// other units.  One entry point, declared in tpr_kernels.hip.
#include <hip/hip_runtime.h>

#include "../../include/toppra_hip.h"
#include "tpr_device.hpp"
#include "tpr_group.hip.inc"
#include "tpr_dense_args.hpp"
#include "tpr_dense.hip.inc"

// The same passes with the rows generated from path samples (SampledStage): nC = 2 + (4 | 2 | 0) d by the flags.
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_sampled_launch(const tpr::SampledArgs *A, int feasible, hipStream_t stream) {
    return tpr::dense_dispatch<tpr::SampledStage>(*A, feasible, stream);
}

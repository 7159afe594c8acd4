// tpr_dense_tu.hip -- translation unit of the dense-row kernels (tpr_dense.hip.inc): the reference's seidelWrapper contract
// for ANY canonical-linear constraint set.  build.py compiles it in parallel with the other units.  One entry point,
// declared in tpr_kernels.hip.
#include <hip/hip_runtime.h>

#include "../../include/toppra_hip.h"
#include "tpr_device.hpp"
#include "tpr_group.hip.inc"
#include "tpr_dense_args.hpp"
#include "tpr_dense.hip.inc"

// The passes on rows read from arrays (DenseStage), on the layout dense_dispatch picks for nC.
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_dense_launch(const tpr::DenseArgs *A, int feasible, hipStream_t stream) {
    return tpr::dense_dispatch<tpr::DenseStage>(*A, feasible, stream);
}

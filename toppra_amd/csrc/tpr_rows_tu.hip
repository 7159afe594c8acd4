// tpr_rows_tu.hip -- translation unit of the row-assembly kernels (tpr_rows.hip.inc): the dense problem of a constraint list
// with second-order / torque constraints, and the path at the gridpoints for the inverse dynamics that feed it.  build.py
// compiles it in parallel with the other units.  Three entry points, declared in tpr_kernels.hip.
#include <hip/hip_runtime.h>

#include "../../include/toppra_hip.h"
#include "tpr_rows.hip.inc"

// Tile and LDS of one launch: the largest tile up to kRowsTile whose record -- q', q'' and the blocks' a | b | c at tile + 1
// gridpoints, the tile's deltas, the acceleration limits -- stays within 48 KB (three blocks per CU and more).
// 0 = launched, -1 = one gridpoint's record does not fit, -2 = more than 65535 tiles.
namespace {
template <class Args, class Kernel>
int rows_launch(Kernel kernel, const Args *A, double *a, double *b, double *c, double *low, double *high, double *deltas, hipStream_t stream) {
    const size_t per_point = (size_t)2 * A->d + A->wsum, fixed = (size_t)2 * A->d;
    int cap = tpr::kRowsTile;
    while (cap > 1 && ((cap + 1) * per_point + cap + fixed) * sizeof(double) > 48 * 1024) cap /= 2;
    const size_t lds = ((cap + 1) * per_point + cap + fixed) * sizeof(double);
    if (lds > 64 * 1024) return -1;
    const unsigned tiles = (unsigned)((A->N + 1 + cap - 1) / cap);
    if (tiles > 65535u) return -2;
    const int tile = (int)((A->N + 1 + tiles - 1) / tiles);  // (N + 1) split evenly, as tpr_constraint_params_batch
    hipLaunchKernelGGL(kernel, dim3((unsigned)A->B, tiles), dim3(256), lds, stream, *A, tile, cap, a, b, c, low,
                       high, deltas);
    return 0;
}
}  // namespace

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_rows_launch(const tpr::RowsArgs *A, double *a, double *b, double *c, double *low,
                                                                        double *high, double *deltas, hipStream_t stream) {
    return rows_launch(tpr::second_order_rows_kernel, A, a, b, c, low, high, deltas, stream);
}
// ... for a path given as samples
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_sampled_rows_launch(const tpr::SampledRowsArgs *A, double *a, double *b, double *c,
                                                                                double *low, double *high, double *deltas, hipStream_t stream) {
    return rows_launch(tpr::sampled_rows_kernel, A, a, b, c, low, high, deltas, stream);
}

extern "C" __attribute__((visibility("hidden"))) int tpr_tu_path_eval_launch(const tpr::PathEvalArgs *A, hipStream_t stream) {
    const long long total = (long long)A->B * (A->N + 1) * A->d;  // one thread per (gridpoint, joint)
    if (total > (long long)0x7fffffff * 256) return -1;
    hipLaunchKernelGGL(tpr::path_eval_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, *A);
    return 0;
}

// tpr_chain_launch.hpp -- what the launchers of the rigid-body units (tpr_chain_tu.hip, tpr_tree_tu.hip) share on the host: the
// launch geometry (one wave of 64 points per block), the dof range every launcher guards its LDS size with, and the attribute
// a kernel needs before it may take more than 64 KB of dynamic LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/toppra_hip.h"
#include "tpr_chain_args.hpp"

namespace tpr {
inline unsigned chain_blocks(int npoints) { return (unsigned)(((long long)npoints + kChainBlock - 1) / kChainBlock); }
inline bool chain_dof_ok(int d) { return d >= 1 && d <= TPR_MAX_DOF; }

// The runtime-dof kernels take up to the whole LDS of a CU; above 64 KB a kernel has to be told so, once per device: `done`
// is the kernel's bit mask of the devices that have been told (the attribute is raised to the full 160 KB, so one call serves
// every dof and fork count).
template <class Kernel>
int chain_allow_lds(Kernel kernel, size_t lds, std::atomic<unsigned long long> &done) {
    if (lds > (size_t)kChainLdsBytes) return -1;
    if (lds <= 64 * 1024) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
    if (done.load(std::memory_order_relaxed) >> dev & 1ull) return 0;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kChainLdsBytes) != hipSuccess) return -1;
    done.fetch_or(1ull << dev, std::memory_order_relaxed);
    return 0;
}

// hipLaunchKernelGGL for a kernel that takes its argument block by value, with the launchers' guard in it: 0 once launched, -1
// for a dof outside 1 .. 32 (the dof sizes the dynamic LDS).
template <class Args>
int chain_launch(void (*kernel)(Args), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args &A) {
    if (!chain_dof_ok(A.M.d)) return -1;
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, A);
    return 0;
}
}  // namespace tpr

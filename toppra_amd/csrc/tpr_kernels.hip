// tpr_kernels.hip -- libtoppra_hip.so: HIP kernels + the C-ABI of include/toppra_hip.h (gfx950).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see build.py).
// -ffp-contract=off is a correctness flag, not a tuning knob: see tpr_device.hpp.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/toppra_hip.h"
#include "tpr_device.hpp"
#include "tpr_lane.hip.inc"
#include "tpr_group.hip.inc"
#include "tpr_wave.hip.inc"
#include "tpr_pair.hip.inc"
#include "tpr_spline.hip.inc"
#include "tpr_param.hip.inc"
#include "tpr_robust_args.hpp"
#include "tpr_lane_dense.hip.inc"

// kernel family 3, one translation unit per dof (tpr_cert_tu.hip): 1..TPR_CERT_MAX_DOF (build.py: 15; the measurement builds: 8).
// TPR_CERT_DOFS(X) expands X(d) for every dof linked; it spells the entry points' declarations and the launchers' cases.
#ifndef TPR_CERT_MAX_DOF
#define TPR_CERT_MAX_DOF 15
#endif
#if TPR_CERT_MAX_DOF == 15
#define TPR_CERT_DOFS_ABOVE_8(X) X(9) X(10) X(11) X(12) X(13) X(14) X(15)
#elif TPR_CERT_MAX_DOF == 8
#define TPR_CERT_DOFS_ABOVE_8(X)
#else
#error "TPR_CERT_MAX_DOF: 15 (the product) or 8 (the measurement builds)"
#endif
#define TPR_CERT_DOFS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) TPR_CERT_DOFS_ABOVE_8(X)
#define TPR_CERT_DECLARE(d) \
    __attribute__((visibility("hidden"))) int tpr_tu_cert_launch_##d(const tpr::GroupArgs *, hipStream_t); \
    __attribute__((visibility("hidden"))) int tpr_tu_cert_feasible_launch_##d(const tpr::GroupArgs *, double *, hipStream_t); \
    __attribute__((visibility("hidden"))) int tpr_tu_cert_sd_launch_##d(const tpr::GroupArgs *, hipStream_t);
extern "C" {
__attribute__((visibility("hidden"))) int tpr_tu_dense_launch(const tpr::DenseArgs *, int, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_robust_launch_lo(const tpr::RobustArgs *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_robust_launch_hi(const tpr::RobustArgs *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_robust_lane_launch(const tpr::RobustArgs *, hipStream_t);
TPR_CERT_DOFS(TPR_CERT_DECLARE)
#undef TPR_CERT_DECLARE
}

namespace {

thread_local std::string g_err;
// Default device of host-pointer calls: the calling THREAD's last successful tpr_init, else the process's (a thread
// that never called tpr_init inherits what another one selected).  Both, and the table of verified devices, may be
// touched by several threads working on different GPUs.
std::atomic<int> g_process_device{-1};
thread_local int t_device = -1;
std::atomic<bool> g_checked[64];  // devices already verified to be gfx950
inline int default_device() { return t_device >= 0 ? t_device : g_process_device.load(std::memory_order_relaxed); }

// HIP's current device is per thread and other libraries (torch) move it.  Every entry point runs on
// the device its data lives on -- the device of the pointers with TPR_DEVICE_PTRS, the tpr_init()
// device otherwise -- and puts the caller's current device back on return.
struct DeviceScope {
    int prev = -1, dev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceScope(int want) : dev(want) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
    }
    ~DeviceScope() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
};

// Device a call should run on: the one `device_ptr` lives on (TPR_DEVICE_PTRS), else default_device().
int call_device(bool device_ptrs, const void *device_ptr) {
    if (device_ptrs && device_ptr) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, device_ptr) == hipSuccess && attr.device >= 0) return attr.device;
        (void)hipGetLastError();
    }
    return default_device();
}

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(TPR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

// One C-ABI call: its stream, the device it runs on (DeviceScope) and host<->device staging for callers that hand over
// host buffers.  With TPR_DEVICE_PTRS every pointer passes through untouched and only scratch() allocates.
// `device_ptr`: the pointer whose device the call follows.
struct Staging {
    bool device_ptrs;
    hipStream_t stream;
    DeviceScope scope;
    std::vector<void *> owned;
    struct Out { void *host; void *dev; size_t bytes; };
    std::vector<Out> outs;
    hipError_t err = hipSuccess;

    Staging(bool dev, const void *device_ptr, void *stream_)
        : device_ptrs(dev), stream(static_cast<hipStream_t>(stream_)), scope(call_device(dev, device_ptr)) {}
    ~Staging() {
        for (void *p : owned) (void)hipFreeAsync(p, stream);  // stream-ordered pool: no device sync, memory is reused
    }
    // Stream-ordered memory for `count` T (nullptr for none, or after an error: see `err`).  It joins `owned` at once, so
    // that no early return leaks it.
    template <class T>
    T *scratch(size_t count) {
        void *d = nullptr;
        if (count == 0 || err != hipSuccess) return nullptr;
        err = hipMallocAsync(&d, count * sizeof(T), stream);
        if (err != hipSuccess) return nullptr;
        owned.push_back(d);
        return static_cast<T *>(d);
    }
    template <class T>
    const T *in(const T *p, size_t count) {
        if (!p || device_ptrs || count == 0) return p;
        T *d = scratch<T>(count);
        if (d) err = hipMemcpyAsync(d, p, count * sizeof(T), hipMemcpyHostToDevice, stream);
        return d;
    }
    template <class T>
    T *out(T *p, size_t count, bool copy_in = false) {
        if (!p || device_ptrs || count == 0) return p;
        T *d = scratch<T>(count);
        if (!d) return nullptr;
        if (copy_in) err = hipMemcpyAsync(d, p, count * sizeof(T), hipMemcpyHostToDevice, stream);
        outs.push_back({p, d, count * sizeof(T)});
        return d;
    }
    // TPR_E_HIP once the device could not be selected or an allocation / a copy of the staging has failed
    int failed() const {
        const hipError_t e = scope.err != hipSuccess ? scope.err : err;
        return e == hipSuccess ? TPR_E_OK : fail(TPR_E_HIP, hipGetErrorString(e));
    }
    // The way out of a call that has launched its kernels: their launch errors, then (host buffers) the outputs' copies
    // and the synchronisation.
    int finish() {
        hipError_t e = err;
        if (e == hipSuccess) {
            // a kernel that could not be launched leaves its error in the runtime's per-thread slot only: ask for it on
            // both paths (round 3: a host-buffer call whose launch failed returned uninitialised outputs without a word)
            e = hipGetLastError();
            if (e == hipSuccess && !device_ptrs) {
                for (auto &o : outs) {
                    e = hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, stream);
                    if (e != hipSuccess) break;
                }
                if (e == hipSuccess) e = hipStreamSynchronize(stream);
            }
        }
        return e == hipSuccess ? TPR_E_OK : fail(TPR_E_HIP, std::string("S.finish(): ") + hipGetErrorString(e));
    }
};

int check_problem(const tpr_problem *p) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (!p) return fail(TPR_E_BADARG, "null problem");
    if (p->B < 0 || p->N < 1 || p->nseg < 1) return fail(TPR_E_BADARG, "need B >= 0, N >= 1, nseg >= 1");
    if (p->d < 1 || p->d > TPR_MAX_DOF) return fail(TPR_E_UNSUPPORTED, "dof must be in [1, TPR_MAX_DOF]");
    if (!p->coef || !p->breaks || !p->grid) return fail(TPR_E_BADARG, "coef/breaks/grid are required");
    if ((p->flags & TPR_HAS_VELOCITY) && !p->vlim) return fail(TPR_E_BADARG, "TPR_HAS_VELOCITY without vlim");
    if ((p->flags & TPR_HAS_ACCELERATION) && !p->alim) return fail(TPR_E_BADARG, "TPR_HAS_ACCELERATION without alim");
    return TPR_E_OK;
}

int rows_per_lp(const tpr_problem *p) {
    return 2 + ((p->flags & TPR_HAS_ACCELERATION) ? ((p->flags & TPR_ACC_INTERPOLATION) ? 4 : 2) * p->d : 0);
}

// Element counts of the path's inputs: the cubic pieces [B][4][nseg][d], their breakpoints and the gridpoints, the last
// two shared by the batch unless the flags say per trajectory.
struct PathCounts { size_t coef, breaks, grid; };
PathCounts path_counts(const tpr_problem *p) {
    const size_t B = (size_t)p->B, d = (size_t)p->d, nseg = (size_t)p->nseg, N = (size_t)p->N;
    return {B * 4 * nseg * d, ((p->flags & TPR_BREAKS_PER_TRAJ) ? B : 1) * (nseg + 1), ((p->flags & TPR_GRID_PER_TRAJ) ? B : 1) * (N + 1)};
}
// ... staged into any argument block that names them coef / breaks / grid
template <class Args>
void stage_path(const tpr_problem *p, Staging &S, Args &A) {
    const PathCounts n = path_counts(p);
    A.coef = S.in(p->coef, n.coef);
    A.breaks = S.in(p->breaks, n.breaks);
    A.grid = S.in(p->grid, n.grid);
}

// Stage the inputs of a problem; returns the kernel argument block.
tpr::BatchArgs stage_problem(const tpr_problem *p, Staging &S) {
    tpr::BatchArgs A{};
    const size_t B = (size_t)p->B, d = (size_t)p->d;
    A.B = p->B; A.d = p->d; A.nseg = p->nseg; A.N = p->N; A.flags = p->flags;
    stage_path(p, S, A);
    A.vlim = S.in(p->vlim, B * d * 2);
    A.alim = S.in(p->alim, B * d * 2);
    A.sd_start = S.in(p->sd_start, B);
    A.sd_end = S.in(p->sd_end, B);
    return A;
}

using tpr::kMaxDynamicLds;
// Batch sizes of pick_variant's automatic choices.  Two trajectories per wave (family 5) between these two
// (tools/gpu_crossover.py) ...
constexpr int kPairAutoMinBatch = 2560, kPairAutoMaxBatch = 9215;
// ... one wave per trajectory (family 4) up to this many trajectories (4096: 0.86 vs 1.11 ms for family 2; 8192: 1.51 vs
// 1.31 -- tools/gpu_wave_check.py)
constexpr int kWaveAutoMaxBatch = 5120;

// The argument block of families 2 and 3 from the call's.  (The feasible-sets launchers get sd_end_hi and backward_only
// too: always their defaults there, because tpr_feasible_sets_batch never sets them.)
tpr::GroupArgs group_args(const tpr::BatchArgs &A) {
    return tpr::GroupArgs{A.B, A.nseg, A.N, A.flags, A.coef, A.breaks, A.grid, A.vlim, A.alim,
                          A.sd_start, A.sd_end, A.sd2, A.sd, A.u, A.K, A.status, A.sd_end_hi, A.backward_only};
}

// tpr::for_dof for this unit's launchers: TPR_E_UNSUPPORTED outside 1..16 dof
template <class F>
int dispatch_dof(int d, F &&f) {
    const int rc = tpr::for_dof(d, 1, f);
    return rc == 1 ? fail(TPR_E_UNSUPPORTED, "dof out of range") : rc;
}

// Family 2 (rows across lanes): tpr::group_launch_geometry decides block size and where the spline table lives.
template <int D, int L>
int launch_group(const tpr::BatchArgs &A, hipStream_t stream) {
    const tpr::GroupLaunch g = tpr::group_launch_geometry<D, L>(A.B, A.nseg);
    const tpr::GroupArgs G = group_args(A);
    if (g.table_in_lds) hipLaunchKernelGGL((tpr::group_solve_kernel<D, L, true>), dim3(g.blocks), dim3(g.threads), g.lds, stream, G);
    else hipLaunchKernelGGL((tpr::group_solve_kernel<D, L, false>), dim3(g.blocks), dim3(g.threads), g.lds, stream, G);
    return TPR_E_OK;
}

// The rows-across-lanes kernels cover every constraint set of the path -- acceleration with
// Interpolation (the reference's default) or Collocation or absent, velocity optional -- for every
// supported dof: 8 lanes per trajectory up to d = 8, 16 lanes above.  (Missing acceleration blocks are
// disabled rows in the Interpolation slot layout, see GroupTraj::nblk.)
bool group_supported(const tpr::BatchArgs &A) { return A.d >= 1 && A.d <= TPR_MAX_DOF_FAST; }

// ... the robust kernel and family 3 are written for the full Interpolation row set
bool interp_rows(const tpr::BatchArgs &A) {
    const int need = TPR_HAS_ACCELERATION | TPR_ACC_INTERPOLATION;
    return (A.flags & need) == need;
}

int dispatch_sd_forward(int d, const tpr::SdArgs &A, hipStream_t stream) {
    return dispatch_dof(d, [&](auto D, auto L) {
        const tpr::GroupLaunch g = tpr::group_launch_geometry<D(), L()>(A.B, A.nseg);
        if (g.table_in_lds) hipLaunchKernelGGL((tpr::group_sd_forward_kernel<D(), L(), true>), dim3(g.blocks), dim3(g.threads), g.lds, stream, A);
        else hipLaunchKernelGGL((tpr::group_sd_forward_kernel<D(), L(), false>), dim3(g.blocks), dim3(g.threads), g.lds, stream, A);
        return TPR_E_OK;
    });
}

// The certified lane kernel (family 3) serves the same constraint set up to 15 dof when sd2, u and
// status are requested; the strict mode stays with family 2.
bool cert_supported(const tpr::BatchArgs &A) {
    return group_supported(A) && (A.flags & TPR_HAS_ACCELERATION) && A.d <= TPR_CERT_MAX_DOF &&
           !(A.flags & TPR_STRICT_SEIDEL) && A.N >= 1 && !A.active &&
           (A.backward_only || (A.sd2 && A.u && A.status));
}

// Return codes of the per-dof translation units of family 3: 0, or a negative "this instantiation does not exist".
int cert_tu_rc(int rc) {
    return rc < 0 ? fail(TPR_E_UNSUPPORTED, "kernel family 3: this combination of dof / discretisation / certificate mode is not instantiated") : rc;
}

// Kernel family 3 lives in its own translation units, one per dof (tpr_cert_tu.hip; build.py compiles them in parallel).
int launch_cert(const tpr::BatchArgs &A, hipStream_t stream) {
    const tpr::GroupArgs G = group_args(A);
#define TPR_CERT_CASE(d) case d: return cert_tu_rc(tpr_tu_cert_launch_##d(&G, stream));
    switch (A.d) { TPR_CERT_DOFS(TPR_CERT_CASE) }
#undef TPR_CERT_CASE
    return fail(TPR_E_UNSUPPORTED, "variant 3: dof not instantiated");
}

// compute_feasible_sets on the certified lane design: the constraint sets and dofs of family 3, fresh warm-start state
bool cert_feasible_supported(const tpr::BatchArgs &A) {
    return group_supported(A) && (A.flags & TPR_HAS_ACCELERATION) && A.d <= TPR_CERT_MAX_DOF &&
           !(A.flags & TPR_STRICT_SEIDEL) && !A.active;
}

int launch_cert_feasible(const tpr::BatchArgs &A, double *X, hipStream_t stream) {
    const tpr::GroupArgs G = group_args(A);
#define TPR_CERT_CASE(d) case d: return cert_tu_rc(tpr_tu_cert_feasible_launch_##d(&G, X, stream));
    switch (A.d) { TPR_CERT_DOFS(TPR_CERT_CASE) }
#undef TPR_CERT_CASE
    return fail(TPR_E_UNSUPPORTED, "variant 3: dof not instantiated");
}

// TOPPRAsd on family 3: backward scan and both forward profiles in one launch
int launch_cert_sd(const tpr::BatchArgs &A, double *xf, double *uf, double *xl, double *ul, double *dur, hipStream_t stream) {
    tpr::GroupArgs G = group_args(A);
    G.sd = nullptr; G.sd_end_hi = nullptr; G.backward_only = 0;  // (one launch: the whole backward scan, then the profiles instead of sd)
    G.sd_xf = xf; G.sd_uf = uf; G.sd_xl = xl; G.sd_ul = ul; G.sd_dur = dur;
#define TPR_CERT_CASE(d) case d: return cert_tu_rc(tpr_tu_cert_sd_launch_##d(&G, stream));
    switch (A.d) { TPR_CERT_DOFS(TPR_CERT_CASE) }
#undef TPR_CERT_CASE
    return fail(TPR_E_UNSUPPORTED, "variant 3: dof not instantiated");
}

int dispatch_group_feasible(const tpr::BatchArgs &A, double *X, hipStream_t stream) {
    const tpr::GroupArgs G = group_args(A);
    return dispatch_dof(A.d, [&](auto D, auto L) {
        const tpr::GroupLaunch g = tpr::group_launch_geometry<D(), L()>(A.B, A.nseg);
        if (g.table_in_lds) hipLaunchKernelGGL((tpr::group_feasible_kernel<D(), L(), true>), dim3(g.blocks), dim3(g.threads), g.lds, stream, G, X);
        else hipLaunchKernelGGL((tpr::group_feasible_kernel<D(), L(), false>), dim3(g.blocks), dim3(g.threads), g.lds, stream, G, X);
        return TPR_E_OK;
    });
}

// The robust (conic) kernels live in their own translation units (tpr_robust_tu.hip): 0 = launched, 1 = the shape needs
// the generic lane kernel (very long spline tables), -1 = dof not served.
int dispatch_group_robust(const tpr::RobustArgs &P, hipStream_t stream) {
    int rc = P.A.d <= 8 ? tpr_tu_robust_launch_lo(&P, stream) : tpr_tu_robust_launch_hi(&P, stream);
    if (rc == 1) rc = tpr_tu_robust_lane_launch(&P, stream);
    return rc < 0 ? fail(TPR_E_UNSUPPORTED, "dof out of range") : TPR_E_OK;
}

// Family 4 (one trajectory per wave): every constraint set, every dof; grid, x box and K of the trajectory must
// fit the dynamic LDS of a block (5 (N+1) doubles: N <= 1480; the spline table joins them when there is room).
size_t wave_lds_bytes(const tpr::BatchArgs &A, bool table_in_lds) {
    return tpr::wave_lds_doubles(A.N, A.nseg, A.d, table_in_lds) * sizeof(double);
}
bool wave_supported(const tpr::BatchArgs &A) {
    return A.d >= 1 && A.d <= TPR_MAX_DOF && A.N >= 1 && A.nseg <= 65535 && wave_lds_bytes(A, false) <= kMaxDynamicLds;
}

constexpr int kWaveSplitMaxBatch = 768;  // two waves per trajectory (one per LP of a backward stage) up to this many trajectories
int launch_wave(const tpr::BatchArgs &A, hipStream_t stream) {
    const bool table = wave_lds_bytes(A, true) <= kMaxDynamicLds;
    const size_t lds = wave_lds_bytes(A, table);
    const int slots = (4 * A.d + 6 + 63) / 64;  // virtual rows per LP / 64 lanes
    // a handful of trajectories (BASELINE config 1): the two LPs of a backward stage on two waves (wave_solve_kernel<.., SPLIT>)
    const bool split = slots == 1 && !A.feasible_X && A.B <= kWaveSplitMaxBatch;
    const dim3 grid(A.B), block(split ? 128 : 64);
#define TPR_LAUNCH_WAVE(SS)                                                                                   \
    do {                                                                                                      \
        if (table) hipLaunchKernelGGL((tpr::wave_solve_kernel<SS, true>), grid, block, lds, stream, A);       \
        else hipLaunchKernelGGL((tpr::wave_solve_kernel<SS, false>), grid, block, lds, stream, A);            \
    } while (0)
    if (split) {
        if (table) hipLaunchKernelGGL((tpr::wave_solve_kernel<1, true, true>), grid, block, lds, stream, A);
        else hipLaunchKernelGGL((tpr::wave_solve_kernel<1, false, true>), grid, block, lds, stream, A);
        return TPR_E_OK;
    }
    switch (slots) {
        case 1: TPR_LAUNCH_WAVE(1); break;
        case 2: TPR_LAUNCH_WAVE(2); break;
        case 3: TPR_LAUNCH_WAVE(3); break;
        default: return fail(TPR_E_UNSUPPORTED, "variant 4: dof out of range");
    }
#undef TPR_LAUNCH_WAVE
    return TPR_E_OK;
}

// Family 5 (two trajectories per wave, 32 lanes each): the fused solve for 1..7 dof; both trajectories' LDS tables in one
// block.  Not the wrapper's warm-start state, not the stand-alone backward scan, not feasible sets (family 4 has those).
size_t pair_lds_bytes(const tpr::BatchArgs &A, bool table_in_lds) {
    return 2 * ((tpr::wave_lds_doubles(A.N, A.nseg, A.d, table_in_lds) + 1) & ~(size_t)1) * sizeof(double);
}
bool pair_supported(const tpr::BatchArgs &A) {
    return A.d >= 1 && A.d <= 7 && A.N >= 1 && A.nseg <= 65535 && !A.active && !A.feasible_X && !A.backward_only && !A.sd_end_hi &&
           pair_lds_bytes(A, false) <= kMaxDynamicLds;
}
int launch_pair(const tpr::BatchArgs &A, hipStream_t stream) {
    const bool table = pair_lds_bytes(A, true) <= kMaxDynamicLds;
    const size_t lds = pair_lds_bytes(A, table);
    const dim3 grid((A.B + 1) / 2), block(64);
    if (table) hipLaunchKernelGGL((tpr::pair_solve_kernel<true>), grid, block, lds, stream, A);
    else hipLaunchKernelGGL((tpr::pair_solve_kernel<false>), grid, block, lds, stream, A);
    return TPR_E_OK;
}

// Batch size from which family 3 is the automatic choice (solve, TOPPRAsd).
// (measured against family 2, 9..14 dof: tools/gpu_crossover_slim.py, profiles/r06_crossover_9_14_dof.log)
int cert_auto_from(int d) { return d <= 8 ? 9216 : (d <= 10 ? 14336 : (d == 11 ? 15360 : (d == 12 ? 17408 : (d == 13 ? 22528 : (d == 14 ? 27648 : 36864))))); }

// Kernel family of a solve (tpr_problem.variant 0 = auto).
int pick_variant(int requested, const tpr::BatchArgs &A) {
    if (requested != 0) return requested;
    // the wrapper object's warm-start state in / out: family 4 maintains it, and so does the generic lane kernel (family 1)
    // for what family 4 cannot take (N > 1480); families 2 and 3 neither read nor update it
    if (A.active) return wave_supported(A) ? 4 : 1;
    // Batches that cannot fill the chip are bound by the latency of a trajectory's 3N sequential stage LPs: one
    // wave per trajectory (family 4).  Family 3 finishes up to 65536 trajectories (one wave per SIMD) in one
    // fixed-latency round, which beats family 2's throughput from about a quarter of that batch upward
    // (tools/gpu_crossover.py); family 2 serves the strict mode and what is left.
    // ... two trajectories per wave (family 5) from the batch size at which one wave per trajectory stops being free: the
    // chip holds 1024 waves at one per SIMD, and family 4's waves leave half their lanes idle at <= 7 dof
    // (... while eight blocks still fit a CU's LDS -- two waves per SIMD, all a 4096-trajectory batch can use: N <= ~240 at 7 dof)
    if (pair_supported(A) && A.B >= kPairAutoMinBatch && A.B <= kPairAutoMaxBatch && pair_lds_bytes(A, true) <= 160 * 1024 / 8) return 5;
    if (wave_supported(A) && A.B <= kWaveAutoMaxBatch) return 4;
    // (round 4, after families 2 and 4 learnt to follow the lower-bound trace too: at 7 dof family 2 leads between ~5600 and
    // ~9200 trajectories, 1.7 - 1.9 ms against family 3's 2.1 - 2.2 at any size up to 65536; the slim blocks of 9..13 dof
    // take 3.2 - 4.4 ms for a partial round and pay from ~18000 / ~22000 trajectories: profiles/r04_family_crossover.log)
    if (cert_supported(A) && A.B >= cert_auto_from(A.d)) return 3;
    return group_supported(A) ? 2 : (wave_supported(A) ? 4 : 1);
}

int launch_solve(const tpr_problem *p, const tpr::BatchArgs &A, hipStream_t stream) {
    if (A.B == 0) return TPR_E_OK;
    const int variant = pick_variant(p->variant, A);
    if (A.active && (variant == 2 || variant == 3))
        return fail(TPR_E_UNSUPPORTED, "tpr_problem.active (warm-start state in / out) is maintained by kernel families 4 and 1 only: leave variant at 0");
    switch (variant) {
        case 5: {
            if (!pair_supported(A))
                return fail(TPR_E_UNSUPPORTED, "variant 5 (two trajectories per wave) serves the fused solve for 1..7 dof with N <= ~800 and no warm-start state");
            return launch_pair(A, stream);
        }
        case 4: {
            if (!wave_supported(A)) return fail(TPR_E_UNSUPPORTED, "variant 4: N too large for the per-trajectory LDS tables (N <= 1480)");
            return launch_wave(A, stream);
        }
        case 3: {
            if (!cert_supported(A))
                return fail(TPR_E_UNSUPPORTED, "variant 3 needs an acceleration constraint, d <= 15, sd2/u/status outputs, no strict mode");
            return launch_cert(A, stream);
        }
        case 2: {
            if (!group_supported(A)) return fail(TPR_E_UNSUPPORTED, "variant 2: dof out of range");
            // up to 8 dof a trajectory fits 8 lanes; batches that leave most SIMDs idle at that width
            // (<= 8192 trajectories = 1024 waves) run 16 lanes per trajectory: 1.42 -> 1.15 ms at 4096 x 7 x 200
            const bool wide = A.B <= 8192;
            return dispatch_dof(A.d, [&](auto D, auto L) {
                if constexpr (L() == 8)
                    if (wide) return launch_group<D(), 16>(A, stream);
                return launch_group<D(), L()>(A, stream);
            });
        }
        case 1: {
            const int block = 64;
            if (A.backward_only)  // compute_controllable_sets on its own
                hipLaunchKernelGGL(tpr::lane_controllable_kernel, dim3((A.B + block - 1) / block), dim3(block), 0, stream, A,
                                   A.sd_end, A.sd_end_hi ? A.sd_end_hi : A.sd_end);
            else
                hipLaunchKernelGGL(tpr::lane_solve_kernel, dim3((A.B + block - 1) / block), dim3(block), 0, stream, A);
            return TPR_E_OK;
        }
        default:
            return fail(TPR_E_UNSUPPORTED, "unknown kernel variant");
    }
}

// Host-buffer calls on a handful of trajectories (the reference's own use: ONE trajectory per
// compute_parameterization call) are all latency.  Instead of a dozen stream-ordered allocations and pageable copies
// they go through one page-locked, device-mapped arena per calling thread: the inputs are packed into it by the CPU,
// the kernel reads them over PCIe (every input is fetched once, by coalesced loads issued together) and writes its
// outputs straight back into it; one launch, one stream synchronisation, two memcpy's on the host.
constexpr int kNotSmall = 1;
constexpr size_t kSmallCallBytes = 1 << 20;
struct HostArena {
    void *ptr = nullptr;
    size_t cap = 0;
    int device = -1;
};
thread_local HostArena g_arena;  // (never freed: a thread's exit may come after the runtime's own teardown)

int solve_small_host_call(const tpr_problem *p, const tpr_result *r, hipStream_t stream, int device) {
    const size_t B = (size_t)p->B, d = (size_t)p->d, N = (size_t)p->N;
    const PathCounts path = path_counts(p);
    struct Piece { const void *src; void *dst; size_t bytes, off; };
    Piece in[7] = {{p->coef, nullptr, path.coef * 8, 0}, {p->breaks, nullptr, path.breaks * 8, 0}, {p->grid, nullptr, path.grid * 8, 0},
                   {p->vlim, nullptr, B * d * 16, 0}, {p->alim, nullptr, B * d * 16, 0},
                   {p->sd_start, nullptr, B * 8, 0}, {p->sd_end, nullptr, B * 8, 0}};
    Piece out[6] = {{nullptr, r->sd2, B * (N + 1) * 8, 0}, {nullptr, r->sd, B * (N + 1) * 8, 0}, {nullptr, r->u, B * N * 8, 0},
                    {nullptr, r->K, B * (N + 1) * 16, 0}, {nullptr, r->status, B * 4, 0},
                    {p->active, p->active, B * 16, 0}};  // (in and out)
    size_t total = 0;
    for (auto &q : in) { q.off = total; if (q.src) total += (q.bytes + 15) & ~(size_t)15; }
    for (auto &q : out) { q.off = total; if (q.dst) total += (q.bytes + 15) & ~(size_t)15; }
    if (total > kSmallCallBytes) return kNotSmall;
    tpr::BatchArgs A{};
    A.B = p->B; A.d = p->d; A.nseg = p->nseg; A.N = p->N; A.flags = p->flags;
    A.sd2 = r->sd2; A.sd = r->sd; A.u = r->u; A.K = r->K; A.status = r->status;  // (what is asked for decides the family)
    A.active = p->active;
    if (pick_variant(p->variant, A) != 4) return kNotSmall;  // the other families want workspaces: the general path
    if (g_arena.cap < total || g_arena.device != device) {
        if (g_arena.ptr) (void)hipHostFree(g_arena.ptr);
        g_arena = HostArena{};
        void *mem = nullptr;
        const size_t cap = total > (size_t)(256 << 10) ? kSmallCallBytes : (size_t)(256 << 10);
        if (hipHostMalloc(&mem, cap, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return kNotSmall; }
        g_arena.ptr = mem; g_arena.cap = cap; g_arena.device = device;
    }
    char *base = static_cast<char *>(g_arena.ptr);
    for (auto &q : in) if (q.src) std::memcpy(base + q.off, q.src, q.bytes);
    if (out[5].src) std::memcpy(base + out[5].off, out[5].src, out[5].bytes);
    auto at = [&](const Piece &q) { return reinterpret_cast<double *>(base + q.off); };
    A.coef = at(in[0]); A.breaks = at(in[1]); A.grid = at(in[2]);
    A.vlim = in[3].src ? at(in[3]) : nullptr; A.alim = in[4].src ? at(in[4]) : nullptr;
    A.sd_start = in[5].src ? at(in[5]) : nullptr; A.sd_end = in[6].src ? at(in[6]) : nullptr;
    A.sd2 = out[0].dst ? at(out[0]) : nullptr; A.sd = out[1].dst ? at(out[1]) : nullptr;
    A.u = out[2].dst ? at(out[2]) : nullptr; A.K = out[3].dst ? at(out[3]) : nullptr;
    A.status = out[4].dst ? reinterpret_cast<int32_t *>(base + out[4].off) : nullptr;
    A.active = out[5].dst ? reinterpret_cast<int32_t *>(base + out[5].off) : nullptr;
    if (int rc = launch_solve(p, A, stream)) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    for (auto &q : out) if (q.dst) std::memcpy(q.dst, base + q.off, q.bytes);
    return TPR_E_OK;
}

// TOPPRAsd's workspace: the fastest / slowest profiles (x [B][N+1], u [B][N] each), `extra` more doubles per trajectory
// behind them (what an entry needs besides: an alpha array the caller did not give, family 3's durations), the
// bisection's worklist with its counter, and a status array when the caller wants none.
struct SdWork {
    double *xf = nullptr, *uf = nullptr, *xl = nullptr, *ul = nullptr, *extra = nullptr;
    int32_t *wlist = nullptr;
};
SdWork sd_workspace(Staging &S, size_t B, size_t N, size_t extra, int32_t *&status) {
    SdWork W;
    const size_t per = 2 * (N + 1) + 2 * N;
    double *ws = S.scratch<double>(B * (per + extra) + 1);
    W.wlist = S.scratch<int32_t>(B + 2);
    if (!status) status = S.scratch<int32_t>(B + 1);
    if (ws) { W.xf = ws; W.uf = ws + B * (N + 1); W.xl = ws + B * (2 * N + 1); W.ul = ws + B * (3 * N + 2); W.extra = ws + B * per; }
    return W;
}

// ... and its last step, from the two profiles of W to the blend: G carries the call's sizes, steps (grid or deltas),
// desired durations and outputs.  `dur`: the profiles' durations [B][2] when the forward scans summed them, else nullptr.
int launch_sd_finish(tpr::SdBlendArgs G, const SdWork &W, const double *dur, hipStream_t stream) {
    const size_t B = (size_t)G.B;
    int32_t *wlist = W.wlist;
    G.xf = W.xf; G.uf = W.uf; G.xl = W.xl; G.ul = W.ul;
    const size_t finish_lds = 5 * ((size_t)G.N + 1) * sizeof(double);
    if (finish_lds <= kMaxDynamicLds) {
        // one wave per trajectory: durations, bisection and the blend from LDS-resident profiles
        G.dur = dur;  // (the three-kernel path below computes its own)
        hipLaunchKernelGGL(tpr::sd_finish_kernel, dim3(G.B), dim3(64), finish_lds, stream, G);
    } else {
        HIP_TRY(hipMemsetAsync(wlist + B, 0, sizeof(int32_t), stream));  // the worklist's counter sits behind it
        hipLaunchKernelGGL(tpr::sd_decide_kernel, dim3((G.B + 63) / 64), dim3(64), 0, stream, G, wlist, wlist + B);
        hipLaunchKernelGGL(tpr::sd_bisect_kernel, dim3((G.B + 63) / 64), dim3(64), 0, stream, G, wlist, wlist + B);
        hipLaunchKernelGGL(tpr::sd_blend_kernel, dim3(G.B), dim3(64), 0, stream, G);
    }
    return TPR_E_OK;
}

// compute_reachable_sets around either lane kernel, once the problem is staged in A: the rest of the entry point
template <class Args>
int reachable_sets(Staging &S, const Args &A, void (*kernel)(Args, const double *, const double *, double *, double *),
                   const double *sdmin, const double *sdmax, double *L, double *X) {
    const size_t B = (size_t)A.B, N = (size_t)A.N;
    const double *dmin = S.in(sdmin, B), *dmax = S.in(sdmax, B);
    double *dL = S.out(L, B * (N + 1) * 2);
    double *dX = S.out(X, B * (N + 1) * 2);
    if (!dX) dX = S.scratch<double>(B * (N + 1) * 2);  // the feasible sets are an intermediate when the caller does not ask for them
    if (int rc = S.failed()) return rc;
    if (A.B > 0) hipLaunchKernelGGL(kernel, dim3((A.B + 63) / 64), dim3(64), 0, S.stream, A, dmin, dmax, dL, dX);
    return S.finish();
}

// ---- the dense-row passes (tpr_dense.hip.inc), whatever feeds a stage's rows ------------------------------------------------
// One host path for the three families: rows read from arrays (tpr_*_dense_batch), generated from path samples
// (tpr_*_sampled_batch), generated from samples with the stage boxes read (tpr_*_sampled_boxed_batch).  A source -- DenseSource,
// SampledSource, BoxedSource below, each next to its check and its stager -- holds the call's problem and says what differs:
//   check()     what is refused before anything is staged;
//   anchor()    the pointer whose device the call runs on;
//   stage(S)    -> Args: DenseArgs / SampledArgs / BoxedArgs;
//   launch      its unit's tpr_tu_*_launch (0 = solve, 1 = feasible sets, 2 = TOPPRAsd's forward scans; != 0: no layout);
//   reachable   its instantiation of lane_dense_reachable_kernel;
//   grid(A)     what TOPPRAsd's steps are differences of (null: they are A.deltas);
//   name        the prefix of its messages.
// A pass is the source's check, the check of its own pointers, the staging and the launch, in this order (which refusal wins
// when two arguments are bad: tests/test_dense_refusal_order.py); an entry is one call of its pass on its source.
template <class Src>
int launch_rows(const typename Src::Args &A, int pass, const char *what, hipStream_t stream) {
    if (A.B > 0 && Src::launch(&A, pass, stream) != 0)
        return fail(TPR_E_UNSUPPORTED, std::string(Src::name) + " " + what + ": no kernel for this row count");
    return TPR_E_OK;
}

template <class Src>
int rows_solve(const Src &src, const tpr_result *r, void *stream_) {
    if (int rc = src.check()) return rc;
    if (!r || !r->K) return fail(TPR_E_BADARG, std::string(Src::name) + " solve: r->K is required");
    Staging S(src.p->flags & TPR_DEVICE_PTRS, src.anchor(), stream_);
    if (int rc = S.failed()) return rc;
    typename Src::Args A = src.stage(S);
    const size_t B = (size_t)A.B, N = (size_t)A.N;
    A.sd_start = S.in(src.p->sd_start, B); A.sd_end = S.in(src.p->sd_end, B);
    A.sd2 = S.out(r->sd2, B * (N + 1)); A.sd = S.out(r->sd, B * (N + 1)); A.u = S.out(r->u, B * N);
    A.K = S.out(r->K, B * (N + 1) * 2); A.status = S.out(r->status, B);
    if (int rc = S.failed()) return rc;
    if (int rc = launch_rows<Src>(A, 0, "solve", S.stream)) return rc;
    return S.finish();
}

template <class Src>
int rows_solve_desired_duration(const Src &src, const double *desired, double atol, const tpr_result *r, double *alpha, void *stream_) {
    if (int rc = src.check()) return rc;
    if (!r || !r->K || !desired) return fail(TPR_E_BADARG, "result.K and desired are required");
    Staging S(src.p->flags & TPR_DEVICE_PTRS, src.anchor(), stream_);
    if (int rc = S.failed()) return rc;
    typename Src::Args A = src.stage(S);
    const size_t B = (size_t)A.B, N = (size_t)A.N;
    const double *ddes = S.in(desired, B);
    A.sd_start = S.in(src.p->sd_start, B); A.sd_end = S.in(src.p->sd_end, B);
    double *dsd2 = S.out(r->sd2, B * (N + 1)), *dsd = S.out(r->sd, B * (N + 1)), *du = S.out(r->u, B * N);
    A.K = S.out(r->K, B * (N + 1) * 2); A.status = S.out(r->status, B);
    double *dalpha = S.out(alpha, B);
    const SdWork W = sd_workspace(S, B, N, dalpha ? 0 : 1, A.status);
    if (int rc = S.failed()) return rc;
    if (!dalpha) dalpha = W.extra;
    if (A.B > 0) {
        A.sd_xf = W.xf; A.sd_uf = W.uf; A.sd_xl = W.xl; A.sd_ul = W.ul;
        // backward scan -> K and the controllability verdict, the two forward scans, then durations / bisection / blend
        A.backward_only = 1;
        if (Src::launch(&A, 0, S.stream) != 0 || Src::launch(&A, 2, S.stream) != 0)
            return fail(TPR_E_UNSUPPORTED, std::string(Src::name) + " TOPPRAsd: no kernel for this row count");
        tpr::SdBlendArgs G{A.B, A.N, A.flags, atol, Src::grid(A), ddes, nullptr, nullptr, nullptr, nullptr, A.status,
                           dsd2, dsd, du, dalpha, A.status, A.deltas};
        if (int rc = launch_sd_finish(G, W, nullptr, S.stream)) return rc;
    }
    return S.finish();
}

template <class Src>
int rows_controllable_sets(const Src &src, const double *sdmin, const double *sdmax, double *K, void *stream_) {
    if (int rc = src.check()) return rc;
    if (!sdmin || !sdmax || !K) return fail(TPR_E_BADARG, "sdmin/sdmax/K are required");
    Staging S(src.p->flags & TPR_DEVICE_PTRS, src.anchor(), stream_);
    if (int rc = S.failed()) return rc;
    typename Src::Args A = src.stage(S);
    const size_t B = (size_t)A.B, N = (size_t)A.N;
    A.sd_end = S.in(sdmin, B); A.sd_end_hi = S.in(sdmax, B);
    A.K = S.out(K, B * (N + 1) * 2);
    A.backward_only = 1;
    if (int rc = S.failed()) return rc;
    if (int rc = launch_rows<Src>(A, 0, "controllable sets", S.stream)) return rc;
    return S.finish();
}

template <class Src>
int rows_feasible_sets(const Src &src, double *X, void *stream_) {
    if (int rc = src.check()) return rc;
    if (!X) return fail(TPR_E_BADARG, "X is required");
    Staging S(src.p->flags & TPR_DEVICE_PTRS, src.anchor(), stream_);
    if (int rc = S.failed()) return rc;
    typename Src::Args A = src.stage(S);
    A.X = S.out(X, (size_t)A.B * ((size_t)A.N + 1) * 2);
    if (int rc = S.failed()) return rc;
    if (int rc = launch_rows<Src>(A, 1, "feasible sets", S.stream)) return rc;
    return S.finish();
}

template <class Src>
int rows_reachable_sets(const Src &src, const double *sdmin, const double *sdmax, double *L, double *X, void *stream_) {
    if (int rc = src.check()) return rc;
    if (!sdmin || !sdmax || !L) return fail(TPR_E_BADARG, "sdmin/sdmax/L are required");
    Staging S(src.p->flags & TPR_DEVICE_PTRS, src.anchor(), stream_);
    if (int rc = S.failed()) return rc;
    return reachable_sets(S, src.stage(S), Src::reachable, sdmin, sdmax, L, X);
}

// Knot-parallel spline parametrizer (tpr_spline.hip.inc): a block per trajectory, all N + 1 knots in LDS -- their times,
// their d right-hand sides and `xcols` working columns (the kernel's XC: max(d - 1, 2) for the coefficient table,
// max(d, 2) when it samples).  Up to 16 dof and 1024 knots, 256 bytes of static LDS beside the columns.
size_t pcr_lds_bytes(size_t d, size_t N, size_t xcols) { return (1 + d + xcols) * ((N + 1) | 1) * sizeof(double); }
bool pcr_supported(size_t d, size_t N, size_t lds) { return d <= 16 && N + 1 <= 1024 && lds <= kMaxDynamicLds - 256; }
template <bool SAMPLE>
void launch_param_pcr(const tpr::ParamSplineArgs &K, double *coef_t, const tpr::ParamSampleArgs &Q, size_t lds, hipStream_t stream) {
    const int kpt = K.N + 1 <= 256 ? 1 : (K.N + 1 <= 512 ? 2 : 4);  // knots per thread of the 256
    const dim3 grid((unsigned)K.B), block(256);
    (void)tpr::for_dof(K.d, 0, [&](auto D, auto) {
        if (kpt == 1) hipLaunchKernelGGL((tpr::param_spline_pcr_kernel<D(), 1, SAMPLE>), grid, block, lds, stream, K, coef_t, Q);
        else if (kpt == 2) hipLaunchKernelGGL((tpr::param_spline_pcr_kernel<D(), 2, SAMPLE>), grid, block, lds, stream, K, coef_t, Q);
        else hipLaunchKernelGGL((tpr::param_spline_pcr_kernel<D(), 4, SAMPLE>), grid, block, lds, stream, K, coef_t, Q);
        return 0;
    });
}

}  // namespace

extern "C" {

const char *tpr_last_error(void) { return g_err.c_str(); }

const char *tpr_version(void) { return "toppra_hip 0.2 (gfx950)"; }
// ABI guard: the structures of this header grow at the END from version to version (0.2: tpr_problem.active); a binding built
// against an older header would pass a shorter structure, so it compares these sizes with its own before the first call.
int tpr_abi_sizes(int32_t *problem_bytes, int32_t *result_bytes, int32_t *dense_problem_bytes) {
    if (problem_bytes) *problem_bytes = (int32_t)sizeof(tpr_problem);
    if (result_bytes) *result_bytes = (int32_t)sizeof(tpr_result);
    if (dense_problem_bytes) *dense_problem_bytes = (int32_t)sizeof(tpr_dense_problem);
    return 2;  // ABI revision
}

int tpr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int tpr_init(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail(TPR_E_HIP, "no HIP device visible");
    if (device < 0 || device >= n || device >= 64) return fail(TPR_E_BADARG, "device index out of range");
    if (!g_checked[device].load(std::memory_order_acquire)) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(TPR_E_UNSUPPORTED, std::string("this library is built for gfx950 only, found ") + prop.gcnArchName);
        // Workspaces and host-call staging come from the device's stream-ordered pool (Staging::scratch).  Its default
        // release threshold is 0: whatever was freed goes back to the driver at the next synchronisation, and a call that
        // needs a 1.2 GB workspace (tpr_param_spline_batch at the headline shape) maps it afresh every time -- 65 ms per
        // call instead of 2 on some boxes (profiles/r03: the kernel itself takes 1.9 ms).  Keep freed memory in the pool.
        hipMemPool_t pool = nullptr;
        if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess && pool) {
            uint64_t keep = UINT64_MAX;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        }
        (void)hipGetLastError();
        g_checked[device].store(true, std::memory_order_release);
    }
    t_device = device;  // the caller's current device is left alone: every entry scopes its own (DeviceScope)
    g_process_device.store(device, std::memory_order_relaxed);
    return TPR_E_OK;
}


int tpr_solve_batch(const tpr_problem *p, const tpr_result *r, void *stream_) {
    if (int rc = check_problem(p)) return rc;
    if (!r) return fail(TPR_E_BADARG, "null result");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);  // (allocates nothing until it stages)
    if (int rc = S.failed()) return rc;
    if (!S.device_ptrs && p->B > 0) {
        const int rc = solve_small_host_call(p, r, S.stream, S.scope.dev);
        if (rc != kNotSmall) return rc;
    }
    tpr::BatchArgs A = stage_problem(p, S);
    const size_t B = (size_t)p->B, N = (size_t)p->N;
    A.active = S.out(p->active, B * 4, true);  // the wrapper object's warm-start state, in / out
    A.sd2 = S.out(r->sd2, B * (N + 1));
    A.sd = S.out(r->sd, B * (N + 1));
    A.status = S.out(r->status, B);
    // outputs the caller does not want (the controllable sets, which the forward scan still reads; the path
    // accelerations, which retiming -- compute_trajectory -- never looks at) live in a stream-ordered workspace
    // (S.scratch): no host copy, no caller buffer, and the fast kernel family still serves the call
    // (family 4 keeps K in LDS and skips what is not asked for: no workspace, no HBM traffic for it)
    A.u = r->u ? S.out(r->u, B * N) : nullptr;
    A.K = r->K ? S.out(r->K, B * (N + 1) * 2) : nullptr;
    {
        tpr::BatchArgs probe = A;  // the variant the call will take, with every output it could ask a workspace for
        if (!probe.u) probe.u = reinterpret_cast<double *>(8);
        if (!probe.K) probe.K = reinterpret_cast<double *>(8);
        const int v = pick_variant(p->variant, probe);
        if (v != 4 && v != 5) {  // (families 4 and 5 keep K in LDS and skip what is not asked for)
            if (!A.u) A.u = S.scratch<double>(B * N);
            if (!A.K) A.K = S.scratch<double>(B * (N + 1) * 2);
        }
    }
    if (int rc = S.failed()) return rc;
    if (int rc = launch_solve(p, A, S.stream)) return rc;
    return S.finish();
}

int tpr_solve_desired_duration_batch(const tpr_problem *p, const double *desired, double atol,
                                     const tpr_result *r, double *alpha, void *stream_) {
    if (int rc = check_problem(p)) return rc;
    if (!r || !r->K || !desired) return fail(TPR_E_BADARG, "result.K and desired are required");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    tpr::BatchArgs A = stage_problem(p, S);
    if (!group_supported(A)) return fail(TPR_E_UNSUPPORTED, "TOPPRAsd: dof out of range");
    const size_t B = (size_t)p->B, N = (size_t)p->N;
    const double *ddes = S.in(desired, B);
    A.sd2 = S.out(r->sd2, B * (N + 1));
    A.sd = S.out(r->sd, B * (N + 1));
    A.u = S.out(r->u, B * N);
    A.K = S.out(r->K, B * (N + 1) * 2);
    A.status = S.out(r->status, B);
    double *dalpha = S.out(alpha, B);
    // (3 more doubles per trajectory: alpha when the caller wants none, then the two durations family 3's forward scans sum)
    const SdWork W = sd_workspace(S, B, N, 3, A.status);
    if (int rc = S.failed()) return rc;
    if (!dalpha) dalpha = W.extra;
    if (A.B > 0) {
        const double *dur = nullptr;
        tpr::BatchArgs Ab = A;
        Ab.backward_only = 1;
        // p->variant: 0 = auto; 2 / 3 force the rows-across-lanes scans / the certified lane kernel for both scans
        const bool fused = p->variant == 3 || (p->variant == 0 && cert_supported(Ab) && A.B >= cert_auto_from(A.d));
        if (fused) {
            // family 3: backward scan + fastest / slowest forward profiles in ONE launch (cert_solve_kernel<SDFWD>)
            if (!cert_supported(Ab)) return fail(TPR_E_UNSUPPORTED, "variant 3 needs an acceleration constraint, d <= 15, no strict mode");
            if (int rc = launch_cert_sd(A, W.xf, W.uf, W.xl, W.ul, W.extra + B, S.stream)) return rc;
            dur = W.extra + B;
        } else {
            // backward scan -> K and the controllability verdict (the time-optimal forward scan is not needed), then
            // the two forward scans on the rows-across-lanes kernel
            if (int rc = launch_solve(p, Ab, S.stream)) return rc;
            tpr::SdArgs F{A.B, A.nseg, A.N, A.flags, A.coef, A.breaks, A.grid, A.vlim, A.alim, A.sd_start, A.K,
                          A.status, W.xf, W.uf, W.xl, W.ul};
            if (int rc = dispatch_sd_forward(A.d, F, S.stream)) return rc;
        }
        tpr::SdBlendArgs G{A.B, A.N, A.flags, atol, A.grid, ddes, nullptr, nullptr, nullptr, nullptr, A.status,
                           A.sd2, A.sd, A.u, dalpha, A.status};
        if (int rc = launch_sd_finish(G, W, dur, S.stream)) return rc;
    }
    return S.finish();
}

int tpr_robust_solve_batch(const tpr_problem *p, const double *ellipsoid, const tpr_result *r, double *X,
                           void *stream_) {
    if (int rc = check_problem(p)) return rc;
    if (!r || !r->K || !ellipsoid) return fail(TPR_E_BADARG, "result.K and ellipsoid are required");
    if (!(p->flags & TPR_HAS_ACCELERATION)) return fail(TPR_E_BADARG, "the robust path needs an acceleration constraint");
    if (ellipsoid[0] < 0 || ellipsoid[1] < 0 || ellipsoid[2] < 0) return fail(TPR_E_BADARG, "ellipsoid axes must be non-negative");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    tpr::RobustArgs P{};
    P.A = stage_problem(p, S);
    const size_t B = (size_t)p->B, N = (size_t)p->N;
    P.A.sd2 = S.out(r->sd2, B * (N + 1));
    P.A.sd = S.out(r->sd, B * (N + 1));
    P.A.u = S.out(r->u, B * N);
    P.A.K = S.out(r->K, B * (N + 1) * 2);
    P.A.status = S.out(r->status, B);
    P.X = S.out(X, B * (N + 1) * 2);
    P.ru = ellipsoid[0]; P.rx = ellipsoid[1]; P.rc = ellipsoid[2];
    if (int rc = S.failed()) return rc;
    if (P.A.B > 0) {
        // p->variant: 0 = auto, 1 = the generic lane kernel (one trajectory per lane, rows in scratch), 2 = rows across lanes
        if (p->variant != 1 && group_supported(P.A)) {  // up to 16 dof, Interpolation or Collocation, with or without feasible sets
            if (int rc = dispatch_group_robust(P, S.stream)) return rc;
        } else {
            (void)tpr_tu_robust_lane_launch(&P, S.stream);
        }
    }
    return S.finish();
}

int tpr_solve_batch_timed(const tpr_problem *p, const tpr_result *r, void *stream_, int reps,
                          float *ms_per_launch) {
    if (int rc = check_problem(p)) return rc;
    if (!(p->flags & TPR_DEVICE_PTRS)) return fail(TPR_E_BADARG, "timed entry needs TPR_DEVICE_PTRS");
    if (!r || !r->K || reps < 1 || !ms_per_launch) return fail(TPR_E_BADARG, "bad timed arguments");
    Staging S(true, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    tpr::BatchArgs A = stage_problem(p, S);
    A.sd2 = r->sd2; A.sd = r->sd; A.u = r->u; A.K = r->K; A.status = r->status;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, S.stream));
    for (int i = 0; i < reps; ++i)
        if (int rc = launch_solve(p, A, S.stream)) return rc;
    HIP_TRY(hipEventRecord(e1, S.stream));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    HIP_TRY(hipGetLastError());
    *ms_per_launch = ms / (float)reps;
    return TPR_E_OK;
}

int tpr_controllable_sets_batch(const tpr_problem *p, const double *sdmin, const double *sdmax,
                                double *K, void *stream_) {
    if (int rc = check_problem(p)) return rc;
    if (!sdmin || !sdmax || !K) return fail(TPR_E_BADARG, "sdmin/sdmax/K are required");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    tpr::BatchArgs A = stage_problem(p, S);
    const size_t B = (size_t)p->B, N = (size_t)p->N;
    const double *dmin = S.in(sdmin, B), *dmax = S.in(sdmax, B);
    A.K = S.out(K, B * (N + 1) * 2);
    A.active = S.out(p->active, B * 4, true);
    if (int rc = S.failed()) return rc;
    if (A.B > 0) {
        if ((group_supported(A) || wave_supported(A)) && A.N >= 1) {  // the backward scan of the fast kernels
            A.sd_end = dmin;
            A.sd_end_hi = dmax;
            A.backward_only = 1;
            if (int rc = launch_solve(p, A, S.stream)) return rc;
        } else {
            hipLaunchKernelGGL(tpr::lane_controllable_kernel, dim3((A.B + 63) / 64), dim3(64), 0, S.stream, A,
                               dmin, dmax);
        }
    }
    return S.finish();
}

// ---- dense rows (any canonical-linear constraint list): tpr_dense.hip.inc ----------------------------------------
namespace {
int check_dense(const tpr_dense_problem *p) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (!p) return fail(TPR_E_BADARG, "null dense problem");
    if (p->B < 0 || p->N < 1) return fail(TPR_E_BADARG, "dense problem: B >= 0, N >= 1");
    if (p->nC < 2 || p->nC > 122) return fail(TPR_E_UNSUPPORTED, "dense problem: 2 <= nC <= 122 rows per stage (incl. the two x_next rows)");
    if (!p->a || !p->b || !p->c || !p->low || !p->high || !p->deltas) return fail(TPR_E_BADARG, "dense problem: a, b, c, low, high, deltas are required");
    return TPR_E_OK;
}
tpr::DenseArgs stage_dense(const tpr_dense_problem *p, Staging &S) {
    tpr::DenseArgs A{};
    const size_t B = (size_t)p->B, N = (size_t)p->N, nC = (size_t)p->nC;
    A.B = p->B; A.N = p->N; A.nC = p->nC; A.flags = p->flags;
    A.a = S.in(p->a, B * (N + 1) * nC); A.b = S.in(p->b, B * (N + 1) * nC); A.c = S.in(p->c, B * (N + 1) * nC);
    A.low = S.in(p->low, B * (N + 1) * 2); A.high = S.in(p->high, B * (N + 1) * 2);
    A.deltas = S.in(p->deltas, B * N);
    A.active = S.out(p->active, B * 4, true);
    return A;
}
struct DenseSource {
    using Args = tpr::DenseArgs;
    static constexpr const char *name = "dense";
    static constexpr auto launch = tpr_tu_dense_launch;
    static constexpr auto reachable = tpr::lane_dense_reachable_kernel<Args>;
    const tpr_dense_problem *p;
    int check() const { return check_dense(p); }
    const void *anchor() const { return p->a; }
    Args stage(Staging &S) const { return stage_dense(p, S); }
    static const double *grid(const Args &) { return nullptr; }
};
}  // namespace

int tpr_solve_dense_batch(const tpr_dense_problem *p, const tpr_result *r, void *stream_) {
    return rows_solve(DenseSource{p}, r, stream_);
}

int tpr_solve_desired_duration_dense_batch(const tpr_dense_problem *p, const double *desired, double atol, const tpr_result *r,
                                           double *alpha, void *stream_) {
    return rows_solve_desired_duration(DenseSource{p}, desired, atol, r, alpha, stream_);
}

int tpr_reachable_sets_dense_batch(const tpr_dense_problem *p, const double *sdmin, const double *sdmax, double *L, double *X,
                                   void *stream_) {
    return rows_reachable_sets(DenseSource{p}, sdmin, sdmax, L, X, stream_);
}

int tpr_controllable_sets_dense_batch(const tpr_dense_problem *p, const double *sdmin, const double *sdmax, double *K,
                                      void *stream_) {
    return rows_controllable_sets(DenseSource{p}, sdmin, sdmax, K, stream_);
}

int tpr_feasible_sets_dense_batch(const tpr_dense_problem *p, double *X, void *stream_) {
    return rows_feasible_sets(DenseSource{p}, X, stream_);
}

int tpr_reachable_sets_batch(const tpr_problem *p, const double *sdmin, const double *sdmax, double *L, double *X,
                             void *stream_) {
    if (int rc = check_problem(p)) return rc;
    if (!sdmin || !sdmax || !L) return fail(TPR_E_BADARG, "sdmin/sdmax/L are required");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    tpr::BatchArgs A = stage_problem(p, S);
    return reachable_sets(S, A, tpr::lane_reachable_kernel, sdmin, sdmax, L, X);
}

int tpr_feasible_sets_batch(const tpr_problem *p, double *X, void *stream_) {
    if (int rc = check_problem(p)) return rc;
    if (!X) return fail(TPR_E_BADARG, "X is required");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    tpr::BatchArgs A = stage_problem(p, S);
    double *dX = S.out(X, (size_t)p->B * (p->N + 1) * 2);
    A.active = S.out(p->active, (size_t)p->B * 4, true);
    if (int rc = S.failed()) return rc;
    if (A.B > 0) {
        // p->variant: 0 = auto, 2 / 3 / 4 force a kernel family (1: the generic lane kernel)
        const int want = p->variant;
        const bool wave_auto = wave_supported(A) && (A.active || A.B <= 64 || !group_supported(A));
        if (want == 3 && !cert_feasible_supported(A))
            return fail(TPR_E_UNSUPPORTED, "variant 3 needs an acceleration constraint, d <= 15, no strict mode, no warm-start state");
        if (want == 4 && !wave_supported(A)) return fail(TPR_E_UNSUPPORTED, "variant 4: N too large for the per-trajectory LDS tables");
        if (A.active && (want == 2 || want == 3))
            return fail(TPR_E_UNSUPPORTED, "tpr_problem.active (warm-start state in / out) is maintained by kernel families 4 and 1 only: leave variant at 0");
        if (A.active && want == 0 && !wave_supported(A)) {  // N > 1480: the generic lane kernel carries the state
            hipLaunchKernelGGL(tpr::lane_feasible_kernel, dim3((A.B + 63) / 64), dim3(64), 0, S.stream, A, dX);
        } else if (want == 4 || (want == 0 && wave_auto)) {
            // one trajectory per wave: a handful of trajectories (latency), 17..32 dof, or the wrapper object's
            // warm-start state in / out
            A.feasible_X = dX;
            if (int rc = launch_wave(A, S.stream)) return rc;
        } else if (want == 3 || (want == 0 && cert_feasible_supported(A) && A.B >= (A.d <= 8 ? 8192 : cert_auto_from(A.d)))) {
            // one trajectory per lane, certified answers (family 3): a fixed-latency round up to 65536 trajectories
            if (int rc = launch_cert_feasible(A, dX, S.stream)) return rc;
        } else if (group_supported(A) && want != 1) {
            if (int rc = dispatch_group_feasible(A, dX, S.stream)) return rc;
        } else {
            hipLaunchKernelGGL(tpr::lane_feasible_kernel, dim3((A.B + 63) / 64), dim3(64), 0, S.stream, A, dX);
        }
    }
    return S.finish();
}

int tpr_constraint_params_batch(const tpr_problem *p, double *a, double *b, double *c, double *low,
                                double *high, double *xbound, double *qs, double *qss, void *stream_) {
    if (int rc = check_problem(p)) return rc;
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    tpr::BatchArgs A = stage_problem(p, S);
    const size_t pts = (size_t)p->B * (p->N + 1), nC = (size_t)rows_per_lp(p);
    double *da = S.out(a, pts * nC), *db = S.out(b, pts * nC), *dc = S.out(c, pts * nC);
    double *dlow = S.out(low, pts * 2), *dhigh = S.out(high, pts * 2), *dxb = S.out(xbound, pts * 2);
    double *dqs = S.out(qs, pts * p->d), *dqss = S.out(qss, pts * p->d);
    if (int rc = S.failed()) return rc;
    if (pts > 0) {
        const unsigned tiles = (unsigned)((p->N + 1 + tpr::kParamsTile - 1) / tpr::kParamsTile);
        if (tiles > 65535u) return fail(TPR_E_UNSUPPORTED, "tpr_constraint_params_batch: more than 2 M gridpoints");
        const int tile = (int)((p->N + 1 + tiles - 1) / tiles);
        const size_t lds = ((size_t)2 * (tpr::kParamsTile + 1) * p->d + tpr::kParamsTile + 2 * p->d) * sizeof(double);
        hipLaunchKernelGGL(tpr::params_tile_kernel, dim3((unsigned)p->B, tiles), dim3(256), lds, S.stream, A, tile,
                           da, db, dc, dlow, dhigh, dxb, dqs, dqss);
    }
    return S.finish();
}

int tpr_solve_stagewise_batch(const tpr_problem *p, const int32_t *stage, const double *g,
                              const double *xb, int32_t *active, int solve_lp1d, double *out,
                              void *stream_) {
    if (int rc = check_problem(p)) return rc;
    if (!stage || !g || !xb || !active || !out) return fail(TPR_E_BADARG, "null stagewise argument");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    tpr::BatchArgs A = stage_problem(p, S);
    const size_t B = (size_t)p->B;
    const int32_t *dstage = S.in(stage, B);
    const double *dg = S.in(g, B * 2), *dxb = S.in(xb, B * 4);
    int32_t *dact = S.out(active, B * 4, true);
    double *dout = S.out(out, B * 2);
    if (int rc = S.failed()) return rc;
    if (A.B > 0)
        hipLaunchKernelGGL(tpr::lane_stagewise_kernel, dim3((A.B + 63) / 64), dim3(64), 0, S.stream, A, dstage,
                           dg, dxb, dact, solve_lp1d, dout);
    return S.finish();
}

int tpr_const_accel_times_batch(const tpr_problem *p, const double *sd, double *ts, double *us, void *stream_) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (!p || p->B < 0 || p->N < 1 || !p->grid || !sd || !ts) return fail(TPR_E_BADARG, "bad const-accel arguments");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->grid, stream_);
    if (int rc = S.failed()) return rc;
    const size_t B = (size_t)p->B, N = (size_t)p->N;
    tpr::ParamArgs A{};
    A.B = p->B; A.N = p->N; A.flags = p->flags;
    A.grid = S.in(p->grid, path_counts(p).grid);
    A.sd = S.in(sd, B * (N + 1));
    A.ts = S.out(ts, B * (N + 1));
    A.us = S.out(us, B * N);
    if (int rc = S.failed()) return rc;
    if (A.B > 0) {
        const size_t lds = 2 * ((size_t)A.N + 1) * sizeof(double);
        if (lds <= kMaxDynamicLds) hipLaunchKernelGGL(tpr::const_accel_times_kernel, dim3(A.B), dim3(64), lds, S.stream, A);
        else hipLaunchKernelGGL(tpr::const_accel_times_lane_kernel, dim3((A.B + 63) / 64), dim3(64), 0, S.stream, A);
    }
    return S.finish();
}

int tpr_const_accel_eval_batch(const tpr_problem *p, const double *sd, const double *ts, const double *us,
                               int T, const double *times, int order, double *out, void *stream_) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (!p || p->B < 0 || p->N < 1 || p->d < 1 || p->nseg < 1 || !p->coef || !p->breaks || !p->grid || !sd || !ts ||
        !us || !times || !out || T < 0 || order < 0 || order > 2)
        return fail(TPR_E_BADARG, "bad const-accel eval arguments");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    const size_t B = (size_t)p->B, N = (size_t)p->N, d = (size_t)p->d;
    tpr::EvalArgs A{};
    A.B = p->B; A.N = p->N; A.d = p->d; A.nseg = p->nseg; A.T = T; A.flags = p->flags; A.order = order;
    stage_path(p, S, A);
    A.sd = S.in(sd, B * (N + 1));
    A.ts = S.in(ts, B * (N + 1));
    A.us = S.in(us, B * N);
    A.times = S.in(times, B * (size_t)T);
    A.out = S.out(out, B * (size_t)T * d);
    if (int rc = S.failed()) return rc;
    const long long total = (long long)p->B * T * p->d;  // one thread per (sample, dof)
    if (total > (long long)0x7fffffff * 256) return fail(TPR_E_BADARG, "constant-acceleration evaluation: B T d too large for one launch");
    if (total > 0)
        hipLaunchKernelGGL(tpr::const_accel_eval_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S.stream, A);
    return S.finish();
}

namespace {
// Launch the fit of B*d splines of up to m points: short splines keep their working arrays in registers /
// scratch; longer ones use a stream-ordered global workspace of 6 m doubles per spline.
int launch_spline_fit(const tpr::SplineArgs &A, const int32_t *counts, Staging &S) {
    hipStream_t stream = S.stream;
    const long long total = (long long)A.B * A.d;
    if (total <= 0) return TPR_E_OK;
    const dim3 grid((unsigned)((total + 127) / 128)), block(128);
    if (A.m <= 8) {  // the usual handful of waypoints: unrolled, arrays in registers
        hipLaunchKernelGGL((tpr::spline_fit_kernel<8>), grid, block, 0, stream, A, counts, (double *)nullptr);
        return TPR_E_OK;
    }
    if (A.m <= tpr::kSplineMaxPts) {
        hipLaunchKernelGGL((tpr::spline_fit_kernel<tpr::kSplineMaxPts>), grid, block, 0, stream, A, counts, (double *)nullptr);
        return TPR_E_OK;
    }
    double *ws = S.scratch<double>((size_t)6 * A.m * (size_t)total);
    if (S.err != hipSuccess) return fail(TPR_E_HIP, std::string("spline-fit workspace: ") + hipGetErrorString(S.err));
    hipLaunchKernelGGL((tpr::spline_fit_kernel<0>), grid, block, 0, stream, A, counts, ws);
    return TPR_E_OK;
}
}  // namespace

int tpr_spline_fit_batch(int B, int m, int d, const double *knots, int knots_per_path,
                         const double *waypoints, int bc_start, int bc_end, const double *bc_start_val,
                         const double *bc_end_val, double *coef, int device_ptrs, void *stream_) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (B < 0 || d < 1 || m < 2 || !knots || !waypoints || !coef)
        return fail(TPR_E_BADARG, "spline fit needs m >= 2 waypoints, knots, waypoints, coef");
    if (bc_start < 0 || bc_start > 2 || bc_end < 0 || bc_end > 2) return fail(TPR_E_BADARG, "unknown boundary condition");
    Staging S(device_ptrs != 0, waypoints, stream_);
    if (int rc = S.failed()) return rc;
    tpr::SplineArgs A{};
    A.B = B; A.m = m; A.d = d; A.knots_per_path = knots_per_path; A.bc0 = bc_start; A.bc1 = bc_end;
    A.knots = S.in(knots, (size_t)(knots_per_path ? B : 1) * m);
    A.way = S.in(waypoints, (size_t)B * m * d);
    A.bcv0 = S.in(bc_start_val, (size_t)B * d);
    A.bcv1 = S.in(bc_end_val, (size_t)B * d);
    A.coef = S.out(coef, (size_t)B * 4 * (m - 1) * d);
    if (int rc = S.failed()) return rc;
    if (int rc = launch_spline_fit(A, nullptr, S)) return rc;
    return S.finish();
}

int tpr_param_spline_batch(const tpr_problem *p, const double *sd, double *knot_times, int32_t *counts, double *coef_t,
                           void *stream_) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (!p || p->B < 0 || p->N < 1 || p->d < 1 || p->nseg < 1 || !p->coef || !p->breaks || !p->grid || !sd || !knot_times ||
        !counts || !coef_t)
        return fail(TPR_E_BADARG, "bad spline-parametrizer arguments");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    const size_t B = (size_t)p->B, N = (size_t)p->N, d = (size_t)p->d;
    tpr::ParamSplineArgs K{};
    K.B = p->B; K.N = p->N; K.d = p->d; K.nseg = p->nseg; K.flags = p->flags;
    stage_path(p, S, K);
    K.sd = S.in(sd, B * (N + 1));
    K.tk = S.out(knot_times, B * (N + 1));
    K.counts = S.out(counts, B);
    double *dcoef = S.out(coef_t, B * 4 * N * d);
    if (int rc = S.failed()) return rc;
    if (p->variant < 0 || p->variant > 3) return fail(TPR_E_BADARG, "spline parametrizer: variant 0 (auto), 1 (generic), 2 (fused, LAPACK order), 3 (knot-parallel)");
    const size_t pcr_lds = pcr_lds_bytes(d, N, std::max<size_t>(d - 1, 2));
    const bool pcr_fits = pcr_supported(d, N, pcr_lds);
    if (p->variant == 3 && !pcr_fits)
        return fail(TPR_E_UNSUPPORTED, "spline parametrizer variant 3 needs d <= 16 and about 2 (d + 1) (N + 1) doubles of LDS (<= 64 KB)");
    if (B > 0 && pcr_fits && (p->variant == 0 || p->variant == 3)) {
        launch_param_pcr<false>(K, dcoef, tpr::ParamSampleArgs{}, pcr_lds, S.stream);
        return S.finish();
    }
    if (B > 0 && d <= 64 && N <= 65535 && p->variant != 1) {
        // one kernel (tpr_spline.hip.inc): a wave owns floor(64/d) trajectories; workspace = the eliminated right-hand
        // sides [tasks][N+1][64], the eliminated matrix rows [tasks][N+1][3][tpw], the knots' path positions [B][N+1]
        tpr::ParamFusedArgs F{};
        F.K = K; F.coef_t = dcoef; F.tpw = std::min(64 / (int)d, tpr::kPsMaxTpw);
        const size_t tasks = (B + F.tpw - 1) / F.tpw;
        const size_t rhs_n = tasks * (N + 1) * 64, rows_n = tasks * (N + 1) * 3 * F.tpw, sk_n = B * (N + 1);
        F.rhs = S.scratch<double>(rhs_n + rows_n + sk_n);
        if (S.err != hipSuccess) return fail(TPR_E_HIP, std::string("spline-parametrizer workspace: ") + hipGetErrorString(S.err));
        F.rows = F.rhs + rhs_n;
        F.sk = F.rows + rows_n;
        const size_t lds = ((size_t)(tpr::kPsTile + 1) * (128 + 5 * F.tpw) + 64) * sizeof(double) + (size_t)F.tpw * sizeof(int);
        hipLaunchKernelGGL(tpr::param_spline_fused_kernel<tpr::kPsTile>, dim3((unsigned)tasks), dim3(64), lds, S.stream, F);
        return S.finish();
    }
    // generic path (d > 64, or variant 1): waypoints q(s_i) and the two end derivatives, then the spline-fit kernel
    K.way = S.scratch<double>(B * (N + 1) * d + 2 * B * d);
    if (int rc = S.failed()) return rc;
    if (B > 0) {
        K.bcv0 = K.way + B * (N + 1) * d;
        K.bcv1 = K.bcv0 + B * d;
        hipLaunchKernelGGL(tpr::param_spline_knots_kernel<tpr::ParamSplineArgs>, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, S.stream, K);
        tpr::SplineArgs A{};
        A.B = p->B; A.m = p->N + 1; A.d = p->d; A.knots_per_path = 1; A.bc0 = tpr::kBcFirst; A.bc1 = tpr::kBcFirst;
        A.knots = K.tk; A.way = K.way; A.bcv0 = K.bcv0; A.bcv1 = K.bcv1; A.coef = dcoef;
        if (int rc = launch_spline_fit(A, K.counts, S)) return rc;
    }
    return S.finish();
}

int tpr_param_spline_sample_batch(const tpr_problem *p, const double *sd, int T, const double *times, int times_per_traj,
                                  int fractions, double *q, double *qd, double *qdd, double *duration, void *stream_) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (!p || p->B < 0 || p->N < 1 || p->d < 1 || p->nseg < 1 || !p->coef || !p->breaks || !p->grid || !sd || !times || T < 0 ||
        (!q && !qd && !qdd))
        return fail(TPR_E_BADARG, "bad spline-sampling arguments");
    if (!times_per_traj && !fractions) return fail(TPR_E_BADARG, "shared sample times must be fractions of each trajectory's duration");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    const size_t B = (size_t)p->B, N = (size_t)p->N, d = (size_t)p->d;
    tpr::ParamSplineArgs K{};
    K.B = p->B; K.N = p->N; K.d = p->d; K.nseg = p->nseg; K.flags = p->flags;
    stage_path(p, S, K);
    K.sd = S.in(sd, B * (N + 1));
    tpr::ParamSampleArgs Q{};
    Q.T = T; Q.fractions = fractions; Q.times_per_traj = times_per_traj;
    Q.times = S.in(times, (times_per_traj ? B : 1) * (size_t)T);
    Q.q[0] = S.out(q, B * T * d); Q.q[1] = S.out(qd, B * T * d); Q.q[2] = S.out(qdd, B * T * d);
    Q.duration = S.out(duration, B);
    if (int rc = S.failed()) return rc;
    const size_t lds = pcr_lds_bytes(d, N, std::max<size_t>(d, 2));  // (sampling keeps the knot times: one column more)
    if (!pcr_supported(d, N, lds))
        return fail(TPR_E_UNSUPPORTED, "spline sampling: d <= 16 and about (2 d + 1) (N + 1) doubles of LDS (<= 64 KB); use tpr_param_spline_batch + tpr_ppoly_eval_batch");
    if (B > 0 && T > 0) launch_param_pcr<true>(K, nullptr, Q, lds, S.stream);
    return S.finish();
}

int tpr_ppoly_eval_batch(int B, int nseg, int d, const double *coef, const double *breaks, const int32_t *counts, int T,
                         const double *times, int order, double *out, int device_ptrs, void *stream_) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (B < 0 || nseg < 1 || d < 1 || T < 0 || order < 0 || order > 2 || !coef || !breaks || !times || !out)
        return fail(TPR_E_BADARG, "bad piecewise-polynomial evaluation arguments");
    Staging S(device_ptrs != 0, coef, stream_);
    if (int rc = S.failed()) return rc;
    tpr::PpolyArgs A{};
    A.B = B; A.nseg = nseg; A.d = d; A.T = T; A.order = order;
    A.coef = S.in(coef, (size_t)B * 4 * nseg * d);
    A.breaks = S.in(breaks, (size_t)B * (nseg + 1));
    A.counts = S.in(counts, (size_t)B);
    A.times = S.in(times, (size_t)B * T);
    A.out = S.out(out, (size_t)B * T * d);
    if (int rc = S.failed()) return rc;
    const long long total = (long long)B * T * d;  // one thread per (sample, dof)
    if (total > (long long)0x7fffffff * 256) return fail(TPR_E_BADARG, "piecewise-polynomial evaluation: B T d too large for one launch");
    // (round 3 also tried a block per path with the breakpoints searched in LDS on the thread-per-sample form: 1.07 ->
    // 1.20 ms -- the scattered coefficient rows were what it waited for, not the search)
    if (total > 0)
        hipLaunchKernelGGL(tpr::ppoly_eval_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S.stream, A);
    return S.finish();
}

int tpr_lp1d_batch(int n, int nrows, const double *v, const double *a, const double *b,
                   const double *low, const double *high, int32_t *result, double *optval,
                   double *optvar, int32_t *active, void *stream_) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (n < 0 || nrows < 0 || !v || !low || !high || !result || !optval || !optvar || !active)
        return fail(TPR_E_BADARG, "bad lp1d arguments");
    Staging S(false, nullptr, stream_);
    if (int rc = S.failed()) return rc;
    const size_t nn = (size_t)n, rows = nn * (size_t)nrows;
    const double *dv = S.in(v, nn * 2), *da = S.in(a, rows), *db = S.in(b, rows);
    const double *dlow = S.in(low, nn), *dhigh = S.in(high, nn);
    int32_t *dres = S.out(result, nn), *dact = S.out(active, nn);
    double *dval = S.out(optval, nn), *dvar = S.out(optvar, nn);
    if (int rc = S.failed()) return rc;
    if (n > 0)
        hipLaunchKernelGGL(tpr::lp1d_kernel, dim3((n + 63) / 64), dim3(64), 0, S.stream, n, nrows, dv, da, db,
                           dlow, dhigh, dres, dval, dvar, dact);
    return S.finish();
}

int tpr_lp2d_batch(int n, int nrows, const double *v, const double *a, const double *b,
                   const double *c, const double *low, const double *high, const int32_t *active_in,
                   int32_t *result, double *optval, double *optvar, int32_t *active_out,
                   void *stream_) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (n < 0 || nrows < 0 || nrows > tpr::kKatMaxRows || !v || !low || !high || !active_in || !result ||
        !optval || !optvar || !active_out)
        return fail(TPR_E_BADARG, "bad lp2d arguments (nrows <= 128)");
    Staging S(false, nullptr, stream_);
    if (int rc = S.failed()) return rc;
    const size_t nn = (size_t)n, rows = nn * (size_t)nrows;
    const double *dv = S.in(v, nn * 3), *da = S.in(a, rows), *db = S.in(b, rows), *dc = S.in(c, rows);
    const double *dlow = S.in(low, nn * 2), *dhigh = S.in(high, nn * 2);
    const int32_t *dain = S.in(active_in, nn * 2);
    int32_t *dres = S.out(result, nn), *daout = S.out(active_out, nn * 2);
    double *dval = S.out(optval, nn), *dvar = S.out(optvar, nn * 2);
    if (int rc = S.failed()) return rc;
    if (n > 0)
        hipLaunchKernelGGL(tpr::lp2d_kernel, dim3((n + 63) / 64), dim3(64), 0, S.stream, n, nrows, dv, da, db,
                           dc, dlow, dhigh, dain, dres, dval, dvar, daout);
    return S.finish();
}

}  // extern "C"

// ---- dense rows of second-order / torque constraints built on the GPU: tpr_rows.hip.inc (host side only here; the kernels
// are a unit of their own, csrc/tpr_rows_tu.hip) -------------------------------------------------------------------------
#include "tpr_rows_args.hpp"
namespace {
// The second-order blocks of a row entry staged into its argument block (A.nC holds the rows before them on entry, the
// stage's rows on return): shared by tpr_second_order_rows_batch and tpr_sampled_rows_batch.
int stage_row_blocks(tpr::RowsArgs &A, Staging &S, int nblocks, const tpr_second_order_block *blocks, int dof, const char *who) {
    const size_t B = (size_t)A.B, pts = B * ((size_t)A.N + 1);
    A.nblocks = nblocks;
    for (int j = 0; j < nblocks; ++j) {
        const tpr_second_order_block &U = blocks[j];
        tpr::RowsBlock &K = A.blk[j];
        const int fkind = U.flags & (TPR_SO_F_SHARED | TPR_SO_F_PER_TRAJ | TPR_SO_F_PER_POINT);
        const int gkind = U.flags & (TPR_SO_G_PER_TRAJ | TPR_SO_G_PER_POINT);
        if (U.p < 1 || !U.w0 || !U.wa || !U.wb || !U.g) return fail(TPR_E_BADARG, "second-order block: p >= 1 and w0, wa, wb, g are required");
        if ((fkind & (fkind - 1)) || gkind == (TPR_SO_G_PER_TRAJ | TPR_SO_G_PER_POINT)) return fail(TPR_E_BADARG, "second-order block: one F layout and one g layout");
        if (fkind ? (!U.F || U.m < 1) : (U.F != nullptr)) return fail(TPR_E_BADARG, "second-order block: F [m][p] with an F flag, NULL for the signed identity");
        if (U.friction && U.p != dof) return fail(TPR_E_BADARG, "second-order block: dry friction needs p == d");
        K.p = U.p; K.m = fkind ? U.m : 2 * U.p; K.flags = U.flags; K.col0 = A.nC; K.lds0 = A.wsum;
        const size_t m = (size_t)K.m, w = (size_t)U.p;
        if (m > 122) return fail(TPR_E_UNSUPPORTED, "second-order block: more than 122 rows per stage");
        A.nC += ((U.flags & TPR_SO_INTERPOLATION) ? 2 : 1) * K.m;
        A.wsum += 3 * U.p;
        if (A.nC > 122 || A.wsum > 3 * 1024) return fail(TPR_E_UNSUPPORTED, std::string(who) + ": more than 122 rows per stage (incl. the two x_next rows), or blocks wider than 1024 in all");
        K.w0 = S.in(U.w0, pts * w); K.wa = S.in(U.wa, pts * w); K.wb = S.in(U.wb, pts * w);
        K.F = S.in(U.F, (fkind == TPR_SO_F_PER_POINT ? pts : fkind == TPR_SO_F_PER_TRAJ ? B : 1) * m * w);
        K.g = S.in(U.g, (gkind == TPR_SO_G_PER_POINT ? pts : gkind == TPR_SO_G_PER_TRAJ ? B : 1) * m);
        K.friction = S.in(U.friction, B * w);
    }
    return TPR_E_OK;
}
}  // namespace

extern "C" {
__attribute__((visibility("hidden"))) int tpr_tu_rows_launch(const tpr::RowsArgs *, double *, double *, double *, double *, double *,
                                                             double *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_path_eval_launch(const tpr::PathEvalArgs *, hipStream_t);

int tpr_second_order_block_bytes(void) { return (int)sizeof(tpr_second_order_block); }

int tpr_path_eval_batch(const tpr_problem *p, double *q, double *qs, double *qss, void *stream_) {
    if (int rc = check_problem(p)) return rc;
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    tpr::PathEvalArgs A{};
    A.B = p->B; A.d = p->d; A.nseg = p->nseg; A.N = p->N; A.flags = p->flags;
    stage_path(p, S, A);
    const size_t n = (size_t)p->B * (p->N + 1) * p->d;
    A.q = S.out(q, n); A.qs = S.out(qs, n); A.qss = S.out(qss, n);
    if (int rc = S.failed()) return rc;
    if (n > 0 && tpr_tu_path_eval_launch(&A, S.stream) != 0) return fail(TPR_E_BADARG, "tpr_path_eval_batch: B (N + 1) d too large for one launch");
    return S.finish();
}

int tpr_second_order_rows_batch(const tpr_problem *p, int nblocks, const tpr_second_order_block *blocks, double *a, double *b,
                                double *c, double *low, double *high, double *deltas, void *stream_) {
    if (int rc = check_problem(p)) return rc;
    if (nblocks < 0 || nblocks > TPR_SO_MAX_BLOCKS || (nblocks > 0 && !blocks))
        return fail(TPR_E_BADARG, "tpr_second_order_rows_batch: 0 <= nblocks <= TPR_SO_MAX_BLOCKS");
    if (!a || !b || !c || !low || !high) return fail(TPR_E_BADARG, "tpr_second_order_rows_batch: a, b, c, low, high are required");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->coef, stream_);
    if (int rc = S.failed()) return rc;
    const size_t B = (size_t)p->B, d = (size_t)p->d, pts = B * ((size_t)p->N + 1);
    tpr::RowsArgs A{};
    A.B = p->B; A.d = p->d; A.nseg = p->nseg; A.N = p->N; A.flags = p->flags;
    stage_path(p, S, A);
    A.vlim = S.in(p->vlim, B * d * 2);
    A.alim = S.in(p->alim, B * d * 2);
    A.nC = rows_per_lp(p);
    if (int rc = stage_row_blocks(A, S, nblocks, blocks, p->d, "tpr_second_order_rows_batch")) return rc;
    const size_t nC = (size_t)A.nC;
    double *da = S.out(a, pts * nC), *db = S.out(b, pts * nC), *dc = S.out(c, pts * nC);
    double *dlow = S.out(low, pts * 2), *dhigh = S.out(high, pts * 2), *ddel = S.out(deltas, B * (size_t)p->N);
    if (int rc = S.failed()) return rc;
    if (pts > 0) {
        const int rc = tpr_tu_rows_launch(&A, da, db, dc, dlow, dhigh, ddel, S.stream);
        if (rc != 0) return fail(TPR_E_UNSUPPORTED, rc == -1 ? "tpr_second_order_rows_batch: one gridpoint's coefficients do not fit the LDS" : "tpr_second_order_rows_batch: more than 65535 tiles of gridpoints");
    }
    return S.finish();
}
}  // extern "C"

// ---- any geometric path: the path given as samples at the gridpoints (tpr_sampled_problem) -------------------------------
// The dense-row passes with SampledStage in place of DenseStage (csrc/tpr_sampled_tu.hip), the row kernel and the spline
// parametrizer's knot kernel with a sample source.
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_sampled_launch(const tpr::SampledArgs *, int, hipStream_t);
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_sampled_rows_launch(const tpr::SampledRowsArgs *, double *, double *, double *,
                                                                                double *, double *, double *, hipStream_t);
namespace {
int sampled_rows_per_lp(const tpr_sampled_problem *p) {
    return 2 + ((p->flags & TPR_HAS_ACCELERATION) ? ((p->flags & TPR_ACC_INTERPOLATION) ? 4 : 2) * p->d : 0);
}
// solver: the fused passes (rows across lanes: nC <= 122), else the row / parametrizer entries
int check_sampled(const tpr_sampled_problem *p, bool solver) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (!p) return fail(TPR_E_BADARG, "null sampled problem");
    if (p->B < 0 || p->N < 1) return fail(TPR_E_BADARG, "sampled problem: B >= 0, N >= 1");
    if (p->d < 1 || p->d > TPR_MAX_DOF) return fail(TPR_E_UNSUPPORTED, "sampled problem: dof must be in [1, TPR_MAX_DOF]");
    if (!p->grid || !p->qs || !p->qss) return fail(TPR_E_BADARG, "sampled problem: grid, qs, qss are required");
    if ((p->flags & TPR_HAS_VELOCITY) && !p->vlim) return fail(TPR_E_BADARG, "TPR_HAS_VELOCITY without vlim");
    if ((p->flags & TPR_HAS_ACCELERATION) && !p->alim) return fail(TPR_E_BADARG, "TPR_HAS_ACCELERATION without alim");
    if (solver && sampled_rows_per_lp(p) > 122)
        return fail(TPR_E_UNSUPPORTED, "sampled problem: more than 122 rows per stage (2 + 4 d under Interpolation: d <= 30; Collocation: d <= 32)");
    return TPR_E_OK;
}
tpr::SampledArgs stage_sampled(const tpr_sampled_problem *p, Staging &S) {
    tpr::SampledArgs A{};
    const size_t B = (size_t)p->B, N = (size_t)p->N, d = (size_t)p->d;
    A.B = p->B; A.N = p->N; A.d = p->d; A.flags = p->flags; A.nC = sampled_rows_per_lp(p);
    A.grid = S.in(p->grid, ((p->flags & TPR_GRID_PER_TRAJ) ? B : 1) * (N + 1));
    A.qs = S.in(p->qs, B * (N + 1) * d); A.qss = S.in(p->qss, B * (N + 1) * d);
    A.vlim = S.in(p->vlim, B * d * 2); A.alim = S.in(p->alim, B * d * 2);
    A.active = S.out(p->active, B * 4, true);
    return A;
}
struct SampledSource {
    using Args = tpr::SampledArgs;
    static constexpr const char *name = "sampled";
    static constexpr auto launch = tpr_tu_sampled_launch;
    static constexpr auto reachable = tpr::lane_dense_reachable_kernel<Args>;
    const tpr_sampled_problem *p;
    int check() const { return check_sampled(p, true); }
    const void *anchor() const { return p->qs; }
    Args stage(Staging &S) const { return stage_sampled(p, S); }
    static const double *grid(const Args &A) { return A.grid; }
};
}  // namespace

extern "C" {
int tpr_sampled_problem_bytes(void) { return (int)sizeof(tpr_sampled_problem); }

int tpr_solve_sampled_batch(const tpr_sampled_problem *p, const tpr_result *r, void *stream_) {
    return rows_solve(SampledSource{p}, r, stream_);
}

int tpr_solve_desired_duration_sampled_batch(const tpr_sampled_problem *p, const double *desired, double atol, const tpr_result *r,
                                             double *alpha, void *stream_) {
    return rows_solve_desired_duration(SampledSource{p}, desired, atol, r, alpha, stream_);
}

int tpr_controllable_sets_sampled_batch(const tpr_sampled_problem *p, const double *sdmin, const double *sdmax, double *K,
                                        void *stream_) {
    return rows_controllable_sets(SampledSource{p}, sdmin, sdmax, K, stream_);
}

int tpr_feasible_sets_sampled_batch(const tpr_sampled_problem *p, double *X, void *stream_) {
    return rows_feasible_sets(SampledSource{p}, X, stream_);
}

int tpr_reachable_sets_sampled_batch(const tpr_sampled_problem *p, const double *sdmin, const double *sdmax, double *L, double *X,
                                     void *stream_) {
    return rows_reachable_sets(SampledSource{p}, sdmin, sdmax, L, X, stream_);
}

int tpr_sampled_rows_batch(const tpr_sampled_problem *p, int nblocks, const tpr_second_order_block *blocks, double *a, double *b,
                           double *c, double *low, double *high, double *deltas, double *xbound, void *stream_) {
    if (int rc = check_sampled(p, false)) return rc;
    if (nblocks < 0 || nblocks > TPR_SO_MAX_BLOCKS || (nblocks > 0 && !blocks))
        return fail(TPR_E_BADARG, "tpr_sampled_rows_batch: 0 <= nblocks <= TPR_SO_MAX_BLOCKS");
    if (!a || !b || !c || !low || !high) return fail(TPR_E_BADARG, "tpr_sampled_rows_batch: a, b, c, low, high are required");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->qs, stream_);
    if (int rc = S.failed()) return rc;
    const size_t B = (size_t)p->B, d = (size_t)p->d, pts = B * ((size_t)p->N + 1);
    tpr::SampledRowsArgs A{};
    A.B = p->B; A.d = p->d; A.nseg = 0; A.N = p->N; A.flags = p->flags;
    A.grid = S.in(p->grid, ((p->flags & TPR_GRID_PER_TRAJ) ? B : 1) * ((size_t)p->N + 1));
    A.qs = S.in(p->qs, pts * d); A.qss = S.in(p->qss, pts * d);
    A.vlim = S.in(p->vlim, B * d * 2);
    A.alim = S.in(p->alim, B * d * 2);
    A.nC = sampled_rows_per_lp(p);
    if (int rc = stage_row_blocks(A, S, nblocks, blocks, p->d, "tpr_sampled_rows_batch")) return rc;
    const size_t nC = (size_t)A.nC;
    double *da = S.out(a, pts * nC), *db = S.out(b, pts * nC), *dc = S.out(c, pts * nC);
    double *dlow = S.out(low, pts * 2), *dhigh = S.out(high, pts * 2), *ddel = S.out(deltas, B * (size_t)p->N);
    A.xbound = S.out(xbound, pts * 2);
    if (int rc = S.failed()) return rc;
    if (pts > 0) {
        const int rc = tpr_tu_sampled_rows_launch(&A, da, db, dc, dlow, dhigh, ddel, S.stream);
        if (rc != 0) return fail(TPR_E_UNSUPPORTED, rc == -1 ? "tpr_sampled_rows_batch: one gridpoint's coefficients do not fit the LDS" : "tpr_sampled_rows_batch: more than 65535 tiles of gridpoints");
    }
    return S.finish();
}

int tpr_param_spline_samples_batch(const tpr_sampled_problem *p, const double *sd, double *knot_times, int32_t *counts,
                                   double *coef_t, void *stream_) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (!p || p->B < 0 || p->N < 1 || p->d < 1 || !p->grid || !p->q || !p->qs || !sd || !knot_times || !counts || !coef_t)
        return fail(TPR_E_BADARG, "bad sampled spline-parametrizer arguments (grid, q, qs, sd and the outputs are required)");
    Staging S(p->flags & TPR_DEVICE_PTRS, p->q, stream_);
    if (int rc = S.failed()) return rc;
    const size_t B = (size_t)p->B, N = (size_t)p->N, d = (size_t)p->d;
    tpr::ParamSamplesArgs K{};
    K.B = p->B; K.N = p->N; K.d = p->d; K.nseg = 0; K.flags = p->flags;
    K.grid = S.in(p->grid, ((p->flags & TPR_GRID_PER_TRAJ) ? B : 1) * (N + 1));
    K.q = S.in(p->q, B * (N + 1) * d); K.qs = S.in(p->qs, B * (N + 1) * d);
    K.sd = S.in(sd, B * (N + 1));
    K.tk = S.out(knot_times, B * (N + 1));
    K.counts = S.out(counts, B);
    double *dcoef = S.out(coef_t, B * 4 * N * d);
    K.way = S.scratch<double>(B * (N + 1) * d + 2 * B * d);
    if (int rc = S.failed()) return rc;
    if (B > 0) {
        K.bcv0 = K.way + B * (N + 1) * d;
        K.bcv1 = K.bcv0 + B * d;
        hipLaunchKernelGGL(tpr::param_spline_knots_kernel<tpr::ParamSamplesArgs>, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, S.stream, K);
        tpr::SplineArgs A{};
        A.B = p->B; A.m = p->N + 1; A.d = p->d; A.knots_per_path = 1; A.bc0 = tpr::kBcFirst; A.bc1 = tpr::kBcFirst;
        A.knots = K.tk; A.way = K.way; A.bcv0 = K.bcv0; A.bcv1 = K.bcv1; A.coef = dcoef;
        if (int rc = launch_spline_fit(A, K.counts, S)) return rc;
    }
    return S.finish();
}
}  // extern "C"

// ---- first-order constraints of any kind: stage boxes built on the GPU, the sampled passes reading them -------------------
// The box kernel and the dense-row passes with BoxedSampledStage live in csrc/tpr_boxed_tu.hip.
#include "tpr_boxed_args.hpp"
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_boxed_launch(const tpr::BoxedArgs *, int, hipStream_t);
extern "C" __attribute__((visibility("hidden"))) int tpr_tu_stage_boxes_launch(tpr::BoxesArgs *, hipStream_t);
namespace {
// the checks of the sampled passes, and: the box carries every first-order constraint
int check_boxed(const tpr_sampled_problem *p, const double *low, const double *high) {
    if (int rc = check_sampled(p, true)) return rc;
    if (p->vlim || (p->flags & TPR_HAS_VELOCITY))
        return fail(TPR_E_UNSUPPORTED, "boxed sampled problem: vlim must be NULL and TPR_HAS_VELOCITY clear (the boxes carry every first-order constraint: make the limits a source of tpr_stage_boxes_batch)");
    if (!low || !high) return fail(TPR_E_BADARG, "boxed sampled problem: low, high are required");
    return TPR_E_OK;
}
tpr::BoxedArgs stage_boxed(const tpr_sampled_problem *p, const double *low, const double *high, Staging &S) {
    tpr::BoxedArgs A{};
    static_cast<tpr::SampledArgs &>(A) = stage_sampled(p, S);
    const size_t pts = (size_t)p->B * ((size_t)p->N + 1);
    A.low = S.in(low, pts * 2); A.high = S.in(high, pts * 2);
    return A;
}
struct BoxedSource {
    using Args = tpr::BoxedArgs;
    static constexpr const char *name = "boxed sampled";
    static constexpr auto launch = tpr_tu_boxed_launch;
    static constexpr auto reachable = tpr::lane_dense_reachable_kernel<Args>;
    const tpr_sampled_problem *p;
    const double *low, *high;
    int check() const { return check_boxed(p, low, high); }
    const void *anchor() const { return p->qs; }
    Args stage(Staging &S) const { return stage_boxed(p, low, high, S); }
    static const double *grid(const Args &A) { return A.grid; }
};
}  // namespace

extern "C" {
int tpr_bound_source_bytes(void) { return (int)sizeof(tpr_bound_source); }

int tpr_stage_boxes_batch(int B, int N, int d, const double *qs, int nsrc, const tpr_bound_source *src, int flags, double *low,
                          double *high, void *stream_) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (B < 0 || N < 1) return fail(TPR_E_BADARG, "tpr_stage_boxes_batch: B >= 0, N >= 1");
    if (nsrc < 0 || nsrc > TPR_BOUND_MAX_SOURCES || (nsrc > 0 && !src))
        return fail(TPR_E_BADARG, "tpr_stage_boxes_batch: 0 <= nsrc <= TPR_BOUND_MAX_SOURCES");
    if (!low || !high) return fail(TPR_E_BADARG, "tpr_stage_boxes_batch: low, high are required");
    bool vel = false;
    for (int j = 0; j < nsrc; ++j) {
        if (src[j].kind < TPR_BOUND_VLIM || src[j].kind > TPR_BOUND_U) return fail(TPR_E_BADARG, "tpr_stage_boxes_batch: unknown bound source kind");
        if (!src[j].data) return fail(TPR_E_BADARG, "tpr_stage_boxes_batch: a bound source without data");
        vel |= src[j].kind == TPR_BOUND_VLIM || src[j].kind == TPR_BOUND_VLIM_GRID;
    }
    if (vel && (!qs || d < 1)) return fail(TPR_E_BADARG, "tpr_stage_boxes_batch: a VLIM* source needs qs and d >= 1");
    if (vel && d > TPR_MAX_DOF) return fail(TPR_E_UNSUPPORTED, "tpr_stage_boxes_batch: dof must be in [1, TPR_MAX_DOF]");
    const size_t pts = (size_t)B * ((size_t)N + 1);
    if (pts > (size_t)0x7fffffff) return fail(TPR_E_UNSUPPORTED, "tpr_stage_boxes_batch: more than 2^31 - 1 gridpoints in the batch");
    Staging S(flags & TPR_DEVICE_PTRS, low, stream_);
    if (int rc = S.failed()) return rc;
    tpr::BoxesArgs A{};
    A.B = B; A.N = N; A.d = vel ? d : 1; A.nsrc = nsrc;
    A.qs = vel ? S.in(qs, pts * (size_t)d) : nullptr;
    for (int j = 0; j < nsrc; ++j) {
        const bool shared = src[j].flags & TPR_BOUND_SHARED;
        const size_t lead = shared ? 1 : (size_t)B;
        size_t count = 0;
        switch (src[j].kind) {
            case TPR_BOUND_VLIM: count = lead * (size_t)d * 2; break;
            case TPR_BOUND_VLIM_GRID: count = lead * ((size_t)N + 1) * (size_t)d * 2; break;
            default: count = lead * ((size_t)N + 1) * 2; break;
        }
        A.src[j] = tpr::BoxSource{src[j].kind, src[j].flags, S.in(src[j].data, count)};
    }
    A.low = S.out(low, pts * 2); A.high = S.out(high, pts * 2);
    if (int rc = S.failed()) return rc;
    if (pts > 0) {
        const int rc = tpr_tu_stage_boxes_launch(&A, S.stream);
        if (rc != 0) return fail(TPR_E_UNSUPPORTED, rc == -1 ? "tpr_stage_boxes_batch: one gridpoint's joints do not fit the LDS" : "tpr_stage_boxes_batch: more than 2^31 - 1 gridpoints in the batch");
    }
    return S.finish();
}

int tpr_solve_sampled_boxed_batch(const tpr_sampled_problem *p, const double *low, const double *high, const tpr_result *r,
                                  void *stream_) {
    return rows_solve(BoxedSource{p, low, high}, r, stream_);
}

int tpr_solve_desired_duration_sampled_boxed_batch(const tpr_sampled_problem *p, const double *low, const double *high,
                                                   const double *desired, double atol, const tpr_result *r, double *alpha,
                                                   void *stream_) {
    return rows_solve_desired_duration(BoxedSource{p, low, high}, desired, atol, r, alpha, stream_);
}

int tpr_controllable_sets_sampled_boxed_batch(const tpr_sampled_problem *p, const double *low, const double *high,
                                              const double *sdmin, const double *sdmax, double *K, void *stream_) {
    return rows_controllable_sets(BoxedSource{p, low, high}, sdmin, sdmax, K, stream_);
}

int tpr_feasible_sets_sampled_boxed_batch(const tpr_sampled_problem *p, const double *low, const double *high, double *X,
                                          void *stream_) {
    return rows_feasible_sets(BoxedSource{p, low, high}, X, stream_);
}

int tpr_reachable_sets_sampled_boxed_batch(const tpr_sampled_problem *p, const double *low, const double *high,
                                           const double *sdmin, const double *sdmax, double *L, double *X, void *stream_) {
    return rows_reachable_sets(BoxedSource{p, low, high}, sdmin, sdmax, L, X, stream_);
}
}  // extern "C"

// ---- a rigid-body chain or tree evaluated on the GPU (tpr_chain.hip.inc, tpr_chain_tu.hip; tpr_tree.hip.inc, tpr_tree_tu.hip;
// tpr_mount.hip.inc, tpr_mount_tu.hip; tpr_joint.hip.inc, tpr_joint_tu.hip; tpr_momentum.hip.inc, tpr_momentum_tu.hip;
// tpr_effmass.hip.inc, tpr_effmass_tu.hip) ---------------------------------------------------------------------------------------
// One host path for the family: an entry is its argument checks, in an order that is its own and is behaviour (which refusal
// wins when two arguments are bad: tests/test_rigid_refusal_order.py), then run_rigid() with what it stages and what it launches.
#include "tpr_mount_args.hpp"
#include "tpr_joint_args.hpp"
#include "tpr_momentum_args.hpp"
#include "tpr_effmass_args.hpp"
#include "../../include/toppra_hip_contact.h"
extern "C" {
__attribute__((visibility("hidden"))) int tpr_tu_chain_dynamics_launch(const tpr::ChainDynArgs *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_chain_terms_launch(const tpr::ChainTermsArgs *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_chain_tool_launch(const tpr::ChainToolArgs *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_chain_accel_launch(const tpr::ChainAccelArgs *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_chain_accel_terms_launch(const tpr::ChainAccelTermsArgs *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_chain_wrench_launch(const tpr::ChainWrenchArgs *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_chain_wrench_terms_launch(const tpr::ChainWrenchTermsArgs *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_chain_points_speed_launch(const tpr::ChainPointsSpeedArgs *, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_chain_points_accel_launch(const tpr::ChainPointsAccelArgs *, int terms, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_tree_dynamics_launch(const tpr::TreeDynArgs *, int forks, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_tree_terms_launch(const tpr::TreeTermsArgs *, int forks, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_mount_wrench_launch(const tpr::MountWrenchArgs *, int forks, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_mount_wrench_terms_launch(const tpr::MountWrenchTermsArgs *, int forks, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_joint_wrench_launch(const tpr::JointWrenchArgs *, int forks, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_joint_wrench_terms_launch(const tpr::JointWrenchTermsArgs *, int forks, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_momentum_launch(const tpr::MomentumArgs *, int forks, hipStream_t);
__attribute__((visibility("hidden"))) int tpr_tu_effmass_launch(const tpr::EffMassArgs *, int forks, hipStream_t);
}
namespace {
// The gridpoints of a batch given as (B, N).
int batch_points(int B, int N, const char *who, long long &npoints) {
    if (B < 0 || N < 0) return fail(TPR_E_BADARG, std::string(who) + ": B >= 0, N >= 0");
    npoints = (long long)B * ((long long)N + 1);
    return TPR_E_OK;
}
int required(bool all_given, const char *who, const char *names) {
    return all_given ? TPR_E_OK : fail(TPR_E_BADARG, std::string(who) + ": " + names + " are required");
}
// joint_type and parent are read here, on the host: a device pointer in their place is refused, not dereferenced
int refuse_device_pointer(const void *ptr, const char *who, const char *what) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return TPR_E_OK;
    }
    if (attr.type != hipMemoryTypeDevice) return TPR_E_OK;
    return fail(TPR_E_BADARG, std::string(who) + ": " + what + " must be a host array, also with TPR_DEVICE_PTRS");
}
// What every chain entry refuses before any launch: the model's shape, its joint types (a host array), the point count.
// (a tree's links are a tpr_chain whose tool is not read: need_tool = false)
int check_chain(const tpr_chain *c, long long npoints, const char *who, bool need_tool = true) {
    if (default_device() < 0) return fail(TPR_E_HIP, "tpr_init() has not succeeded");
    if (!c) return fail(TPR_E_BADARG, std::string(who) + ": null chain");
    if (c->d < 1 || c->d > TPR_MAX_DOF) return fail(TPR_E_BADARG, std::string(who) + ": the chain's dof must be in [1, TPR_MAX_DOF]");
    if (!c->joint_type || !c->axis || !c->rot || !c->trans || !c->mass || !c->com || !c->inertia || !c->gravity || (need_tool && !c->tool))
        return fail(TPR_E_BADARG, std::string(who) + ": every array of the chain is required");
    if (int rc = refuse_device_pointer(c->joint_type, who, "joint_type")) return rc;
    for (int i = 0; i < c->d; ++i)
        if (c->joint_type[i] != TPR_JOINT_REVOLUTE && c->joint_type[i] != TPR_JOINT_PRISMATIC)
            return fail(TPR_E_BADARG, std::string(who) + ": unknown joint type");
    if (npoints < 0) return fail(TPR_E_BADARG, std::string(who) + ": a negative point count");
    if (npoints > 0x7fffffffLL) return fail(TPR_E_UNSUPPORTED, std::string(who) + ": more than 2^31 - 1 points");
    return TPR_E_OK;
}
// (a tree's kernels do not read the tool: it stays null)
tpr::ChainModel stage_links(const tpr_chain *c, Staging &S, bool with_tool) {
    tpr::ChainModel M{};
    const size_t d = (size_t)c->d;
    M.d = c->d;
    for (int i = 0; i < c->d; ++i) M.prismatic |= (uint32_t)(c->joint_type[i] == TPR_JOINT_PRISMATIC) << i;
    M.axis = S.in(c->axis, 3 * d); M.rot = S.in(c->rot, 9 * d); M.trans = S.in(c->trans, 3 * d);
    M.mass = S.in(c->mass, d); M.com = S.in(c->com, 3 * d); M.inertia = S.in(c->inertia, 6 * d);
    M.gravity = S.in(c->gravity, 3);
    if (with_tool) M.tool = S.in(c->tool, 3);
    return M;
}
// A payload is a host struct of 22 doubles: read here, handed to the kernels by value.
static_assert(sizeof(tpr_payload) == 22 * sizeof(double) && sizeof(tpr::ChainPayload) == sizeof(tpr_payload), "tpr_payload is 22 packed doubles");
int check_payload(const tpr_payload *p, const char *who) {
    if (!p) return fail(TPR_E_BADARG, std::string(who) + ": null payload");
    const double *v = &p->mass;
    for (int k = 0; k < 22; ++k)
        if (!std::isfinite(v[k])) return fail(TPR_E_BADARG, std::string(who) + ": every entry of the payload must be finite");
    if (!(p->mass >= 0.0)) return fail(TPR_E_BADARG, std::string(who) + ": the payload's mass must be >= 0");
    return TPR_E_OK;
}
tpr::ChainPayload stage_payload(const tpr_payload *p) {
    tpr::ChainPayload P;
    std::memcpy(&P, p, sizeof(P));
    return P;
}
// A control-point set is a host struct: read here, handed to the kernels by value.  Checked before anything else of a call (it
// needs no device), against the chain's dof: the kernels index their outputs by it.
static_assert(sizeof(tpr::ChainPoints) == sizeof(tpr_chain_points) && TPR_CHAIN_MAX_POINTS == tpr::kChainMaxPoints, "tpr_chain_points is ChainPoints");
int check_points(const tpr_chain *c, const tpr_chain_points *p, const char *who) {
    if (!c) return fail(TPR_E_BADARG, std::string(who) + ": null chain");
    if (!p) return fail(TPR_E_BADARG, std::string(who) + ": null control points");
    if (p->count < 1 || p->count > TPR_CHAIN_MAX_POINTS) return fail(TPR_E_BADARG, std::string(who) + ": the point count must be in [1, TPR_CHAIN_MAX_POINTS]");
    for (int k = 0; k < p->count; ++k) {
        if (p->link[k] < 0 || p->link[k] >= c->d) return fail(TPR_E_BADARG, std::string(who) + ": a control point's link is outside the chain");
        for (int j = 0; j < 3; ++j)
            if (!std::isfinite(p->offset[k][j])) return fail(TPR_E_BADARG, std::string(who) + ": every control point's offset must be finite");
    }
    return TPR_E_OK;
}
tpr::ChainPoints stage_points(const tpr_chain_points *p) {
    tpr::ChainPoints P{};
    P.count = p->count;
    for (int k = 0; k < p->count; ++k) {  // (entries past count stay zero)
        P.link[k] = p->link[k];
        for (int j = 0; j < 3; ++j) P.offset[k][j] = p->offset[k][j];
    }
    return P;
}
// What the tree entries refuse before any launch: what the chain entries refuse (the tool apart), and the parent table -- a host
// array like joint_type, read here, once per call: T takes the kernels' tables, forks their fork count.
int check_tree(const tpr_chain *links, const int32_t *parent, long long npoints, const char *who, tpr::TreeTables &T, int &forks) {
    if (int rc = check_chain(links, npoints, who, false)) return rc;
    if (!parent) return fail(TPR_E_BADARG, std::string(who) + ": null parent array");
    if (int rc = refuse_device_pointer(parent, who, "parent")) return rc;
    forks = tpr::tree_tables(parent, links->d, T);
    if (forks < 0) {
        const int i = -1 - forks;
        return fail(TPR_E_BADARG, std::string(who) + ": the parent of link " + std::to_string(i) + " is " + std::to_string(parent[i]) +
                                      ", outside -1 .. " + std::to_string(i - 1) + " (links are numbered after their parents)");
    }
    if (forks > TPR_TREE_MAX_FORKS)
        return fail(TPR_E_UNSUPPORTED, std::string(who) + ": the tree has " + std::to_string(forks) + " forks, more than TPR_TREE_MAX_FORKS = " +
                                           std::to_string(TPR_TREE_MAX_FORKS));
    return TPR_E_OK;
}
// A mount is a host struct of 16 doubles: read here, handed to the kernels by value; null = the base frame, no platform.  Its
// frame is held to what a chain's rotations and a payload's frame are: orthonormal with determinant +1, to 1e-12.
static_assert(sizeof(tpr_mount) == 16 * sizeof(double) && sizeof(tpr::MountFrame) == sizeof(tpr_mount), "tpr_mount is 16 packed doubles");
int check_mount(const tpr_mount *m, const char *who) {
    if (!m) return TPR_E_OK;
    const double *v = m->rot, *R = m->rot;
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(v[k])) return fail(TPR_E_BADARG, std::string(who) + ": every entry of the mount must be finite");
    bool frame = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            frame = frame && std::fabs(R[r] * R[c] + R[3 + r] * R[3 + c] + R[6 + r] * R[6 + c] - (r == c ? 1.0 : 0.0)) <= 1e-12;
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (!frame || !(std::fabs(det - 1.0) <= 1e-12))
        return fail(TPR_E_BADARG, std::string(who) + ": the mount's rot must be orthonormal with determinant +1 (to 1e-12)");
    if (!(m->mass >= 0.0)) return fail(TPR_E_BADARG, std::string(who) + ": the mount's mass must be >= 0");
    return TPR_E_OK;
}
tpr::MountFrame stage_mount(const tpr_mount *m) {
    tpr::MountFrame P{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}, 0.0, {0.0, 0.0, 0.0}};
    if (m) std::memcpy(&P, m, sizeof(P));
    return P;
}
// A link set is a mask, bit i = link i: at least one link, none outside the robot.
int check_link_mask(const tpr_chain *links, uint32_t mask, const char *who) {
    if (mask == 0) return fail(TPR_E_BADARG, std::string(who) + ": the link set is empty (link_mask = 0)");
    if (links->d < 32 && (mask >> links->d) != 0) return fail(TPR_E_BADARG, std::string(who) + ": the link set names a link outside the robot");
    return TPR_E_OK;
}
// A section set is a host struct: read here, handed to the kernels by value with the mask of its links and the lowest of them.
// Its frames are held to what a mount's is: orthonormal with determinant +1, to 1e-12.
static_assert(sizeof(tpr_joint_sections) == 40 + 8 * 12 * sizeof(double) && TPR_JOINT_MAX_SECTIONS == tpr::kJointMaxSections,
              "tpr_joint_sections is a count, 8 links, a word of padding and 96 doubles");
int check_sections(const tpr_chain *links, const tpr_joint_sections *s, const char *who) {
    if (!s) return fail(TPR_E_BADARG, std::string(who) + ": null sections");
    if (s->count < 1 || s->count > TPR_JOINT_MAX_SECTIONS)
        return fail(TPR_E_BADARG, std::string(who) + ": the section count must be in [1, TPR_JOINT_MAX_SECTIONS]");
    for (int k = 0; k < s->count; ++k)
        if (s->link[k] < 0 || s->link[k] >= links->d) return fail(TPR_E_BADARG, std::string(who) + ": a section's link is outside the robot");
    for (int k = 0; k < s->count; ++k) {
        const double *R = s->rot[k];
        for (int j = 0; j < 9; ++j)
            if (!std::isfinite(R[j])) return fail(TPR_E_BADARG, std::string(who) + ": every entry of the sections must be finite");
        for (int j = 0; j < 3; ++j)
            if (!std::isfinite(s->origin[k][j])) return fail(TPR_E_BADARG, std::string(who) + ": every entry of the sections must be finite");
    }
    for (int k = 0; k < s->count; ++k) {
        const double *R = s->rot[k];
        bool frame = true;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                frame = frame && std::fabs(R[r] * R[c] + R[3 + r] * R[3 + c] + R[6 + r] * R[6 + c] - (r == c ? 1.0 : 0.0)) <= 1e-12;
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!frame || !(std::fabs(det - 1.0) <= 1e-12))
            return fail(TPR_E_BADARG, std::string(who) + ": a section's rot must be orthonormal with determinant +1 (to 1e-12)");
    }
    return TPR_E_OK;
}
tpr::JointSections stage_sections(const tpr_joint_sections *s) {
    tpr::JointSections P{};
    P.count = s->count;
    P.lowest = s->link[0];
    for (int k = 0; k < s->count; ++k) {  // (entries past count stay zero)
        P.link[k] = s->link[k];
        P.mask |= 1u << s->link[k];
        if (s->link[k] < P.lowest) P.lowest = s->link[k];
        for (int j = 0; j < 9; ++j) P.rot[k][j] = s->rot[k][j];
        for (int j = 0; j < 3; ++j) P.origin[k][j] = s->origin[k][j];
    }
    return P;
}

// The argument block of a launch on the links `c`: the model staged, the point count set, the rest zero.
template <class Args>
Args rigid_args(const tpr_chain *c, long long npoints, Staging &S, bool with_tool = true) {
    Args A{};
    A.M = stage_links(c, S, with_tool);
    A.npoints = (int)npoints;
    return A;
}
// Arrays of `count` doubles each into fields of any argument block.
struct StagedIn { const double **field; const double *from; };
struct StagedOut { double **field; double *to; };
void stage_inputs(Staging &S, size_t count, std::initializer_list<StagedIn> arrays) {
    for (const StagedIn &a : arrays) *a.field = S.in(a.from, count);
}
void stage_outputs(Staging &S, size_t count, std::initializer_list<StagedOut> arrays) {
    for (const StagedOut &a : arrays) *a.field = S.out(a.to, count);
}
// A checked call from here to its return: `fill(S)` stages the arrays and returns the argument block, `launch(&block, stream)`
// is the unit's launcher (not called for an empty batch); `device_ptr` tells the device under TPR_DEVICE_PTRS.
template <class Fill, class Launch>
int run_rigid(int flags, const void *device_ptr, void *stream_, long long npoints, const char *no_kernel, Fill fill, Launch launch) {
    Staging S(flags & TPR_DEVICE_PTRS, device_ptr, stream_);
    if (int rc = S.failed()) return rc;
    const auto A = fill(S);
    if (int rc = S.failed()) return rc;
    if (npoints > 0 && launch(&A, S.stream) != 0) return fail(TPR_E_UNSUPPORTED, no_kernel);
    return S.finish();
}
}  // namespace

extern "C" {
int tpr_chain_bytes(void) { return (int)sizeof(tpr_chain); }
int tpr_payload_bytes(void) { return (int)sizeof(tpr_payload); }
int tpr_chain_points_bytes(void) { return (int)sizeof(tpr_chain_points); }
int tpr_mount_bytes(void) { return (int)sizeof(tpr_mount); }
int tpr_joint_sections_bytes(void) { return (int)sizeof(tpr_joint_sections); }

int tpr_chain_inverse_dynamics_batch(const tpr_chain *chain, long long npoints, const double *q, const double *qd, const double *qdd,
                                     double *tau, int flags, void *stream_) {
    const char *who = "tpr_chain_inverse_dynamics_batch";
    if (int rc = check_chain(chain, npoints, who)) return rc;
    if (int rc = required(q && qd && qdd && tau, who, "q, qd, qdd, tau")) return rc;
    return run_rigid(flags, tau, stream_, npoints, "tpr_chain_inverse_dynamics_batch: the kernel's LDS could not be reserved", [&](Staging &S) {
        auto A = rigid_args<tpr::ChainDynArgs>(chain, npoints, S);
        const size_t n = (size_t)npoints * (size_t)chain->d;
        stage_inputs(S, n, {{&A.q, q}, {&A.qd, qd}, {&A.qdd, qdd}});
        stage_outputs(S, n, {{&A.tau, tau}});
        return A;
    }, tpr_tu_chain_dynamics_launch);
}

int tpr_chain_torque_terms_batch(const tpr_chain *chain, int B, int N, const double *q, const double *qs, const double *qss,
                                 double *w0, double *wa, double *wb, int flags, void *stream_) {
    const char *who = "tpr_chain_torque_terms_batch";
    long long npoints = 0;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = check_chain(chain, npoints, who)) return rc;
    if (int rc = required(q && qs && qss && w0 && wa && wb, who, "q, qs, qss, w0, wa, wb")) return rc;
    return run_rigid(flags, w0, stream_, npoints, "tpr_chain_torque_terms_batch: the kernel's LDS could not be reserved", [&](Staging &S) {
        auto A = rigid_args<tpr::ChainTermsArgs>(chain, npoints, S);
        const size_t n = (size_t)npoints * (size_t)chain->d;
        stage_inputs(S, n, {{&A.q, q}, {&A.qs, qs}, {&A.qss, qss}});
        stage_outputs(S, n, {{&A.w0, w0}, {&A.wa, wa}, {&A.wb, wb}});
        return A;
    }, tpr_tu_chain_terms_launch);
}

int tpr_chain_tool_velocity_batch(const tpr_chain *chain, int B, int N, const double *q, const double *qs, const double *Sm,
                                  const double *limit, double *vSv, double *xbound, int flags, void *stream_) {
    const char *who = "tpr_chain_tool_velocity_batch";
    long long npoints = 0;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = check_chain(chain, npoints, who)) return rc;
    if (int rc = required(q && qs, who, "q, qs")) return rc;
    if (!vSv && !xbound) return fail(TPR_E_BADARG, "tpr_chain_tool_velocity_batch: one of vSv, xbound is required");
    if (xbound && !limit) return fail(TPR_E_BADARG, "tpr_chain_tool_velocity_batch: xbound needs limit");
    return run_rigid(flags, vSv ? vSv : xbound, stream_, npoints, "tpr_chain_tool_velocity_batch: no kernel for this dof", [&](Staging &S) {
        auto A = rigid_args<tpr::ChainToolArgs>(chain, npoints, S);
        A.n1 = N + 1;
        stage_inputs(S, (size_t)npoints * (size_t)chain->d, {{&A.q, q}, {&A.qs, qs}});
        A.S = S.in(Sm, 36);
        A.limit = xbound ? S.in(limit, (size_t)B) : nullptr;
        A.vSv = S.out(vSv, (size_t)npoints); A.xbound = S.out(xbound, 2 * (size_t)npoints);
        return A;
    }, tpr_tu_chain_tool_launch);
}

int tpr_chain_tool_acceleration_batch(const tpr_chain *chain, long long npoints, const double *q, const double *qd, const double *qdd,
                                      double *acc, int flags, void *stream_) {
    const char *who = "tpr_chain_tool_acceleration_batch";
    if (int rc = check_chain(chain, npoints, who)) return rc;
    if (int rc = required(q && qd && qdd && acc, who, "q, qd, qdd, acc")) return rc;
    return run_rigid(flags, acc, stream_, npoints, "tpr_chain_tool_acceleration_batch: no kernel for this dof", [&](Staging &S) {
        auto A = rigid_args<tpr::ChainAccelArgs>(chain, npoints, S);
        stage_inputs(S, (size_t)npoints * (size_t)chain->d, {{&A.q, q}, {&A.qd, qd}, {&A.qdd, qdd}});
        stage_outputs(S, 6 * (size_t)npoints, {{&A.acc, acc}});
        return A;
    }, tpr_tu_chain_accel_launch);
}

int tpr_chain_tool_acceleration_terms_batch(const tpr_chain *chain, int B, int N, const double *q, const double *qs, const double *qss,
                                            double *wa, double *wb, int flags, void *stream_) {
    const char *who = "tpr_chain_tool_acceleration_terms_batch";
    long long npoints = 0;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = check_chain(chain, npoints, who)) return rc;
    if (int rc = required(q && qs && qss && wa && wb, who, "q, qs, qss, wa, wb")) return rc;
    return run_rigid(flags, wa, stream_, npoints, "tpr_chain_tool_acceleration_terms_batch: no kernel for this dof", [&](Staging &S) {
        auto A = rigid_args<tpr::ChainAccelTermsArgs>(chain, npoints, S);
        stage_inputs(S, (size_t)npoints * (size_t)chain->d, {{&A.q, q}, {&A.qs, qs}, {&A.qss, qss}});
        stage_outputs(S, 6 * (size_t)npoints, {{&A.wa, wa}, {&A.wb, wb}});
        return A;
    }, tpr_tu_chain_accel_terms_launch);
}

int tpr_chain_tool_wrench_batch(const tpr_chain *chain, const tpr_payload *payload, long long npoints, const double *q, const double *qd,
                                const double *qdd, double *wrench, int flags, void *stream_) {
    const char *who = "tpr_chain_tool_wrench_batch";
    if (int rc = check_chain(chain, npoints, who)) return rc;
    if (int rc = check_payload(payload, who)) return rc;
    if (int rc = required(q && qd && qdd && wrench, who, "q, qd, qdd, wrench")) return rc;
    return run_rigid(flags, wrench, stream_, npoints, "tpr_chain_tool_wrench_batch: no kernel for this dof", [&](Staging &S) {
        auto A = rigid_args<tpr::ChainWrenchArgs>(chain, npoints, S);
        A.P = stage_payload(payload);
        stage_inputs(S, (size_t)npoints * (size_t)chain->d, {{&A.q, q}, {&A.qd, qd}, {&A.qdd, qdd}});
        stage_outputs(S, 6 * (size_t)npoints, {{&A.wrench, wrench}});
        return A;
    }, tpr_tu_chain_wrench_launch);
}

int tpr_chain_tool_wrench_terms_batch(const tpr_chain *chain, const tpr_payload *payload, int B, int N, const double *q, const double *qs,
                                      const double *qss, double *w0, double *wa, double *wb, int flags, void *stream_) {
    const char *who = "tpr_chain_tool_wrench_terms_batch";
    long long npoints = 0;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = check_chain(chain, npoints, who)) return rc;
    if (int rc = check_payload(payload, who)) return rc;
    if (int rc = required(q && qs && qss && w0 && wa && wb, who, "q, qs, qss, w0, wa, wb")) return rc;
    return run_rigid(flags, w0, stream_, npoints, "tpr_chain_tool_wrench_terms_batch: no kernel for this dof", [&](Staging &S) {
        auto A = rigid_args<tpr::ChainWrenchTermsArgs>(chain, npoints, S);
        A.P = stage_payload(payload);
        stage_inputs(S, (size_t)npoints * (size_t)chain->d, {{&A.q, q}, {&A.qs, qs}, {&A.qss, qss}});
        stage_outputs(S, 6 * (size_t)npoints, {{&A.w0, w0}, {&A.wa, wa}, {&A.wb, wb}});
        return A;
    }, tpr_tu_chain_wrench_terms_launch);
}

int tpr_chain_points_speed_batch(const tpr_chain *chain, const tpr_chain_points *points, int B, int N, const double *q, const double *qs,
                                 const double *limit, double *speed2, double *xbound, int flags, void *stream_) {
    const char *who = "tpr_chain_points_speed_batch";
    long long npoints = 0;
    if (int rc = check_points(chain, points, who)) return rc;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = required(q && qs, who, "q, qs")) return rc;
    if (!speed2 && !xbound) return fail(TPR_E_BADARG, "tpr_chain_points_speed_batch: one of speed2, xbound is required");
    if (xbound && !limit) return fail(TPR_E_BADARG, "tpr_chain_points_speed_batch: xbound needs limit");
    if (int rc = check_chain(chain, npoints, who)) return rc;
    return run_rigid(flags, speed2 ? speed2 : xbound, stream_, npoints, "tpr_chain_points_speed_batch: no kernel for this dof and point set", [&](Staging &S) {
        auto A = rigid_args<tpr::ChainPointsSpeedArgs>(chain, npoints, S);
        const size_t count = (size_t)points->count;
        A.P = stage_points(points);
        A.n1 = N + 1;
        stage_inputs(S, (size_t)npoints * (size_t)chain->d, {{&A.q, q}, {&A.qs, qs}});
        A.limit = xbound ? S.in(limit, (size_t)B * count) : nullptr;
        A.speed2 = S.out(speed2, (size_t)npoints * count); A.xbound = S.out(xbound, 2 * (size_t)npoints);
        return A;
    }, tpr_tu_chain_points_speed_launch);
}

int tpr_chain_points_acceleration_batch(const tpr_chain *chain, const tpr_chain_points *points, long long npoints, const double *q,
                                        const double *qd, const double *qdd, double *acc, int flags, void *stream_) {
    const char *who = "tpr_chain_points_acceleration_batch";
    if (int rc = check_points(chain, points, who)) return rc;
    if (int rc = required(q && qd && qdd && acc, who, "q, qd, qdd, acc")) return rc;
    if (int rc = check_chain(chain, npoints, who)) return rc;
    return run_rigid(flags, acc, stream_, npoints, "tpr_chain_points_acceleration_batch: no kernel for this dof and point set", [&](Staging &S) {
        auto A = rigid_args<tpr::ChainPointsAccelArgs>(chain, npoints, S);
        A.P = stage_points(points);
        stage_inputs(S, (size_t)npoints * (size_t)chain->d, {{&A.q, q}, {&A.v1, qd}, {&A.v2, qdd}});
        stage_outputs(S, 3 * (size_t)points->count * (size_t)npoints, {{&A.acc, acc}});
        return A;
    }, [](const tpr::ChainPointsAccelArgs *A, hipStream_t stream) { return tpr_tu_chain_points_accel_launch(A, 0, stream); });
}

int tpr_chain_points_acceleration_terms_batch(const tpr_chain *chain, const tpr_chain_points *points, int B, int N, const double *q,
                                              const double *qs, const double *qss, double *wa, double *wb, int flags, void *stream_) {
    const char *who = "tpr_chain_points_acceleration_terms_batch";
    long long npoints = 0;
    if (int rc = check_points(chain, points, who)) return rc;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = required(q && qs && qss && wa && wb, who, "q, qs, qss, wa, wb")) return rc;
    if (int rc = check_chain(chain, npoints, who)) return rc;
    return run_rigid(flags, wa, stream_, npoints, "tpr_chain_points_acceleration_terms_batch: no kernel for this dof and point set", [&](Staging &S) {
        auto A = rigid_args<tpr::ChainPointsAccelArgs>(chain, npoints, S);
        A.P = stage_points(points);
        stage_inputs(S, (size_t)npoints * (size_t)chain->d, {{&A.q, q}, {&A.v1, qs}, {&A.v2, qss}});
        stage_outputs(S, 3 * (size_t)points->count * (size_t)npoints, {{&A.wa, wa}, {&A.acc, wb}});
        return A;
    }, [](const tpr::ChainPointsAccelArgs *A, hipStream_t stream) { return tpr_tu_chain_points_accel_launch(A, 1, stream); });
}

int tpr_tree_inverse_dynamics_batch(const tpr_chain *links, const int32_t *parent, long long npoints, const double *q, const double *qd,
                                    const double *qdd, double *tau, int flags, void *stream_) {
    const char *who = "tpr_tree_inverse_dynamics_batch";
    tpr::TreeTables T;
    int forks = 0;
    if (int rc = check_tree(links, parent, npoints, who, T, forks)) return rc;
    if (int rc = required(q && qd && qdd && tau, who, "q, qd, qdd, tau")) return rc;
    return run_rigid(flags, tau, stream_, npoints, "tpr_tree_inverse_dynamics_batch: the kernel's LDS could not be reserved", [&](Staging &S) {
        auto A = rigid_args<tpr::TreeDynArgs>(links, npoints, S, false);
        const size_t n = (size_t)npoints * (size_t)links->d;
        A.T = T;
        stage_inputs(S, n, {{&A.q, q}, {&A.qd, qd}, {&A.qdd, qdd}});
        stage_outputs(S, n, {{&A.tau, tau}});
        return A;
    }, [forks](const tpr::TreeDynArgs *A, hipStream_t stream) { return tpr_tu_tree_dynamics_launch(A, forks, stream); });
}

int tpr_tree_torque_terms_batch(const tpr_chain *links, const int32_t *parent, int B, int N, const double *q, const double *qs,
                                const double *qss, double *w0, double *wa, double *wb, int flags, void *stream_) {
    const char *who = "tpr_tree_torque_terms_batch";
    tpr::TreeTables T;
    int forks = 0;
    long long npoints = 0;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = check_tree(links, parent, npoints, who, T, forks)) return rc;
    if (int rc = required(q && qs && qss && w0 && wa && wb, who, "q, qs, qss, w0, wa, wb")) return rc;
    return run_rigid(flags, w0, stream_, npoints, "tpr_tree_torque_terms_batch: the kernel's LDS could not be reserved", [&](Staging &S) {
        auto A = rigid_args<tpr::TreeTermsArgs>(links, npoints, S, false);
        const size_t n = (size_t)npoints * (size_t)links->d;
        A.T = T;
        stage_inputs(S, n, {{&A.q, q}, {&A.qs, qs}, {&A.qss, qss}});
        stage_outputs(S, n, {{&A.w0, w0}, {&A.wa, wa}, {&A.wb, wb}});
        return A;
    }, [forks](const tpr::TreeTermsArgs *A, hipStream_t stream) { return tpr_tu_tree_terms_launch(A, forks, stream); });
}

int tpr_tree_base_wrench_batch(const tpr_chain *links, const int32_t *parent, const tpr_mount *mount, long long npoints, const double *q,
                               const double *qd, const double *qdd, double *wrench, int flags, void *stream_) {
    const char *who = "tpr_tree_base_wrench_batch";
    tpr::TreeTables T;
    int forks = 0;
    if (int rc = check_tree(links, parent, npoints, who, T, forks)) return rc;
    if (int rc = check_mount(mount, who)) return rc;
    if (int rc = required(q && qd && qdd && wrench, who, "q, qd, qdd, wrench")) return rc;
    return run_rigid(flags, wrench, stream_, npoints, "tpr_tree_base_wrench_batch: the kernel's LDS could not be reserved", [&](Staging &S) {
        auto A = rigid_args<tpr::MountWrenchArgs>(links, npoints, S, false);
        A.T = T;
        A.P = stage_mount(mount);
        stage_inputs(S, (size_t)npoints * (size_t)links->d, {{&A.q, q}, {&A.qd, qd}, {&A.qdd, qdd}});
        stage_outputs(S, 6 * (size_t)npoints, {{&A.wrench, wrench}});
        return A;
    }, [forks](const tpr::MountWrenchArgs *A, hipStream_t stream) { return tpr_tu_mount_wrench_launch(A, forks, stream); });
}

int tpr_tree_base_wrench_terms_batch(const tpr_chain *links, const int32_t *parent, const tpr_mount *mount, int B, int N, const double *q,
                                     const double *qs, const double *qss, double *w0, double *wa, double *wb, int flags, void *stream_) {
    const char *who = "tpr_tree_base_wrench_terms_batch";
    tpr::TreeTables T;
    int forks = 0;
    long long npoints = 0;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = check_tree(links, parent, npoints, who, T, forks)) return rc;
    if (int rc = check_mount(mount, who)) return rc;
    if (int rc = required(q && qs && qss && w0 && wa && wb, who, "q, qs, qss, w0, wa, wb")) return rc;
    return run_rigid(flags, w0, stream_, npoints, "tpr_tree_base_wrench_terms_batch: the kernel's LDS could not be reserved", [&](Staging &S) {
        auto A = rigid_args<tpr::MountWrenchTermsArgs>(links, npoints, S, false);
        A.T = T;
        A.P = stage_mount(mount);
        stage_inputs(S, (size_t)npoints * (size_t)links->d, {{&A.q, q}, {&A.qs, qs}, {&A.qss, qss}});
        stage_outputs(S, 6 * (size_t)npoints, {{&A.w0, w0}, {&A.wa, wa}, {&A.wb, wb}});
        return A;
    }, [forks](const tpr::MountWrenchTermsArgs *A, hipStream_t stream) { return tpr_tu_mount_wrench_terms_launch(A, forks, stream); });
}

int tpr_tree_joint_wrench_batch(const tpr_chain *links, const int32_t *parent, const tpr_joint_sections *sections, long long npoints,
                                const double *q, const double *qd, const double *qdd, double *wrench, int flags, void *stream_) {
    const char *who = "tpr_tree_joint_wrench_batch";
    tpr::TreeTables T;
    int forks = 0;
    if (int rc = check_tree(links, parent, npoints, who, T, forks)) return rc;
    if (int rc = check_sections(links, sections, who)) return rc;
    if (int rc = required(q && qd && qdd && wrench, who, "q, qd, qdd, wrench")) return rc;
    return run_rigid(flags, wrench, stream_, npoints, "tpr_tree_joint_wrench_batch: the kernel's LDS could not be reserved", [&](Staging &S) {
        auto A = rigid_args<tpr::JointWrenchArgs>(links, npoints, S, false);
        A.T = T;
        A.S = stage_sections(sections);
        stage_inputs(S, (size_t)npoints * (size_t)links->d, {{&A.q, q}, {&A.qd, qd}, {&A.qdd, qdd}});
        stage_outputs(S, 6 * (size_t)sections->count * (size_t)npoints, {{&A.wrench, wrench}});
        return A;
    }, [forks](const tpr::JointWrenchArgs *A, hipStream_t stream) { return tpr_tu_joint_wrench_launch(A, forks, stream); });
}

int tpr_tree_joint_wrench_terms_batch(const tpr_chain *links, const int32_t *parent, const tpr_joint_sections *sections, int B, int N,
                                      const double *q, const double *qs, const double *qss, double *w0, double *wa, double *wb, int flags,
                                      void *stream_) {
    const char *who = "tpr_tree_joint_wrench_terms_batch";
    tpr::TreeTables T;
    int forks = 0;
    long long npoints = 0;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = check_tree(links, parent, npoints, who, T, forks)) return rc;
    if (int rc = check_sections(links, sections, who)) return rc;
    if (int rc = required(q && qs && qss && w0 && wa && wb, who, "q, qs, qss, w0, wa, wb")) return rc;
    return run_rigid(flags, w0, stream_, npoints, "tpr_tree_joint_wrench_terms_batch: the kernel's LDS could not be reserved", [&](Staging &S) {
        auto A = rigid_args<tpr::JointWrenchTermsArgs>(links, npoints, S, false);
        A.T = T;
        A.S = stage_sections(sections);
        stage_inputs(S, (size_t)npoints * (size_t)links->d, {{&A.q, q}, {&A.qs, qs}, {&A.qss, qss}});
        stage_outputs(S, 6 * (size_t)sections->count * (size_t)npoints, {{&A.w0, w0}, {&A.wa, wa}, {&A.wb, wb}});
        return A;
    }, [forks](const tpr::JointWrenchTermsArgs *A, hipStream_t stream) { return tpr_tu_joint_wrench_terms_launch(A, forks, stream); });
}

int tpr_tree_momentum_batch(const tpr_chain *links, const int32_t *parent, const tpr_mount *mount, uint32_t link_mask, int B, int N,
                            const double *q, const double *qs, const double *limit, double *momentum, double *energy2, double *xbound,
                            int flags, void *stream_) {
    const char *who = "tpr_tree_momentum_batch";
    tpr::TreeTables T;
    int forks = 0;
    long long npoints = 0;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = check_tree(links, parent, npoints, who, T, forks)) return rc;
    if (int rc = check_mount(mount, who)) return rc;
    if (int rc = check_link_mask(links, link_mask, who)) return rc;
    if (int rc = required(q && qs, who, "q, qs")) return rc;
    if (!momentum && !energy2 && !xbound) return fail(TPR_E_BADARG, "tpr_tree_momentum_batch: one of momentum, energy2, xbound is required");
    if (xbound && !limit) return fail(TPR_E_BADARG, "tpr_tree_momentum_batch: xbound needs limit");
    // the walk ends after the highest link of the set; of the forks, it reaches those below that link (their banks are the first)
    int nlinks = 0;
    for (int i = 0; i < links->d; ++i)
        if (link_mask >> i & 1u) nlinks = i + 1;
    int reached = 0;
    for (int i = 0; i < nlinks; ++i) reached += (int)(T.forks >> i & 1u);
    return run_rigid(flags, momentum ? momentum : energy2 ? energy2 : xbound, stream_, npoints,
                     "tpr_tree_momentum_batch: the kernel's LDS could not be reserved", [&](Staging &S) {
        auto A = rigid_args<tpr::MomentumArgs>(links, npoints, S, false);
        A.T = T;
        A.P = stage_mount(mount);
        A.mask = link_mask;
        A.n1 = N + 1;
        A.nlinks = nlinks;
        stage_inputs(S, (size_t)npoints * (size_t)links->d, {{&A.q, q}, {&A.qs, qs}});
        A.limit = xbound ? S.in(limit, 3 * (size_t)B) : nullptr;
        A.momentum = S.out(momentum, 6 * (size_t)npoints); A.energy2 = S.out(energy2, (size_t)npoints);
        A.xbound = S.out(xbound, 2 * (size_t)npoints);
        return A;
    }, [reached](const tpr::MomentumArgs *A, hipStream_t stream) { return tpr_tu_momentum_launch(A, reached, stream); });
}

// (declared in include/toppra_hip_contact.h)
int tpr_tree_effective_mass_batch(const tpr_chain *links, const int32_t *parent, const tpr_chain_points *points, const double *direction,
                                  int B, int N, const double *q, const double *qs, const double *limit, double *speed2, double *mobility,
                                  double *xbound, int flags, void *stream_) {
    const char *who = "tpr_tree_effective_mass_batch";
    tpr::TreeTables T;
    int forks = 0;
    long long npoints = 0;
    if (int rc = batch_points(B, N, who, npoints)) return rc;
    if (int rc = check_tree(links, parent, npoints, who, T, forks)) return rc;
    if (int rc = check_points(links, points, who)) return rc;
    if (direction) {
        if (int rc = refuse_device_pointer(direction, who, "direction")) return rc;
        for (int k = 0; k < 3 * points->count; ++k)
            if (!std::isfinite(direction[k])) return fail(TPR_E_BADARG, std::string(who) + ": every direction must be finite");
    }
    if (!q) return fail(TPR_E_BADARG, std::string(who) + ": q is required");
    if (!qs && (!direction || speed2 || xbound))
        return fail(TPR_E_BADARG, std::string(who) + ": qs is required (but for the mobility alone along given directions)");
    if (!speed2 && !mobility && !xbound) return fail(TPR_E_BADARG, std::string(who) + ": one of speed2, mobility, xbound is required");
    if (xbound && !limit) return fail(TPR_E_BADARG, std::string(who) + ": xbound needs limit");
    return run_rigid(flags, speed2 ? speed2 : mobility ? mobility : xbound, stream_, npoints,
                     "tpr_tree_effective_mass_batch: the kernel's LDS could not be reserved", [&](Staging &S) {
        auto A = rigid_args<tpr::EffMassArgs>(links, npoints, S, false);
        const size_t count = (size_t)points->count;
        A.T = T;
        A.P = stage_points(points);
        A.directed = direction ? 1 : 0;
        for (int p = 0; p < points->count; ++p) {
            for (int j = 0; j < 3; ++j) A.direction[p][j] = direction ? direction[3 * p + j] : 0.0;
            // the point's own link, the links from it to its root, and that root's whole tree
            A.own[points->link[p]] |= (uint16_t)(1u << p);
            int i = points->link[p];
            for (; parent[i] >= 0; i = parent[i]) A.active[i] |= (uint16_t)(1u << p);
            A.active[i] |= (uint16_t)(1u << p);
        }
        for (int i = 0; i < links->d; ++i)  // (parents come first: a link is walked when it is a root with a point, or its parent is)
            if (parent[i] < 0 ? A.active[i] != 0 : (A.walk >> parent[i] & 1u)) A.walk |= 1u << i;
        A.n1 = N + 1;
        A.q = S.in(q, (size_t)npoints * (size_t)links->d);
        A.qs = qs ? S.in(qs, (size_t)npoints * (size_t)links->d) : A.q;  // (no qs: s2 is not asked for, and g does not read it)
        A.limit = xbound ? S.in(limit, 2 * count * (size_t)B) : nullptr;
        A.speed2 = S.out(speed2, count * (size_t)npoints); A.mobility = S.out(mobility, count * (size_t)npoints);
        A.xbound = S.out(xbound, 2 * (size_t)npoints);
        return A;
    }, [forks](const tpr::EffMassArgs *A, hipStream_t stream) { return tpr_tu_effmass_launch(A, forks, stream); });
}
}  // extern "C"

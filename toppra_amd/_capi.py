"""ctypes binding of libtoppra_hip.so (include/toppra_hip.h).

This is the only place the Python host layer touches native code.  There is no CPU fallback:
if the library is missing or no gfx950 device is visible every compute entry raises.
"""
import ctypes as C
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOPPRA_HIP_LIB") or os.path.join(HERE, "libtoppra_hip.so")

MAX_DOF = 32       # generic kernel
MAX_DOF_FAST = 16  # rows-across-lanes kernels
HAS_VELOCITY = 1
HAS_ACCELERATION = 2
ACC_INTERPOLATION = 4
DEVICE_PTRS = 8
BREAKS_PER_TRAJ = 16
GRID_PER_TRAJ = 32
STRICT_SEIDEL = 128
BOUNDARY_SQUARED = 256
SOUND_CERTIFICATES = 512

STATUS_OK, STATUS_FAIL_UNCONTROLLABLE, STATUS_ERR_UNKNOWN = 0, 1, 2

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class ToppraHipError(RuntimeError):
    """The native library is missing, no MI355X is visible, or an API call failed."""


class tpr_problem(C.Structure):
    _fields_ = [("B", C.c_int32), ("d", C.c_int32), ("nseg", C.c_int32), ("N", C.c_int32),
                ("flags", C.c_int32), ("variant", C.c_int32),
                ("coef", C.c_void_p), ("breaks", C.c_void_p), ("grid", C.c_void_p),
                ("vlim", C.c_void_p), ("alim", C.c_void_p),
                ("sd_start", C.c_void_p), ("sd_end", C.c_void_p), ("active", C.c_void_p)]


class tpr_result(C.Structure):
    _fields_ = [("sd2", C.c_void_p), ("sd", C.c_void_p), ("u", C.c_void_p), ("K", C.c_void_p),
                ("status", C.c_void_p)]


class tpr_dense_problem(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("nC", C.c_int32), ("flags", C.c_int32),
                ("a", C.c_void_p), ("b", C.c_void_p), ("c", C.c_void_p),
                ("low", C.c_void_p), ("high", C.c_void_p), ("deltas", C.c_void_p),
                ("sd_start", C.c_void_p), ("sd_end", C.c_void_p), ("active", C.c_void_p)]


class tpr_second_order_block(C.Structure):
    _fields_ = [("p", C.c_int32), ("m", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("w0", C.c_void_p), ("wa", C.c_void_p), ("wb", C.c_void_p),
                ("F", C.c_void_p), ("g", C.c_void_p), ("friction", C.c_void_p)]


class tpr_sampled_problem(C.Structure):
    _fields_ = [("B", C.c_int32), ("d", C.c_int32), ("N", C.c_int32), ("flags", C.c_int32),
                ("grid", C.c_void_p), ("q", C.c_void_p), ("qs", C.c_void_p), ("qss", C.c_void_p),
                ("vlim", C.c_void_p), ("alim", C.c_void_p),
                ("sd_start", C.c_void_p), ("sd_end", C.c_void_p), ("active", C.c_void_p)]


class tpr_bound_source(C.Structure):
    _fields_ = [("kind", C.c_int32), ("flags", C.c_int32), ("data", C.c_void_p)]


class tpr_chain(C.Structure):
    _fields_ = [("d", C.c_int32), ("flags", C.c_int32), ("joint_type", C.c_void_p),
                ("axis", C.c_void_p), ("rot", C.c_void_p), ("trans", C.c_void_p),
                ("mass", C.c_void_p), ("com", C.c_void_p), ("inertia", C.c_void_p),
                ("gravity", C.c_void_p), ("tool", C.c_void_p)]


class tpr_payload(C.Structure):
    _fields_ = [("mass", C.c_double), ("com", C.c_double * 3), ("inertia", C.c_double * 6), ("rot", C.c_double * 9),
                ("origin", C.c_double * 3)]


class tpr_mount(C.Structure):
    _fields_ = [("rot", C.c_double * 9), ("origin", C.c_double * 3), ("mass", C.c_double), ("com", C.c_double * 3)]


JOINT_MAX_SECTIONS = 8  # TPR_JOINT_MAX_SECTIONS: sections in one set


class tpr_joint_sections(C.Structure):
    _fields_ = [("count", C.c_int32), ("link", C.c_int32 * JOINT_MAX_SECTIONS), ("rot", (C.c_double * 9) * JOINT_MAX_SECTIONS),
                ("origin", (C.c_double * 3) * JOINT_MAX_SECTIONS)]


CHAIN_MAX_POINTS = 16  # TPR_CHAIN_MAX_POINTS: control points in one set


class tpr_chain_points(C.Structure):
    _fields_ = [("count", C.c_int32), ("link", C.c_int32 * CHAIN_MAX_POINTS), ("offset", C.c_double * 3 * CHAIN_MAX_POINTS)]


TREE_MAX_FORKS = 4  # TPR_TREE_MAX_FORKS: forks (links with a child that is not the next link) of a kinematic tree
JOINT_REVOLUTE, JOINT_PRISMATIC = 0, 1
# the numeric arrays of tpr_chain, in the order of one packed upload, with their doubles per link (0: per chain, three)
CHAIN_ARRAYS = (("axis", 3), ("rot", 9), ("trans", 3), ("mass", 1), ("com", 3), ("inertia", 6), ("gravity", 0), ("tool", 0))

# tpr_bound_source.kind / .flags
BOUND_VLIM, BOUND_VLIM_GRID, BOUND_X, BOUND_U = 1, 2, 3, 4
BOUND_SHARED = 1
BOUND_MAX_SOURCES = 8
BOUND_KINDS = {"vlim": BOUND_VLIM, "vlim_grid": BOUND_VLIM_GRID, "xbound": BOUND_X, "ubound": BOUND_U}

# tpr_second_order_block.flags
SO_INTERPOLATION, SO_F_SHARED, SO_F_PER_TRAJ, SO_F_PER_POINT, SO_G_PER_TRAJ, SO_G_PER_POINT = 1, 2, 4, 8, 16, 32
SO_MAX_BLOCKS = 8
MAX_DENSE_ROWS = 122  # rows per stage of the dense-row kernels, the two x_next rows included


EXPORTS = (
    "tpr_init", "tpr_device_count", "tpr_last_error", "tpr_version", "tpr_abi_sizes", "tpr_solve_batch",
    "tpr_controllable_sets_batch", "tpr_feasible_sets_batch", "tpr_constraint_params_batch",
    "tpr_solve_stagewise_batch", "tpr_lp1d_batch", "tpr_lp2d_batch", "tpr_solve_batch_timed",
    "tpr_spline_fit_batch", "tpr_const_accel_times_batch", "tpr_const_accel_eval_batch",
    "tpr_solve_desired_duration_batch", "tpr_robust_solve_batch", "tpr_param_spline_batch", "tpr_ppoly_eval_batch",
    "tpr_reachable_sets_batch", "tpr_solve_dense_batch", "tpr_controllable_sets_dense_batch", "tpr_feasible_sets_dense_batch",
    "tpr_solve_desired_duration_dense_batch", "tpr_reachable_sets_dense_batch", "tpr_param_spline_sample_batch",
    "tpr_path_eval_batch", "tpr_second_order_rows_batch", "tpr_second_order_block_bytes",
    "tpr_sampled_problem_bytes", "tpr_sampled_rows_batch", "tpr_solve_sampled_batch", "tpr_controllable_sets_sampled_batch",
    "tpr_feasible_sets_sampled_batch", "tpr_reachable_sets_sampled_batch", "tpr_solve_desired_duration_sampled_batch",
    "tpr_param_spline_samples_batch",
    "tpr_bound_source_bytes", "tpr_stage_boxes_batch", "tpr_solve_sampled_boxed_batch",
    "tpr_solve_desired_duration_sampled_boxed_batch", "tpr_controllable_sets_sampled_boxed_batch",
    "tpr_feasible_sets_sampled_boxed_batch", "tpr_reachable_sets_sampled_boxed_batch",
    "tpr_chain_bytes", "tpr_chain_inverse_dynamics_batch", "tpr_chain_torque_terms_batch", "tpr_chain_tool_velocity_batch",
    "tpr_chain_tool_acceleration_batch", "tpr_chain_tool_acceleration_terms_batch",
    "tpr_payload_bytes", "tpr_chain_tool_wrench_batch", "tpr_chain_tool_wrench_terms_batch",
    "tpr_chain_points_bytes", "tpr_chain_points_speed_batch", "tpr_chain_points_acceleration_batch",
    "tpr_chain_points_acceleration_terms_batch",
    "tpr_tree_inverse_dynamics_batch", "tpr_tree_torque_terms_batch",
    "tpr_mount_bytes", "tpr_tree_base_wrench_batch", "tpr_tree_base_wrench_terms_batch",
    "tpr_joint_sections_bytes", "tpr_tree_joint_wrench_batch", "tpr_tree_joint_wrench_terms_batch",
    "tpr_tree_momentum_batch",
)

_lib = None
_lock = threading.Lock()
_inited_device = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 (soname
    libamdhip64.so.7, but requested by torch under the unversioned name), so if this library pulled
    in /opt/rocm's copy first, a later ``import torch`` would load a second runtime that sees no
    GPU.  Importing torch first makes the dynamic loader bind our NEEDED libamdhip64.so.7 to the
    copy torch already loaded.  Set TOPPRA_HIP_NO_TORCH=1 to skip (torch-free deployments)."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("TOPPRA_HIP_NO_TORCH"):
        return
    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


def load():
    """dlopen the library and declare signatures (no GPU needed for this step)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ToppraHipError(
                "libtoppra_hip.so is not built: run `python -m toppra_amd.build` "
                "(there is no CPU fallback for the TOPP-RA path)")
        _share_hip_runtime_with_torch()
        L = C.CDLL(LIB_PATH)
        L.tpr_init.restype = C.c_int
        L.tpr_init.argtypes = [C.c_int]
        L.tpr_device_count.restype = C.c_int
        L.tpr_last_error.restype = C.c_char_p
        L.tpr_version.restype = C.c_char_p
        I, LL, V = C.c_int, C.c_longlong, C.c_void_p
        P, R, DP, SP = (C.POINTER(s) for s in (tpr_problem, tpr_result, tpr_dense_problem, tpr_sampled_problem))
        SO, BS = C.POINTER(tpr_second_order_block), C.POINTER(tpr_bound_source)
        CP, PP, XP, MP = C.POINTER(tpr_chain), C.POINTER(tpr_payload), C.POINTER(tpr_chain_points), C.POINTER(tpr_mount)
        JP = C.POINTER(tpr_joint_sections)
        # the structs the library reports the size of, one <struct>_bytes() each (tpr_abi_sizes reports the first three at once)
        sized = (tpr_second_order_block, tpr_sampled_problem, tpr_bound_source, tpr_chain, tpr_payload, tpr_chain_points, tpr_mount,
                 tpr_joint_sections)
        # One table of signatures, all returning int.  The entries that do not end in a stream ...
        signatures = {"tpr_abi_sizes": [C.POINTER(C.c_int32)] * 3, "tpr_solve_batch_timed": [P, R, V, I, C.POINTER(C.c_float)]}
        signatures.update({struct.__name__ + "_bytes": [] for struct in sized})
        # ... and (..., void *stream).  The five passes on their four sources: a source's leading arguments (the problem; the
        # boxed entries' low, high), the pass's own, ...
        passes = {"solve": [R], "solve_desired_duration": [V, C.c_double, R, V], "controllable_sets": [V, V, V],
                  "feasible_sets": [V], "reachable_sets": [V, V, V, V]}
        streamed = {"tpr_%s%s_batch" % (name, source): lead + own
                    for source, lead in (("", [P]), ("_dense", [DP]), ("_sampled", [SP]), ("_sampled_boxed", [SP, V, V]))
                    for name, own in passes.items()}
        # ... the other solver entries ...
        streamed.update({
            "tpr_robust_solve_batch": [P, V, R, V],
            "tpr_constraint_params_batch": [P, V, V, V, V, V, V, V, V],
            "tpr_solve_stagewise_batch": [P, V, V, V, V, I, V],
            "tpr_lp1d_batch": [I, I] + [V] * 9,
            "tpr_lp2d_batch": [I, I] + [V] * 11,
            "tpr_spline_fit_batch": [I, I, I, V, I, V, I, I, V, V, V, I],
            "tpr_const_accel_times_batch": [P, V, V, V],
            "tpr_const_accel_eval_batch": [P, V, V, V, I, V, I, V],
            "tpr_param_spline_batch": [P, V, V, V, V],
            "tpr_param_spline_sample_batch": [P, V, I, V, I, I, V, V, V, V],
            "tpr_param_spline_samples_batch": [SP, V, V, V, V],
            "tpr_ppoly_eval_batch": [I, I, I, V, V, V, I, V, I, V, I],
            "tpr_path_eval_batch": [P, V, V, V],
            "tpr_second_order_rows_batch": [P, I, SO, V, V, V, V, V, V],
            "tpr_sampled_rows_batch": [SP, I, SO, V, V, V, V, V, V, V],
            "tpr_stage_boxes_batch": [I, I, I, V, I, BS, I, V, V]})
        # ... and the rigid-body family: (..., int flags, void *stream)
        streamed.update({name: argtypes + [I] for name, argtypes in {
                "tpr_chain_inverse_dynamics_batch": [CP, LL, V, V, V, V],
                "tpr_chain_torque_terms_batch": [CP, I, I, V, V, V, V, V, V],
                "tpr_chain_tool_velocity_batch": [CP, I, I, V, V, V, V, V, V],
                "tpr_chain_tool_acceleration_batch": [CP, LL, V, V, V, V],
                "tpr_chain_tool_acceleration_terms_batch": [CP, I, I, V, V, V, V, V],
                "tpr_chain_tool_wrench_batch": [CP, PP, LL, V, V, V, V],
                "tpr_chain_tool_wrench_terms_batch": [CP, PP, I, I, V, V, V, V, V, V],
                "tpr_chain_points_speed_batch": [CP, XP, I, I, V, V, V, V, V],
                "tpr_chain_points_acceleration_batch": [CP, XP, LL, V, V, V, V],
                "tpr_chain_points_acceleration_terms_batch": [CP, XP, I, I, V, V, V, V, V],
                "tpr_tree_inverse_dynamics_batch": [CP, V, LL, V, V, V, V],
                "tpr_tree_torque_terms_batch": [CP, V, I, I, V, V, V, V, V, V],
                "tpr_tree_base_wrench_batch": [CP, V, MP, LL, V, V, V, V],
                "tpr_tree_base_wrench_terms_batch": [CP, V, MP, I, I, V, V, V, V, V, V],
                "tpr_tree_joint_wrench_batch": [CP, V, JP, LL, V, V, V, V],
                "tpr_tree_joint_wrench_terms_batch": [CP, V, JP, I, I, V, V, V, V, V, V],
                "tpr_tree_momentum_batch": [CP, V, MP, C.c_uint32, I, I, V, V, V, V, V, V]}.items()})
        signatures.update({name: argtypes + [V] for name, argtypes in streamed.items()})

        def declare(name):
            entry = getattr(L, name)
            entry.restype, entry.argtypes = C.c_int, signatures[name]
            return entry

        # the sizes first: a library built from another header is refused as such, not at an entry it lacks
        sizes = [C.c_int32(0), C.c_int32(0), C.c_int32(0)]
        declare("tpr_abi_sizes")(*[C.byref(v) for v in sizes])
        mine = [C.sizeof(tpr_problem), C.sizeof(tpr_result), C.sizeof(tpr_dense_problem)]
        if [v.value for v in sizes] != mine:
            raise ToppraHipError("libtoppra_hip.so was built from another header: its tpr_problem / tpr_result / "
                                 "tpr_dense_problem take %s bytes, this binding declares %s" % ([v.value for v in sizes], mine))
        for struct in sized:
            size = declare(struct.__name__ + "_bytes")
            if size() != C.sizeof(struct):
                raise ToppraHipError("libtoppra_hip.so was built from another header: its %s takes %d bytes, this "
                                     "binding declares %d" % (struct.__name__, size(), C.sizeof(struct)))
        for name in signatures:
            declare(name)
        _lib = L
        return _lib


def last_error():
    return load().tpr_last_error().decode()


def check(rc):
    if rc != 0:
        raise ToppraHipError("libtoppra_hip: %s (code %d)" % (last_error(), rc))


def init(device=None):
    """Make ``device`` the default device of the calling thread's host-pointer calls; raises ToppraHipError when no
    gfx950 device is usable.  The library never moves HIP's current device for its caller: every entry point scopes
    itself to the device its data lives on (the device of the pointers, or this default for host arrays) and puts
    the caller's device back.  Called on every entry -- it is one table look-up plus, the first time a device is
    seen, the gfx950 check.  ``device=None``: the device of the last call, or LOCAL_RANK on the first."""
    global _inited_device
    L = load()
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if _inited_device is None else _inited_device
    check(L.tpr_init(int(device)))
    _inited_device = int(device)
    return _inited_device


def device_count():
    return load().tpr_device_count()


# --------------------------------------------------------------------------------------------
# argument marshalling: numpy (host) or torch CUDA tensors (device, zero-copy)

def is_torch_cuda(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda") and x.is_cuda


def f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def ptr(x):
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr()


def per_traj_vector(name, arr, B, like):
    """A per-trajectory vector ([B], or a scalar broadcast to it) as a contiguous fp64 array of the kind of ``like``, on its
    device: sd_start / sd_end of the builders, sdmin / sdmax / desired_duration / limit of the batch entries."""
    if is_torch_cuda(like):
        import torch
        if not (hasattr(arr, "is_cuda") and arr.is_cuda):
            arr = torch.as_tensor(arr, dtype=torch.float64, device=like.device)
        check_tensor(name, arr, like)
        if arr.ndim == 0:
            arr = arr.expand(B)
        if tuple(arr.shape) != (B,):
            raise ValueError("%s must be a scalar or have shape [B] = [%d], got %s" % (name, B, tuple(arr.shape)))
        return arr.contiguous()
    arr = np.asarray(arr, dtype=np.float64)
    if arr.ndim == 0:
        arr = np.broadcast_to(arr, (B,))
    if arr.shape != (B,):
        raise ValueError("%s must be a scalar or have shape [B] = [%d], got %s" % (name, B, arr.shape))
    return np.ascontiguousarray(arr)


def _limits(p, keep, conv, vlim, alim, interpolation):
    """vlim / alim [B, d, 2] of a spline-table or sampled problem ``p``: checked, kept, pointed to; returns their flag bits."""
    flags = 0
    for name, arr, flag in (("vlim", vlim, HAS_VELOCITY), ("alim", alim, HAS_ACCELERATION)):
        if arr is not None:
            arr = conv(name, arr)
            if tuple(arr.shape) != (p.B, p.d, 2):
                raise ValueError("%s must have shape [B, d, 2] = [%d, %d, 2], got %s" % (name, p.B, p.d, tuple(arr.shape)))
            keep.append(arr)
            setattr(p, name, ptr(arr))
            flags |= flag
    if alim is not None and interpolation:
        flags |= ACC_INTERPOLATION
    return flags


def _finish(p, keep, like, sd_start, sd_end, active):
    """What every builder ends with: sd_start / sd_end as per-trajectory vectors and ``active``, the [B, 4] int32 warm-start
    state of the reference's wrapper object (updated in place), checked, kept and pointed to by ``p``: (p, keep)."""
    for name, arr in (("sd_start", sd_start), ("sd_end", sd_end)):
        if arr is not None:
            arr = per_traj_vector(name, arr, p.B, like)
            keep.append(arr)
            setattr(p, name, ptr(arr))
    if active is not None:
        keep.append(_check_active(active, p.B, like, is_torch_cuda(like)))
        p.active = ptr(active)
    return p, keep


def make_dense_problem(a, b, c, low, high, deltas, sd_start=None, sd_end=None, squared=False, keep=None, active=None):
    """Build a tpr_dense_problem from the arrays of the reference's seidelWrapper (all numpy or all torch-CUDA):
    a, b, c [B, N+1, nC] (a_arr, b_arr, c_arr: nC counts the two reserved x_next rows), low, high [B, N+1, 2],
    deltas [N] or [B, N], sd_start / sd_end scalars or [B], active [B, 4] int32 (the wrapper object's warm-start state,
    in / out).  Shapes and dtypes are validated here: the C-ABI takes raw pointers."""
    dev = is_torch_cuda(a)
    keep = keep if keep is not None else []
    conv = converter(a, "a")
    a = conv("a", a)
    if a.ndim != 3:
        raise ValueError("a must have shape [B, N+1, nC]")
    B, N1, nC = (int(s) for s in a.shape)
    N = N1 - 1
    if N < 1:
        raise ValueError("dense rows need at least two gridpoints")
    if not 2 <= nC <= MAX_DENSE_ROWS:
        raise ValueError("nC = %d rows per stage (incl. the two x_next rows) is outside 2..%d" % (nC, MAX_DENSE_ROWS))
    b, c = conv("b", b), conv("c", c)
    low, high = conv("low", low), conv("high", high)
    for name, arr, shape in (("b", b, (B, N1, nC)), ("c", c, (B, N1, nC)), ("low", low, (B, N1, 2)), ("high", high, (B, N1, 2))):
        if tuple(arr.shape) != shape:
            raise ValueError("%s must have shape %s, got %s" % (name, shape, tuple(arr.shape)))
    deltas = conv("deltas", deltas)
    if deltas.ndim == 1:
        if int(deltas.shape[0]) != N:
            raise ValueError("deltas must have N = %d entries" % N)
        deltas = (deltas.unsqueeze(0).expand(B, N) if dev else np.broadcast_to(deltas, (B, N)))
        deltas = deltas.contiguous() if dev else np.ascontiguousarray(deltas)
    if tuple(deltas.shape) != (B, N):
        raise ValueError("deltas must have shape [N] or [B, N] = [%d, %d], got %s" % (B, N, tuple(deltas.shape)))
    p = tpr_dense_problem(B=B, N=N, nC=nC, flags=(DEVICE_PTRS if dev else 0) | (BOUNDARY_SQUARED if squared else 0))
    keep += [a, b, c, low, high, deltas]
    p.a, p.b, p.c, p.low, p.high, p.deltas = ptr(a), ptr(b), ptr(c), ptr(low), ptr(high), ptr(deltas)
    return _finish(p, keep, a, sd_start, sd_end, active)


def converter(like, like_name):
    """``conv(name, x)`` for the arrays of one call: a contiguous fp64 numpy array when ``like`` is a host array; when it is a
    torch CUDA tensor, ``x`` checked to be an fp64 tensor on like's device, made contiguous."""
    if is_torch_cuda(like):
        def conv(name, x):
            if not (hasattr(x, "is_cuda") and x.is_cuda):
                raise ValueError("%s must be a CUDA tensor like %s (mixing host and device arrays is not supported)" % (name, like_name))
            check_tensor(name, x, like)
            return x.contiguous()
        return conv
    return lambda name, x: f64(x)


def _check_active(active, B, like, dev):
    """[B, 4] int32 warm-start state of the reference's wrapper object, updated in place."""
    if dev:
        import torch
        if not (hasattr(active, "is_cuda") and active.is_cuda) or active.device != like.device or \
                active.dtype != torch.int32 or tuple(active.shape) != (B, 4) or not active.is_contiguous():
            raise ValueError("active must be a contiguous int32 tensor [B, 4] on the problem's device")
    elif not (isinstance(active, np.ndarray) and active.dtype == np.int32 and active.shape == (B, 4)
              and active.flags["C_CONTIGUOUS"]):
        raise ValueError("active must be a C-contiguous int32 array [B, 4] (it is updated in place)")
    return active


def sampled_rows_per_stage(d, alim, interpolation):
    """nC of a sampled problem without second-order blocks: the two x_next rows and the acceleration block."""
    return 2 + ((4 if interpolation else 2) * d if alim is not None else 0)


def check_row_limit(nC):
    """The refusal of a constraint list with more rows per stage than the dense-row kernels hold."""
    if nC > MAX_DENSE_ROWS:
        raise NotImplementedError("%d constraint rows per stage (incl. the two x_next rows): the dense-row kernels hold %d"
                                  % (nC, MAX_DENSE_ROWS))


def make_sampled_problem(grid, q, qs, qss, vlim, alim, sd_start=None, sd_end=None, interpolation=True, keep=None,
                         active=None, squared=False, solver=True):
    """Build a tpr_sampled_problem -- a geometric path given as samples at the gridpoints -- from arrays (all numpy or all
    torch-CUDA): grid [N+1] or [B, N+1] (strictly increasing); q (may be None), qs, qss [B, N+1, d]: path(grid),
    path(grid, 1), path(grid, 2) (qss may be None too with ``solver=False``: the spline
    parametrizer reads q and qs only); vlim / alim [B, d, 2] or None; sd_start / sd_end scalars or [B]; active [B, 4] int32
    (in / out).  Everything that can be refused from shapes alone is refused here, before any launch: ``solver`` (the fused
    passes) holds 122 rows per stage -- d <= 30 under Interpolation, d <= 32 otherwise."""
    dev = is_torch_cuda(qs)
    keep = keep if keep is not None else []
    conv = converter(qs, "qs")
    qs = conv("qs", qs)
    if qs.ndim != 3:
        raise ValueError("qs must have shape [B, N+1, d], got %s" % (tuple(qs.shape),))
    B, N1, d = (int(v) for v in qs.shape)
    N = N1 - 1
    if N < 1:
        raise ValueError("a sampled path needs at least two gridpoints")
    if not 1 <= d <= MAX_DOF:
        raise NotImplementedError("dof %d is outside 1..%d" % (d, MAX_DOF))
    if qss is None and solver:
        raise ValueError("the solver passes need qss = path(grid, 2)")
    qss = None if qss is None else conv("qss", qss)
    q = None if q is None else conv("q", q)
    for name, arr in (("qss", qss), ("q", q)):
        if arr is not None and tuple(arr.shape) != (B, N1, d):
            raise ValueError("%s must have the shape of qs, [B, N+1, d] = [%d, %d, %d], got %s" % (name, B, N1, d, tuple(arr.shape)))
    grid = conv("grid", grid)
    if tuple(grid.shape) not in ((N1,), (B, N1)):
        raise ValueError("grid must have shape [N+1] or [B, N+1] = [%d, %d], got %s" % (B, N1, tuple(grid.shape)))
    if not dev and not np.all(np.diff(grid, axis=-1) > 0):  # device grids are the caller's responsibility
        raise ValueError("grid must be strictly increasing")
    if solver and sampled_rows_per_stage(d, alim, interpolation) > MAX_DENSE_ROWS:
        raise NotImplementedError("%d dof under Interpolation: %d constraint rows per stage (incl. the two x_next rows), the "
                                  "sampled passes hold %d (30 dof; 32 under Collocation)"
                                  % (d, sampled_rows_per_stage(d, alim, interpolation), MAX_DENSE_ROWS))
    flags = (DEVICE_PTRS if dev else 0) | (BOUNDARY_SQUARED if squared else 0) | (GRID_PER_TRAJ if grid.ndim == 2 else 0)
    p = tpr_sampled_problem(B=B, d=d, N=N, flags=0)
    keep += [grid, q, qs, qss]
    p.grid, p.q, p.qs, p.qss = ptr(grid), ptr(q), ptr(qs), ptr(qss)
    p.flags = flags | _limits(p, keep, conv, vlim, alim, interpolation)
    return _finish(p, keep, qs, sd_start, sd_end, active)


def _no_nan(name, arr):
    """Host bounds are checked for NaN (a NaN loses every comparison of the fold and would silently drop the bound); device
    tensors are not read back: NaN bounds there are the caller's error, as NaN samples are."""
    if isinstance(arr, np.ndarray) and np.isnan(arr).any():
        raise ValueError("%s holds NaN (use +-inf for 'no bound')" % name)
    return arr


def make_bound_sources(sources, B, N, d, conv):
    """The ``sources`` of :func:`toppra_amd.batch.stage_boxes_batch` -- an ordered list of ``(kind, array)`` with kind
    "vlim" ([B, d, 2] or [d, 2]), "vlim_grid" ([B, N+1, d, 2] or [N+1, d, 2]), "xbound" / "ubound" ([B, N+1, 2] or [N+1, 2]);
    the shorter shape is one array for the whole batch -- as tpr_bound_source structures: (structs, the converted arrays
    they point to).  Shapes are checked here, numpy arrays also for NaN (+-inf is allowed).  ``d`` is None without samples:
    velocity sources are refused then."""
    sources = list(sources)
    if len(sources) > BOUND_MAX_SOURCES:
        raise NotImplementedError("%d bound sources in one list: the box kernel takes %d" % (len(sources), BOUND_MAX_SOURCES))
    structs = (tpr_bound_source * max(len(sources), 1))()
    keep = []
    for j, (kind, arr) in enumerate(sources):
        if kind not in BOUND_KINDS:
            raise ValueError("sources[%d]: unknown kind %r (one of %s)" % (j, kind, sorted(BOUND_KINDS)))
        name = "sources[%d] (%s)" % (j, kind)
        arr = _no_nan(name, conv(name, arr))
        if kind in ("vlim", "vlim_grid"):
            if d is None:
                raise ValueError("%s needs qs = path(grid, 1)" % name)
            if d > MAX_DOF:
                raise NotImplementedError("%s: dof %d is outside 1..%d" % (name, d, MAX_DOF))
            full = (B, d, 2) if kind == "vlim" else (B, N + 1, d, 2)
        else:
            full = (B, N + 1, 2)
        shape = tuple(int(v) for v in arr.shape)
        if shape not in (full, full[1:]):
            raise ValueError("%s must have shape %s or %s, got %s" % (name, list(full), list(full[1:]), shape))
        keep.append(arr)
        structs[j] = tpr_bound_source(kind=BOUND_KINDS[kind], flags=BOUND_SHARED if shape == full[1:] and full != full[1:] else 0,
                                      data=ptr(arr))
    return structs, keep


def make_boxed_problem(grid, qs, qss, alim, low, high, sd_start=None, sd_end=None, interpolation=True, keep=None, active=None,
                       squared=False, vlim=None):
    """The tpr_sampled_problem of the boxed passes (no velocity limits: the boxes carry every first-order constraint) and the
    checked boxes: (problem, keep, low, high).  low, high [B, N+1, 2] as :func:`toppra_amd.batch.stage_boxes_batch` returns
    them; numpy boxes are checked for NaN.  Everything is refused here, before any launch."""
    if vlim is not None:
        raise NotImplementedError("the boxed passes take no vlim: the boxes carry every first-order constraint -- make the "
                                  "limits a (\"vlim\", vlim) source of stage_boxes_batch")
    p, keep = make_sampled_problem(grid, None, qs, qss, None, alim, sd_start, sd_end, interpolation, keep=keep, active=active,
                                   squared=squared)
    conv = converter(keep[2], "qs")
    out = []
    for name, arr in (("low", low), ("high", high)):
        arr = _no_nan(name, conv(name, arr))
        if tuple(int(v) for v in arr.shape) != (p.B, p.N + 1, 2):
            raise ValueError("%s must have shape [B, N+1, 2] = [%d, %d, 2], got %s" % (name, p.B, p.N + 1, tuple(arr.shape)))
        out.append(arr)
    keep += out
    return p, keep, out[0], out[1]


def check_tensor(name, t, like):
    """Device tensors are passed to the kernels as raw pointers: they must be fp64 and live on the
    same device as ``coef``."""
    import torch
    if t.dtype != torch.float64:
        raise ValueError("%s must be float64 (got %s): the kernels read raw fp64 pointers" % (name, t.dtype))
    if not t.is_cuda or t.device != like.device:
        raise ValueError("%s must live on %s like coef (got %s)" % (name, like.device, t.device))


def check_weight(S):
    """The weight of v' S v must be symmetric positive semi-definite: an indefinite one can make the form negative and its
    bound limit / v' S v an empty box.  A device tensor is read back (36 doubles)."""
    host = S.detach().cpu().numpy() if hasattr(S, "detach") else np.asarray(S, dtype=np.float64)
    if not np.all(np.isfinite(host)) or not np.array_equal(host, host.T):
        raise ValueError("S must be finite and symmetric")
    eig = np.linalg.eigvalsh(host)
    if eig.min() < -1e-12 * max(abs(eig).max(), 1e-300):
        raise ValueError("S must be positive semi-definite (smallest eigenvalue %g)" % eig.min())


def make_problem(coef, breaks, grid, vlim, alim, sd_start=None, sd_end=None, interpolation=True,
                 variant=0, keep=None, strict=False, active=None, squared=False, sound=False):
    """Build a tpr_problem from arrays (all numpy or all torch-CUDA).  `keep` collects the
    converted arrays so they outlive the call.  Shapes and dtypes are validated here -- the C-ABI
    takes raw pointers and sizes, so a short or mistyped array would be read out of bounds:
    coef [B,4,nseg,d]; breaks [nseg+1] or [B,nseg+1]; grid [N+1] or [B,N+1] (strictly increasing);
    vlim/alim [B,d,2]; sd_start/sd_end scalars or [B]; active [B,4] int32 (in/out).  Device tensors must be float64
    on coef's device."""
    dev = is_torch_cuda(coef)
    keep = keep if keep is not None else []
    conv = converter(coef, "coef")
    coef = conv("coef", coef)
    breaks = conv("breaks", breaks)
    grid = conv("grid", grid)
    if coef.ndim != 4 or coef.shape[1] != 4:
        raise ValueError("coef must have shape [B, 4, nseg, d]")
    B, _, nseg, d = (int(s) for s in coef.shape)
    if grid.ndim not in (1, 2) or (grid.ndim == 2 and int(grid.shape[0]) != B):
        raise ValueError("grid must have shape [N+1] or [B, N+1] with B = %d, got %s" % (B, tuple(grid.shape)))
    if breaks.ndim not in (1, 2) or (breaks.ndim == 2 and int(breaks.shape[0]) != B):
        raise ValueError("breaks must have shape [nseg+1] or [B, nseg+1] with B = %d, got %s" % (B, tuple(breaks.shape)))
    N = int(grid.shape[-1]) - 1
    if N < 1:
        raise ValueError("grid needs at least two gridpoints")
    if not dev and not np.all(np.diff(grid, axis=-1) > 0):  # device grids are the caller's responsibility
        raise ValueError("grid must be strictly increasing")
    flags = (DEVICE_PTRS if dev else 0) | (STRICT_SEIDEL if strict else 0) | (BOUNDARY_SQUARED if squared else 0) | \
        (SOUND_CERTIFICATES if sound else 0)
    if breaks.ndim == 2:
        flags |= BREAKS_PER_TRAJ
    if grid.ndim == 2:
        flags |= GRID_PER_TRAJ
    if int(breaks.shape[-1]) != nseg + 1:
        raise ValueError("breaks must have nseg+1 entries")
    p = tpr_problem(B=B, d=d, nseg=nseg, N=N, flags=0, variant=int(variant))
    keep += [coef, breaks, grid]
    p.coef, p.breaks, p.grid = ptr(coef), ptr(breaks), ptr(grid)
    p.flags = flags | _limits(p, keep, conv, vlim, alim, interpolation)
    return _finish(p, keep, coef, sd_start, sd_end, active)

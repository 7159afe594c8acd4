/*
 * toppra_hip.h -- C-ABI of the MI355X-native batched TOPP-RA "seidel" path.
 *
 * This is the drop-in boundary: a plain-C shared library (libtoppra_hip.so) with no torch or
 * Python types in its signatures.  Each entry point names the reference interface it replaces
 * (paths relative to the reference root, hungpham2511/toppra v0.6.2).  The reference calls its
 * solver once per stage from Python (3N calls per trajectory); this library takes over at the
 * *pass* level and adds the batch dimension, so one call solves B independent trajectories.
 *
 * Layouts are trajectory-major, C-contiguous, fp64 (int32 for status / active sets):
 *   coef   [B][4][nseg][d]   scipy CubicSpline.c of each path (interpolator.py:419), highest
 *                            power first
 *   breaks [nseg+1]          spline breakpoints (CubicSpline.x); [B][nseg+1] with
 *                            TPR_BREAKS_PER_TRAJ
 *   grid   [N+1]             path discretisation; [B][N+1] with TPR_GRID_PER_TRAJ
 *   vlim   [B][d][2]         JointVelocityConstraint.vlim      (linear_joint_velocity.py:19-28)
 *   alim   [B][d][2]         JointAccelerationConstraint.alim  (linear_joint_acceleration.py:46-52)
 *                            Infinite and arbitrarily large or small limits are valid inputs; NaN limits are the caller's
 *                            error (the reference rejects them); the velocity bound is computed in fp32 as the reference
 *                            computes it, fp32 overflow and gradual underflow (subnormal squares, exact zeros) included.
 *   sd_start, sd_end [B]     boundary path velocities (NULL = 0)
 *
 * Buffers belong to the caller.  Pointers are host pointers unless TPR_DEVICE_PTRS is set, in
 * which case every pointer in tpr_problem/tpr_result is a device pointer on the current device
 * and the call is asynchronous on `stream` (a hipStream_t passed as void*, NULL = default).
 *
 * Numerical failure is data, not an error code, exactly as in the reference: the per-trajectory
 * status is TPR_STATUS_* and failed outputs are NaN-filled.  The int return value reports API
 * misuse only (0 = ok, negative = error; text via tpr_last_error()).
 */
#ifndef TOPPRA_HIP_H
#define TOPPRA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPR_MAX_DOF 32      /* generic lane-per-trajectory kernel (rows per LP: nC = 2 + 4*d <= 130)          */
#define TPR_MAX_DOF_FAST 16 /* rows-across-lanes kernels (auto at 14..16 dof and for mid-size batches); 17..32 dof: family 4 / 1 */

/* tpr_problem.flags */
#define TPR_HAS_VELOCITY 1      /* JointVelocityConstraint present                             */
#define TPR_HAS_ACCELERATION 2  /* JointAccelerationConstraint present                         */
#define TPR_ACC_INTERPOLATION 4 /* DiscretizationType.Interpolation (reference default), else Collocation */
#define TPR_DEVICE_PTRS 8
#define TPR_BREAKS_PER_TRAJ 16
#define TPR_GRID_PER_TRAJ 32
/* bit 64 is reserved (it selected an approximate mode in round 1, retired: every path is bit-exact now) */
/* sd_start / sd_end (and sdmin / sdmax of tpr_controllable_sets_batch) hold the SQUARED boundary velocities
 * x = sd^2, squared by the caller.  The reference squares them with Python's `**` (reachability_algorithm.py:226,
 * :262): libm pow() for Python floats, which is not correctly rounded (one ulp off sd * sd for ~0.08 % of the
 * values), numpy's sd * sd for arrays.  Without the flag the device computes sd * sd; a caller that must reproduce
 * the Python-float case squares in that very expression and sets the flag (toppra_amd.algorithm.TOPPRA does).
 * Honoured by tpr_solve_batch, tpr_controllable_sets_batch, tpr_solve_desired_duration_batch.                  */
#define TPR_BOUNDARY_SQUARED 256
/* Force every stage LP through the full Seidel iteration (served by the rows-across-lanes kernels).
 * By default the throughput kernels answer a backward LP from a certificate -- the reference's own pivot trace followed
 * with margins far above the solver's tolerances, the final vertex verified against every row, and the reference's
 * last-pivot formulas evaluated for it; what is not predictable runs the full iteration.  Both give the same bits
 * (tests/test_gpu_fullsize.py on the GPU, tests/test_host_cert.py on the CPU: the certificate source against the
 * restatement of the reference, stage LP by stage LP); this flag exists for A/B testing and for callers who want the
 * iteration itself replicated.                                                                     */
#define TPR_STRICT_SEIDEL 128
/* Accepted and ignored since round 4: every kernel family certifies a stage LP only where the reference's WHOLE pivot
 * sequence is predictable (rounds 2-3 had a faster default that bounded the reference's last pivot only and could return
 * an LP's optimum where an earlier pivot of the reference ends its run with "infeasible" -- a 1e-14 sliver, 1 in 1.5e5
 * trajectories of an adversarial family).  Family 3 follows the trace at lane level (prologue pivots, the slide along the
 * limiting row as prefix records: DESIGN.md section 3.1), family 2 certifies a moved pair after one predictable pivot,
 * family 4 the kept pair only; everything else runs the reference's iteration.                                       */
#define TPR_SOUND_CERTIFICATES 512

/* per-trajectory status == ParameterizationReturnCode (algorithm/algorithm.py:49-62) */
#define TPR_STATUS_OK 0
#define TPR_STATUS_FAIL_UNCONTROLLABLE 1
#define TPR_STATUS_ERR_UNKNOWN 2

/* API error codes */
#define TPR_E_OK 0
#define TPR_E_BADARG (-1)
#define TPR_E_HIP (-2)
#define TPR_E_UNSUPPORTED (-3)

typedef struct tpr_problem {
    int32_t B, d, nseg, N;
    int32_t flags;
    int32_t variant; /* kernel selection: 0 = auto, 1 = generic lane-per-trajectory, 2 = rows-across-lanes,
                        3 = lane-per-trajectory certificates (d <= 15; sd2, u, status required),
                        4 = one trajectory per wave (the latency kernel: any dof, N <= 1480; auto for
                            small batches),
                        5 = two trajectories per wave, 32 lanes each (the fused solve for 1..7 dof, N <= ~800;
                            auto between 1536 and 9215 trajectories) */
    const double *coef;
    const double *breaks;
    const double *grid;
    const double *vlim;
    const double *alim;
    const double *sd_start;
    const double *sd_end;
    int32_t *active; /* [B][4] = active_c_up[2], active_c_down[2] (may be NULL = a fresh object): the warm-start
                        state of the reference's seidelWrapper OBJECT (cy_seidel_solverwrapper.pyx:526-527), which
                        persists across the passes run on one instance and is also written by the forward pass's
                        1-D path (:646-649).  Read at the start and updated at the end of tpr_solve_batch,
                        tpr_controllable_sets_batch and tpr_feasible_sets_batch, so that a sequence of passes on one
                        object (examples/plot_kinematics.py:48,72) returns the reference's bits.  Maintained by kernel
                        family 4 (auto-selected when set) and, where that family cannot take the problem (N > 1480),
                        by the generic lane kernel (family 1, auto-selected then); forcing variant 2 or 3 together
                        with a non-NULL state is refused (TPR_E_UNSUPPORTED): those families neither read nor update
                        it.  The other entries ignore it (tpr_solve_stagewise_batch takes its own argument). */
} tpr_problem;

typedef struct tpr_result {
    double *sd2;     /* [B][N+1]    x_i = sd_i^2           (may be NULL)                          */
    double *sd;      /* [B][N+1]    sd_vec = sqrt(x)       (may be NULL)                          */
    double *u;       /* [B][N]      sdd_vec                (may be NULL; tpr_solve_batch keeps it in a
                                                            workspace then, like K)                 */
    double *K;       /* [B][N+1][2] controllable sets      (may be NULL for tpr_solve_batch: kept in
                                                            a stream-ordered workspace then)        */
    int32_t *status; /* [B]                                (may be NULL)                          */
} tpr_result;

/* Library / device management.  tpr_init(device) verifies that `device` is a gfx950 GPU and makes it
 * the default device of the CALLING THREAD's host-pointer calls (a thread that never called tpr_init
 * uses the device of the process's last tpr_init); it must succeed once before any other call and
 * fails (TPR_E_HIP / TPR_E_UNSUPPORTED) otherwise.  The calling thread's current HIP device is NOT
 * changed: every entry point runs on the device its data lives on -- the device of the pointers with
 * TPR_DEVICE_PTRS, the thread's tpr_init device otherwise -- and restores the caller's device on
 * return, so the library is safe next to frameworks (torch) that move the per-thread current device,
 * and threads working on different GPUs do not disturb each other.                                 */
int tpr_init(int device);
int tpr_device_count(void);
const char *tpr_last_error(void);
const char *tpr_version(void);
/* ABI guard (0.2): the structures of this header grow at their END from version to version (tpr_problem.active and
 * tpr_dense_problem.active joined in 0.2); a binding built against an older header would hand over a shorter structure
 * and the library would read past it.  A binding compares these sizes (bytes of tpr_problem, tpr_result,
 * tpr_dense_problem; NULL to skip one) with its own declarations before its first compute call.  Returns the ABI
 * revision (2).                                                                                                      */
int tpr_abi_sizes(int32_t *problem_bytes, int32_t *result_bytes, int32_t *dense_problem_bytes);

/* Replaces ReachabilityAlgorithm.compute_parameterization (+ TOPPRA._forward_step) for B
 * trajectories: algorithm/reachabilitybased/reachability_algorithm.py:240-376,
 * time_optimal_algorithm.py:55-92, including seidelWrapper.__init__'s
 * compute_constraint_params (cy_seidel_solverwrapper.pyx:425-531) which is fused in.            */
int tpr_solve_batch(const tpr_problem *p, const tpr_result *r, void *stream);

/* Replaces TOPPRAsd.compute_parameterization (algorithm/reachabilitybased/
 * desired_duration_algorithm.py:42-234) for B trajectories: the backward scan, the "fastest" and
 * "slowest" forward scans, the duration bisection on their convex combination (absolute tolerance
 * atol, reference default 1e-5) and the blended sd^2 / u.  desired [B] seconds; alpha [B] (may be
 * NULL) receives the blend factor.  Same result struct and status codes as tpr_solve_batch; up to 16 dof.
 * p->variant: 0 = auto -- from 9216 trajectories (9..15 dof: 14336 .. 36864) the certified lane kernel runs the
 * backward scan and both forward profiles in ONE launch, the rows-across-lanes kernels otherwise; 2 / 3 force one.
 * Bisection and blend: one wave per trajectory.                                                      */
int tpr_solve_desired_duration_batch(const tpr_problem *p, const double *desired, double atol,
                                     const tpr_result *r, double *alpha, void *stream);

/* Robust TOPP-RA (BASELINE config 4) -- PARITY UNPINNED against ECOS (absent here; the
 * reference holds no golden vectors for it); cross-checked at 1e-7 against an independent exact solver
 * (oracle/robust_independent.py, tests/test_gpu_robust.py); see csrc/tpr_robust.hip.inc.  Replaces
 * TOPPRA([JointVelocityConstraint, RobustLinearConstraint(JointAccelerationConstraint, ellipsoid)],
 * ..., solver_wrapper="ecos"): compute_parameterization (+ compute_feasible_sets into X when X !=
 * NULL) with the stage problems ecosWrapper.solve_stagewise_optim builds
 * (solverwrapper/ecos_solverwrapper.py:90-207, constraint/conic_constraint.py:19-26) solved exactly
 * instead of by ECOS's interior-point iteration.  ellipsoid = (ru, rx, rc) axes lengths.  The
 * acceleration discretisation follows p->flags (TPR_ACC_INTERPOLATION or Collocation).  p->variant: 0 = auto (rows
 * across lanes up to 16 dof -- Interpolation or Collocation, with or without X --, the generic one-trajectory-per-lane
 * kernel above), 1 = the generic kernel; same bits.                                                   */
int tpr_robust_solve_batch(const tpr_problem *p, const double *ellipsoid, const tpr_result *r, double *X,
                           void *stream);

/* Replaces ReachabilityAlgorithm.compute_controllable_sets(sdmin, sdmax)
 * (reachability_algorithm.py:166-238).  sdmin/sdmax [B]; K [B][N+1][2].  Kernel selection and flags as
 * tpr_solve_batch (backward scan only).                                                           */
int tpr_controllable_sets_batch(const tpr_problem *p, const double *sdmin, const double *sdmax,
                                double *K, void *stream);

/* Replaces ReachabilityAlgorithm.compute_feasible_sets (reachability_algorithm.py:131-164).
 * X [B][N+1][2].  p->variant: 0 = auto (one wave per trajectory for a handful of trajectories, above 16 dof or with
 * p->active; the certified lane kernel from 8192 trajectories up to 8 dof, 14336 .. 36864 at 9 .. 15 dof; rows across lanes
 * otherwise), 1 / 2 / 3 / 4 force a kernel family.  TPR_STRICT_SEIDEL / TPR_SOUND_CERTIFICATES as tpr_solve_batch.   */
int tpr_feasible_sets_batch(const tpr_problem *p, double *X, void *stream);

/* Replaces ReachabilityAlgorithm.compute_reachable_sets(sdmin, sdmax) (reachability_algorithm.py:378-431):
 * the feasible sets, then the forward propagation of the reachable velocities from [sdmin^2, sdmax^2] --
 * including the reference's use of the PREVIOUS interval's delta in the objective (:384) and the warm-start
 * state shared with the feasible-set pass.  sdmin/sdmax [B]; L [B][N+1][2] (zeros after a NaN stage, as in
 * the reference); X [B][N+1][2] feasible sets (may be NULL).                                          */
int tpr_reachable_sets_batch(const tpr_problem *p, const double *sdmin, const double *sdmax, double *L, double *X,
                             void *stream);

/* ---- the seidel path on DENSE rows: any canonical-linear constraint list ------------------------------
 * The entries above regenerate the rows of JointVelocityConstraint + JointAccelerationConstraint from the spline table.
 * seidelWrapper itself is more general (cy_seidel_solverwrapper.pyx:425-531): it flattens ANY list of canonical-linear
 * constraints (SecondOrderConstraint / JointTorqueConstraint with a user's inverse dynamics, varying velocity limits,
 * hand-written a, b, c, F, g) into a_arr, b_arr, c_arr [N+1][nC] (nC counts the two reserved x_next rows 0, 1),
 * low_arr, high_arr [N+1][2] and deltas [N]; solve_stagewise_optim (:549-697) and the scans of
 * reachability_algorithm.py:131-376 read nothing else.  These entries take exactly those arrays for B trajectories
 * (the host side builds them as the reference does: toppra_amd.solverwrapper.dense_rows) and run every stage LP through
 * the reference's full Seidel iteration with its warm-start state (rows across 8 / 16 / 32 lanes per trajectory; nC <= 122).
 * Results are the reference's bits.  flags: TPR_DEVICE_PTRS, TPR_BOUNDARY_SQUARED.                          */
typedef struct tpr_dense_problem {
    int32_t B, N, nC, flags;
    const double *a, *b, *c;         /* [B][N+1][nC]; entries 0, 1 of a stage are ignored (the x_next rows) */
    const double *low, *high;        /* [B][N+1][2]  variable boxes (u, x) */
    const double *deltas;            /* [B][N] */
    const double *sd_start, *sd_end; /* [B] or NULL (zeros) */
    int32_t *active;                 /* [B][4] or NULL: the wrapper object's warm-start state (active_c_up[2], active_c_down[2]),
                                        read at the start of a pass and written back at its end (as tpr_problem.active): passes
                                        chained on ONE object pivot in the reference's order.  NULL = a fresh object. */
} tpr_dense_problem;

/* compute_parameterization (reachability_algorithm.py:240-376): outputs and status codes as tpr_solve_batch (r->K is
 * required; sd2 / sd / u / status may be NULL).                                                            */
int tpr_solve_dense_batch(const tpr_dense_problem *p, const tpr_result *r, void *stream);
/* TOPPRAsd.compute_parameterization (desired_duration_algorithm.py:42-234) on dense rows: as
 * tpr_solve_desired_duration_batch (desired [B] seconds, atol, alpha [B] may be NULL).                       */
int tpr_solve_desired_duration_dense_batch(const tpr_dense_problem *p, const double *desired, double atol,
                                           const tpr_result *r, double *alpha, void *stream);
/* compute_controllable_sets(sdmin, sdmax) (:166-238): K [B][N+1][2]; p->sd_start / sd_end are not used.       */
int tpr_controllable_sets_dense_batch(const tpr_dense_problem *p, const double *sdmin, const double *sdmax, double *K,
                                      void *stream);
/* compute_feasible_sets (:131-164): X [B][N+1][2].                                                          */
int tpr_feasible_sets_dense_batch(const tpr_dense_problem *p, double *X, void *stream);
/* compute_reachable_sets(sdmin, sdmax) (:378-431): as tpr_reachable_sets_batch (L [B][N+1][2]; X may be NULL); one
 * trajectory per lane, the reference's per-stage calls with their stateful warm start.                     */
int tpr_reachable_sets_dense_batch(const tpr_dense_problem *p, const double *sdmin, const double *sdmax, double *L, double *X,
                                   void *stream);

/* Replaces Constraint.compute_constraint_params + the dense row build of seidelWrapper.__init__
 * (linear_joint_velocity.py:43-53, linear_joint_acceleration.py:63-104,
 * linear_constraint.py:164-190, cy_seidel_solverwrapper.pyx:474-520):
 *   a,b,c [B][N+1][nC] (rows 0,1 zero), low, high [B][N+1][2] (the wrapper's variable box),
 *   xbound [B][N+1][2] (the velocity constraint's own x bound, before the +-1e8 box is applied),
 *   qs, qss [B][N+1][d]
 * Any output may be NULL.  nC = 2 + (4d | 2d | 0) by flags.                                      */
int tpr_constraint_params_batch(const tpr_problem *p, double *a, double *b, double *c, double *low,
                                double *high, double *xbound, double *qs, double *qss, void *stream);

/* ---- dense rows of second-order / torque constraints, built on the GPU --------------------------------------
 * Replaces SplineInterpolator.__call__(gridpoints, order) for order 0, 1, 2 (interpolator.py:423-430), the path samples
 * SecondOrderConstraint / JointTorqueConstraint hand to the user's inverse dynamics (linear_second_order.py:146-152,
 * joint_torque.py): q, qs, qss [B][N+1][d] (any may be NULL).  q is scipy PPoly's evaluation of the cubic, qs and qss those of
 * the differentiated coefficient tables (cspl.derivative()): the bits of tpr_constraint_params_batch's qs, qss.  Uses
 * coef / breaks / grid and the flags TPR_DEVICE_PTRS, TPR_BREAKS_PER_TRAJ, TPR_GRID_PER_TRAJ of p.                     */
int tpr_path_eval_batch(const tpr_problem *p, double *q, double *qs, double *qss, void *stream);

/* tpr_second_order_block.flags */
#define TPR_SO_INTERPOLATION 1 /* DiscretizationType.Interpolation for this block, else Collocation                */
#define TPR_SO_F_SHARED 2      /* F [m][p], one for the batch; no F bit = the signed identity [I; -I] (F NULL, m = 2 p) */
#define TPR_SO_F_PER_TRAJ 4    /* F [B][m][p]                                                                       */
#define TPR_SO_F_PER_POINT 8   /* F [B][N+1][m][p]                                                                  */
#define TPR_SO_G_PER_TRAJ 16   /* g [B][m]; no g bit = g [m], one for the batch                                     */
#define TPR_SO_G_PER_POINT 32  /* g [B][N+1][m]                                                                     */
#define TPR_SO_MAX_BLOCKS 8

/* One second-order constraint F w <= g on w = tau(q, qd, qdd) (linear_second_order.py:11-173; JointTorqueConstraint,
 * joint_torque.py:10-116, is the signed identity with g = [tau_max; -tau_min]) as the three inverse-dynamics evaluations
 * that the reference's substitution needs (linear_second_order.py:154-162): w0 = tau(q, 0, 0), wa = tau(q, 0, q'),
 * wb = tau(q, q', q''), each [B][N+1][p].  friction [B][p] (NULL = none; needs p == d): dry friction, friction * sign(q')
 * is added to c.  Pointers follow TPR_DEVICE_PTRS of the problem they are passed with.                              */
typedef struct tpr_second_order_block {
    int32_t p, m, flags, reserved;
    const double *w0, *wa, *wb;
    const double *F, *g;
    const double *friction;
} tpr_second_order_block;
/* ABI guard, as tpr_abi_sizes: bytes of tpr_second_order_block in the library; a binding compares it with its own
 * declaration before its first call of tpr_second_order_rows_batch.                                          */
int tpr_second_order_block_bytes(void);

/* Replaces, for B trajectories, SecondOrderConstraint / JointTorqueConstraint.compute_constraint_params
 * (linear_second_order.py:142-173, joint_torque.py), canonical_to_interpolate (linear_constraint.py:84-192) and the dense
 * row build of seidelWrapper.__init__ (cy_seidel_solverwrapper.pyx:455-520) for the constraint list
 * [velocity (p->vlim), acceleration (p->alim, TPR_ACC_INTERPOLATION), blocks[0], ..., blocks[nblocks-1]]: it writes the
 * complete tpr_dense_problem -- a, b, c [B][N+1][nC] (rows 0, 1 zero, the acceleration block of
 * tpr_constraint_params_batch, then F a, F b, F c - g of each block: m rows under Collocation, 2 m under Interpolation,
 * where stage i holds [a_i | a_{i+1} + (2 delta_i) b_{i+1}] against blkdiag(F_i, F_{i+1}) and the last stage repeats
 * itself), low, high [B][N+1][2] (the +-1e8 box with the velocity constraint's x bound: the values of
 * tpr_constraint_params_batch) and deltas [B][N] (may be NULL).  a = wa - w0, b = wb - w0, c = w0 + friction sign(q'); every
 * operation rounded on its own; a dense F row is summed in index order k = 0 .. p-1, then g is subtracted.
 * nC = 2 + acceleration rows + block rows <= 122; 0 <= nblocks <= TPR_SO_MAX_BLOCKS.                                   */
int tpr_second_order_rows_batch(const tpr_problem *p, int nblocks, const tpr_second_order_block *blocks, double *a,
                                double *b, double *c, double *low, double *high, double *deltas, void *stream);

/* ---- any geometric path: the path given as SAMPLES at the gridpoints -------------------------------------------------
 * The reference's constraints see a path only through path(gridpoints, 1) and path(gridpoints, 2)
 * (linear_joint_velocity.py:48, linear_joint_acceleration.py:72-73, linear_second_order.py:146-152), ParametrizeSpline
 * additionally through path(gridpoints) and the first derivative at the two ends (parametrizer.py:161-196).  A solver fed
 * with these samples therefore returns the reference's bits for ANY AbstractGeometricPath (SimplePath, PolynomialPath,
 * UnivariateSplineInterpolator, a user's own class): nothing of the path's arithmetic is reproduced on the GPU.
 *   grid        [N+1], or [B][N+1] with TPR_GRID_PER_TRAJ
 *   q, qs, qss  [B][N+1][d]: path(grid), path(grid, 1), path(grid, 2); q may be NULL where only the solver is asked.
 *               Samples must be finite: NaN samples are the caller's error, like NaN limits.
 *   vlim, alim, sd_start, sd_end, active: as in tpr_problem.
 * flags: TPR_HAS_VELOCITY, TPR_HAS_ACCELERATION, TPR_ACC_INTERPOLATION, TPR_DEVICE_PTRS, TPR_GRID_PER_TRAJ,
 * TPR_BOUNDARY_SQUARED, with their meanings above.
 * These entries are the dense-row family with the rows generated from the samples.  The fused families 1-5 of
 * tpr_solve_batch (certificates, the cubic evaluated in registers) read a spline table and do not take samples. */
typedef struct tpr_sampled_problem {
    int32_t B, d, N, flags;
    const double *grid;
    const double *q, *qs, *qss;
    const double *vlim, *alim;
    const double *sd_start, *sd_end;
    int32_t *active;
} tpr_sampled_problem;
/* ABI guard, as tpr_second_order_block_bytes: bytes of tpr_sampled_problem in the library.                       */
int tpr_sampled_problem_bytes(void);

/* The counterpart of tpr_constraint_params_batch / tpr_second_order_rows_batch with the samples in place of the spline
 * evaluation (replaces the same reference code: linear_joint_velocity.py:43-53, linear_joint_acceleration.py:63-104,
 * linear_second_order.py:142-173, linear_constraint.py:84-192, cy_seidel_solverwrapper.pyx:455-520): the complete
 * tpr_dense_problem of [velocity, acceleration, blocks[0], ...] -- a, b, c [B][N+1][nC], low, high [B][N+1][2], deltas
 * [B][N] (may be NULL), xbound [B][N+1][2] (may be NULL: the velocity constraint's own x bound, before the +-1e8 box).
 * Every expression after the evaluation of q', q'' is that of the spline entries; same limits (nC <= 122).       */
int tpr_sampled_rows_batch(const tpr_sampled_problem *p, int nblocks, const tpr_second_order_block *blocks, double *a,
                           double *b, double *c, double *low, double *high, double *deltas, double *xbound, void *stream);

/* The passes of the dense family WITHOUT materialised rows: each takes the arguments of its *_dense_batch twin and
 * replaces the same reference code, with a stage's rows produced in registers from qs / qss at gridpoints i and i+1, alim
 * and the velocity box from vlim (4 d doubles read per stage in place of 3 nC).  Results are the bits of the dense pass
 * on the rows tpr_sampled_rows_batch writes (nblocks = 0), warm-start state in and out included.  Limits of the dense
 * family: nC = 2 + 4 d <= 122 under Interpolation (d <= 30), d <= 32 under Collocation or without an acceleration
 * constraint; beyond that TPR_E_UNSUPPORTED.                                                                      */
int tpr_solve_sampled_batch(const tpr_sampled_problem *p, const tpr_result *r, void *stream);
int tpr_solve_desired_duration_sampled_batch(const tpr_sampled_problem *p, const double *desired, double atol,
                                             const tpr_result *r, double *alpha, void *stream);
int tpr_controllable_sets_sampled_batch(const tpr_sampled_problem *p, const double *sdmin, const double *sdmax, double *K,
                                        void *stream);
int tpr_feasible_sets_sampled_batch(const tpr_sampled_problem *p, double *X, void *stream);
int tpr_reachable_sets_sampled_batch(const tpr_sampled_problem *p, const double *sdmin, const double *sdmax, double *L,
                                     double *X, void *stream);

/* ParametrizeSpline (toppra/parametrizer.py:161-196) for a sampled path: as tpr_param_spline_batch's generic variant
 * (1) with the kept samples p->q copied where that variant evaluates the cubic, and the end derivatives p->qs[:, 0] and
 * p->qs[:, N] (the gridpoints must span the path interval, as the reference's do).  sd [B][N+1] -> knot_times
 * [B][N+1], counts [B], coef_t [B][4][N][d]; tpr_ppoly_eval_batch evaluates the result.  p->q and p->qs are required. */
int tpr_param_spline_samples_batch(const tpr_sampled_problem *p, const double *sd, double *knot_times, int32_t *counts,
                                   double *coef_t, void *stream);

/* ---- first-order constraints of any kind: per-stage variable boxes ------------------------------------------------
 * Constraints that only tighten the box of a stage's variables (u, x) = (sdd, sd^2): the `ubound` / `xbound` outputs of
 * compute_constraint_params, which seidelWrapper.__init__ folds into low_arr / high_arr
 * (cy_seidel_solverwrapper.pyx:477-478, 512-520).  A bound source is one such output for the whole batch:               */
#define TPR_BOUND_VLIM      1   /* [B][d][2]        JointVelocityConstraint                      */
#define TPR_BOUND_VLIM_GRID 2   /* [B][N+1][d][2]   JointVelocityConstraintVarying: vlim_func(s_i) */
#define TPR_BOUND_X         3   /* [B][N+1][2]      a constraint's xbound                        */
#define TPR_BOUND_U         4   /* [B][N+1][2]      a constraint's ubound                        */
#define TPR_BOUND_SHARED    1   /* flags: one array for the whole batch (no leading [B])         */
#define TPR_BOUND_MAX_SOURCES 8
typedef struct tpr_bound_source {
    int32_t kind, flags;
    const double *data;
} tpr_bound_source;
/* ABI guard, as tpr_second_order_block_bytes: bytes of tpr_bound_source in the library.                          */
int tpr_bound_source_bytes(void);

/* Replaces the box part of seidelWrapper.__init__ (cy_seidel_solverwrapper.pyx:477-478, 512-520) together with
 * JointVelocityConstraint.compute_constraint_params (linear_joint_velocity.py:43-53, _CythonUtils.pyx:16-59) and
 * JointVelocityConstraintVarying.compute_constraint_params (linear_joint_velocity.py:76-87, _CythonUtils.pyx:61-100) for B
 * trajectories: low, high [B][N+1][2] start at -+1e8 and take the sources IN LIST ORDER with the reference's
 * dbl_max(a, b) = a > b ? a : b / dbl_min(a, b) = a < b ? a : b (a: the running value); a VLIM* source first becomes an
 * xbound from qs = path(grid, 1) [B][N+1][d] with the reference's fp32 running bounds.  qs may be NULL without a VLIM*
 * source (d is ignored then).  flags: TPR_DEVICE_PTRS.  Refused before any launch: nsrc outside 0..TPR_BOUND_MAX_SOURCES,
 * an unknown kind, a NULL source array, a VLIM* source without qs (TPR_E_BADARG); B (N+1) > 2^31 - 1, or d > TPR_MAX_DOF with a
 * VLIM* source (TPR_E_UNSUPPORTED).
 * NaN bounds are the caller's error, as NaN samples are.                                                           */
int tpr_stage_boxes_batch(int B, int N, int d, const double *qs, int nsrc, const tpr_bound_source *src, int flags,
                          double *low, double *high, void *stream);

/* The passes of the sampled family with the boxes of tpr_stage_boxes_batch in place of the velocity limits: each takes the
 * arguments of its *_sampled_batch twin plus low, high [B][N+1][2], and replaces the same reference code as that twin --
 * compute_parameterization (reachability_algorithm.py:166-376, time_optimal_algorithm.py:55-92), TOPPRAsd
 * (desired_duration_algorithm.py:93-234), compute_controllable_sets (reachability_algorithm.py:166-238),
 * compute_feasible_sets (:131-164), compute_reachable_sets (:378-431) -- on a wrapper whose constraint list holds an
 * acceleration constraint and any number of first-order ones (JointVelocityConstraint, JointVelocityConstraintVarying,
 * bound-only LinearConstraints).  A stage reads its box (four doubles) and generates the acceleration rows from qs / qss;
 * results are the bits of the dense pass on the rows tpr_sampled_rows_batch writes without a velocity constraint and
 * these boxes.  p->vlim must be NULL and TPR_HAS_VELOCITY clear -- the box carries every first-order constraint --
 * otherwise TPR_E_UNSUPPORTED.  Limits of the sampled family: nC = 2 + 4 d <= 122 under Interpolation, d <= 32 otherwise. */
int tpr_solve_sampled_boxed_batch(const tpr_sampled_problem *p, const double *low, const double *high, const tpr_result *r,
                                  void *stream);
int tpr_solve_desired_duration_sampled_boxed_batch(const tpr_sampled_problem *p, const double *low, const double *high,
                                                   const double *desired, double atol, const tpr_result *r, double *alpha,
                                                   void *stream);
int tpr_controllable_sets_sampled_boxed_batch(const tpr_sampled_problem *p, const double *low, const double *high,
                                              const double *sdmin, const double *sdmax, double *K, void *stream);
int tpr_feasible_sets_sampled_boxed_batch(const tpr_sampled_problem *p, const double *low, const double *high, double *X,
                                          void *stream);
int tpr_reachable_sets_sampled_boxed_batch(const tpr_sampled_problem *p, const double *low, const double *high,
                                           const double *sdmin, const double *sdmax, double *L, double *X, void *stream);

/* ---- a rigid-body chain evaluated on the GPU: inverse dynamics and tool velocity for a batch --------------------------
 * The reference's Python side leaves the robot to the caller (JointTorqueConstraint takes an inv_dyn callback,
 * joint_torque.py:10-116); its C++ twin evaluates a model itself (cpp/src/toppra/constraint/joint_torque/pinocchio.hpp:
 * recursive Newton-Euler behind JointTorque; constraint/cartesian_velocity_norm/pinocchio.hpp: forward kinematics behind
 * CartesianVelocityNorm, b = v' S v, g = limit).  These entries are that piece for ONE serial chain shared by the batch:
 * a fixed base, d = 1 .. TPR_MAX_DOF links, link i's parent is link i-1 (link 0's is the base = the world frame).
 *   joint_type [d] int32   TPR_JOINT_REVOLUTE / TPR_JOINT_PRISMATIC.  ALWAYS A HOST ARRAY, with or without TPR_DEVICE_PTRS:
 *                          it is the model's structure, read by the host (validation) and handed to the kernels by value;
 *                          a device pointer here is refused (TPR_E_BADARG).
 *   rot   [d][3][3]        row-major; columns = the joint frame's axes in parent coordinates
 *   trans [d][3]           the joint frame's origin in parent coordinates
 *   axis  [d][3]           unit vector in the joint frame: a revolute joint rotates by q_i about it (Rodrigues' formula), a
 *                          prismatic one translates by q_i * axis.  The link frame is the joint frame after that motion.
 *   mass [d], com [d][3] (link frame), inertia [d][6] = xx, yy, zz, xy, xz, yz about the centre of mass in link-frame axes
 *   gravity [3]            gravitational acceleration in the world frame, applied as a base acceleration of -gravity
 *   tool [3]               a point in the last link's frame
 * The numeric arrays follow TPR_DEVICE_PTRS of the call's flags; every lane reads them through uniform loads.  Not modelled:
 * rotor inertia, viscous damping, floating bases (branched trees: the tpr_tree_* entries below).  fp64, every operation rounded on its own; sine and cosine
 * are the device library's (1 - 2 ulp), so results agree with a host evaluation to rounding, not in bits.                */
#define TPR_JOINT_REVOLUTE 0
#define TPR_JOINT_PRISMATIC 1
typedef struct tpr_chain {
    int32_t d, flags; /* flags: reserved, 0 */
    const int32_t *joint_type;
    const double *axis, *rot, *trans;
    const double *mass, *com, *inertia;
    const double *gravity, *tool;
} tpr_chain;
/* ABI guard, as tpr_second_order_block_bytes: bytes of tpr_chain in the library.                                  */
int tpr_chain_bytes(void);

/* tau = RNEA(q, qd, qdd) at npoints points: q, qd, qdd, tau [npoints][d].  One thread per point; 1 .. 8 dof keep a point's
 * state in registers, 9 .. 32 dof in LDS.  flags: TPR_DEVICE_PTRS.  Refused before any launch: a NULL chain, array or
 * buffer, d outside 1 .. TPR_MAX_DOF, an unknown joint type, npoints < 0 (TPR_E_BADARG); npoints > 2^31 - 1
 * (TPR_E_UNSUPPORTED) -- the same for the two entries below, with B (N + 1) as the point count.                       */
int tpr_chain_inverse_dynamics_batch(const tpr_chain *chain, long long npoints, const double *q, const double *qd,
                                     const double *qdd, double *tau, int flags, void *stream);
/* The three evaluations of tpr_second_order_block in one pass over the point (linear_second_order.py:154-162):
 * w0 = tau(q, 0, 0), wa = tau(q, 0, qs), wb = tau(q, qs, qss); q, qs, qss, w0, wa, wb [B][N+1][d].  The recursions share the
 * sines, cosines and link rotations; each output equals tpr_chain_inverse_dynamics_batch on the same arguments (products
 * with an exact zero are dropped, no sum is reordered).                                                               */
int tpr_chain_torque_terms_batch(const tpr_chain *chain, int B, int N, const double *q, const double *qs, const double *qss,
                                 double *w0, double *wa, double *wb, int flags, void *stream);
/* The tool point's spatial velocity for qd = qs -- linear v and angular w, both world-aligned -- as vSv = [v; w]' S [v; w]
 * [B][N+1]; S [6][6] row-major, NULL = the linear speed only (v' v).  With limit [B] it also writes the bound
 * xbound [B][N+1][2] = (0, limit / vSv) on x = sd^2 (an IEEE division: vSv == 0 gives +inf, which tpr_stage_boxes_batch
 * folds against its 1e8 box); vSv or xbound may be NULL, not both; xbound needs limit.  The caller's responsibility, as NaN
 * limits are elsewhere: limit > 0 (limit == 0 at a standstill is 0 / 0 = NaN, and a NaN bound loses every comparison of
 * tpr_stage_boxes_batch's fold, i.e. silently drops out) and S symmetric positive semi-definite (an indefinite S can give
 * vSv < 0 and with it a negative upper bound: an empty box).  toppra_amd's host layer checks both.                       */
int tpr_chain_tool_velocity_batch(const tpr_chain *chain, int B, int N, const double *q, const double *qs, const double *S,
                                  const double *limit, double *vSv, double *xbound, int flags, void *stream);
/* The tool point's acceleration acc(q, qd, qdd) = [lin; ang], [npoints][6], world axes, from the forward recursion of
 * tpr_chain_inverse_dynamics_batch with the base at rest (W = the last link's axes in the world; w, wd, a its angular velocity,
 * angular acceleration and origin acceleration in its own frame):
 *   lin = W (a + wd x tool + w x (w x tool)),   ang = W wd.
 * Pure kinematics: gravity is NOT applied (nor masses read).  lin is the CLASSICAL acceleration of the point -- the second time
 * derivative of its world position, what the reference's example examples-old/cartesian_accel.py reads from
 * GetLinkAccelerations(...)[:3] -- not the spatial one (which lacks w x v).  q, qd, qdd [npoints][d]; one thread per point,
 * any dof, state in registers.  A zero result is +0.  Refusals as tpr_chain_inverse_dynamics_batch.                      */
int tpr_chain_tool_acceleration_batch(const tpr_chain *chain, long long npoints, const double *q, const double *qd,
                                      const double *qdd, double *acc, int flags, void *stream);
/* The evaluations a second-order constraint on that acceleration needs (tpr_second_order_block with p = 6), in one pass:
 * wa = acc(q, 0, qs), wb = acc(q, qs, qss), [B][N+1][6]; w0 = acc(q, 0, 0) is an exact zero and is not computed.  Each
 * output equals tpr_chain_tool_acceleration_batch on the same arguments in every bit (products with an exact zero are
 * dropped, no sum is reordered).  Refusals as tpr_chain_torque_terms_batch.                                            */
int tpr_chain_tool_acceleration_terms_batch(const tpr_chain *chain, int B, int N, const double *q, const double *qs,
                                            const double *qss, double *wa, double *wb, int flags, void *stream);

/* A carried object: a rigid body fixed to the chain's last link, and the frame in which the wrench on it is reported.
 *   mass >= 0; com [3] its centre of mass in the last link's frame; inertia [6] = xx, yy, zz, xy, xz, yz about com in
 *   link-frame axes (the chain's convention); rot [3][3] row-major, columns = the contact frame's axes in last-link
 *   coordinates; origin [3] the contact frame's origin in the last link's frame.
 * ALWAYS A HOST STRUCT, with or without TPR_DEVICE_PTRS: it travels to the kernels by value.                           */
typedef struct tpr_payload {
    double mass, com[3], inertia[6], rot[9], origin[3];
} tpr_payload;
/* ABI guard, as tpr_chain_bytes: bytes of tpr_payload in the library.                                                  */
int tpr_payload_bytes(void);
/* The wrench the last link transmits to the payload, wrench(q, qd, qdd) = [f; n], [npoints][6].  With (w, wd, a) the last
 * link's angular velocity, angular acceleration and origin acceleration in its own frame, from the forward recursion of
 * tpr_chain_inverse_dynamics_batch started at a = -gravity (gravity IS applied):
 *   Fl = m (a + wd x com + w x (w x com)),   Nl = I wd + w x (I w),
 *   f = rot' Fl,   n = rot' (Nl + (com - origin) x Fl):
 * the force the link exerts on the body and its moment about the contact frame's origin, both in contact-frame axes; at rest
 * f is the support of the body's weight.  The chain's own masses are not read.  q, qd, qdd [npoints][d]; one thread per
 * point, any dof, state in registers.  A zero result is +0 (so a massless, inertia-less payload gives +0 throughout).
 * Refusals as tpr_chain_tool_acceleration_batch, and: a NULL payload, a negative or non-finite mass, any non-finite payload
 * entry (TPR_E_BADARG).                                                                                                */
int tpr_chain_tool_wrench_batch(const tpr_chain *chain, const tpr_payload *payload, long long npoints, const double *q,
                                const double *qd, const double *qdd, double *wrench, int flags, void *stream);
/* The three evaluations a second-order constraint on that wrench needs (tpr_second_order_block with p = 6), in one pass
 * over the links: w0 = wrench(q, 0, 0) -- the static wrench, not zero under gravity --, wa = wrench(q, 0, qs),
 * wb = wrench(q, qs, qss), [B][N+1][6].  Each output equals tpr_chain_tool_wrench_batch on the same arguments in every bit
 * (products with an exact zero are dropped, no sum is reordered).  Refusals as tpr_chain_tool_acceleration_terms_batch plus
 * the payload's above.                                                                                                 */
int tpr_chain_tool_wrench_terms_batch(const tpr_chain *chain, const tpr_payload *payload, int B, int N, const double *q,
                                      const double *qs, const double *qss, double *w0, double *wa, double *wb, int flags,
                                      void *stream);

/* Control points: up to TPR_CHAIN_MAX_POINTS points fixed to ANY links of the chain -- an elbow, a camera bracket, a cable
 * carrier -- evaluated in one pass over the links.  Point p sits in the frame of link[p] (0 .. d-1) at offset[p]; several points
 * may share a link; every output lists the points in the struct's order.  ALWAYS A HOST STRUCT, with or without
 * TPR_DEVICE_PTRS: it travels to the kernels by value, and the recursion ends after the deepest link that carries a point.  */
#define TPR_CHAIN_MAX_POINTS 16
typedef struct tpr_chain_points {
    int32_t count;
    int32_t link[TPR_CHAIN_MAX_POINTS];
    double offset[TPR_CHAIN_MAX_POINTS][3];
} tpr_chain_points;
/* ABI guard, as tpr_chain_bytes: bytes of tpr_chain_points in the library.                                             */
int tpr_chain_points_bytes(void);
/* The squared speed of every point for qd = qs: speed2 [B][N+1][count] = |v_p|^2, v_p = W (v + w x offset_p) with (v, w, W)
 * of link[p] from the recursion of tpr_chain_tool_velocity_batch -- a point (k, r) gives, in every bit, what that entry gives
 * with S = NULL for the chain cut after link k with tool = r.  With limit [B][count] also the bound
 * xbound [B][N+1][2] = (0, min_p limit[b][p] / speed2_p) on x = sd^2: ONE bound for the whole set (IEEE divisions: a point that
 * stands still gives +inf and drops out of the minimum).  speed2 or xbound may be NULL, not both; xbound needs limit; limit > 0
 * is the caller's responsibility, as for the tool entry.  Refusals as tpr_chain_tool_velocity_batch, and: a NULL points struct,
 * count outside 1 .. TPR_CHAIN_MAX_POINTS, a link outside 0 .. d-1, a non-finite offset (TPR_E_BADARG).                  */
int tpr_chain_points_speed_batch(const tpr_chain *chain, const tpr_chain_points *points, int B, int N, const double *q,
                                 const double *qs, const double *limit, double *speed2, double *xbound, int flags, void *stream);
/* The linear acceleration of every point, acc [npoints][3 count] (point-major, world axes), from the recursion of
 * tpr_chain_tool_acceleration_batch (base at rest, no gravity):  lin_p = W (a + wd x offset_p + w x (w x offset_p)) with
 * (w, wd, a, W) of link[p] -- the bits of that entry's lin for the chain cut after link k with tool = r.  A point's angular
 * acceleration is its link's and is not part of the output.  A zero result is +0.  Refusals as
 * tpr_chain_tool_acceleration_batch plus the point set's above.                                                        */
int tpr_chain_points_acceleration_batch(const tpr_chain *chain, const tpr_chain_points *points, long long npoints,
                                        const double *q, const double *qd, const double *qdd, double *acc, int flags,
                                        void *stream);
/* The evaluations a second-order constraint on those accelerations needs (tpr_second_order_block with p = 3 count), in one
 * pass: wa = acc(q, 0, qs), wb = acc(q, qs, qss), [B][N+1][3 count]; w0 = acc(q, 0, 0) is an exact zero and is not computed.
 * Each output equals tpr_chain_points_acceleration_batch on the same arguments in every bit.  Refusals as
 * tpr_chain_tool_acceleration_terms_batch plus the point set's above.                                                   */
int tpr_chain_points_acceleration_terms_batch(const tpr_chain *chain, const tpr_chain_points *points, int B, int N,
                                              const double *q, const double *qs, const double *qss, double *wa, double *wb,
                                              int flags, void *stream);

/* ---- a kinematic TREE evaluated on the GPU: inverse dynamics of a branched robot for a batch -------------------------------
 * Two arms on a torso, an arm beside a pan-tilt head, an arm with an articulated gripper, several robots on one base: the
 * torque at a joint below a branching link depends on every joint beyond it in every branch.  The model is tpr_chain's -- `links`
 * gives d = 1 .. TPR_MAX_DOF links with the chain's arrays and conventions; links->tool is NOT read (a tree has no single tip)
 * and may be NULL -- with a parent table beside it:
 *   parent [d] int32   parent[i] is the link that joint i attaches link i to, -1 = the fixed base; the numbering is topological,
 *                      -1 <= parent[i] < i.  Several links may have parent -1 (a forest).  rot[i], trans[i] place joint i in the
 *                      frame of parent[i].  ALWAYS A HOST ARRAY of links->d entries, with or without TPR_DEVICE_PTRS, as
 *                      joint_type is: the structure is read by the host and travels to the kernels by value.
 * A FORK is a link j that is the parent of some link i != j + 1 (the base is never one); it keeps one bank of LDS for what its
 * later children need, and a tree may have at most TPR_TREE_MAX_FORKS of them.  parent = -1, 0, 1, ... is the serial chain.
 * Runtime dof at every dof: one wave of 64 points per block, a point's state in LDS, d * 8 * 512 + forks * 9 * 512 bytes (fused
 * d * 17 * 512 + forks * 18 * 512 while that fits 160 KB, i.e. up to 17 dof with one fork; otherwise the three evaluations run
 * one after another in the same launch).  The children's wrenches are summed at a fork in a fixed order: the children
 * i != j + 1 in descending link number, then child j + 1 plus that sum.  Two bit properties follow from it:
 *   - a chain-shaped tree gives the bits of tpr_chain_inverse_dynamics_batch / tpr_chain_torque_terms_batch at every dof;
 *   - each output of tpr_tree_torque_terms_batch equals tpr_tree_inverse_dynamics_batch on the same arguments in every bit
 *     (products with an exact zero are dropped, no sum is reordered).                                                      */
#define TPR_TREE_MAX_FORKS 4
/* tau = RNEA(q, qd, qdd) of the tree at npoints points: q, qd, qdd, tau [npoints][d].  flags: TPR_DEVICE_PTRS.  Refused before
 * any launch: everything tpr_chain_inverse_dynamics_batch refuses (links->tool apart), a NULL parent, a device pointer as
 * parent, an entry outside -1 .. i-1 (TPR_E_BADARG); more than TPR_TREE_MAX_FORKS forks (TPR_E_UNSUPPORTED).             */
int tpr_tree_inverse_dynamics_batch(const tpr_chain *links, const int32_t *parent, long long npoints, const double *q,
                                    const double *qd, const double *qdd, double *tau, int flags, void *stream);
/* The three evaluations of tpr_second_order_block in one launch, as tpr_chain_torque_terms_batch: w0 = tau(q, 0, 0),
 * wa = tau(q, 0, qs), wb = tau(q, qs, qss); q, qs, qss, w0, wa, wb [B][N+1][d].  Refusals as above, with B (N + 1) as the point
 * count.                                                                                                                  */
int tpr_tree_torque_terms_batch(const tpr_chain *links, const int32_t *parent, int B, int N, const double *q, const double *qs,
                                const double *qss, double *w0, double *wa, double *wb, int flags, void *stream);

/* ---- the base reaction: the wrench a robot's mount exerts ON the robot, for a batch -----------------------------------------
 * What a pedestal's flange, a linear axis, a ceiling plate or the footprint of a cart has to supply: the sum over EVERY link of
 * every root of a tree (a serial chain is the tree parent = -1, 0, 1, ...), gravity included -- at rest the force holds up the
 * weight.  The moment is taken about the origin of a mount frame and both parts are expressed in that frame's axes:
 *   rot [3][3] row-major, columns = the mount frame's axes in base coordinates (orthonormal, determinant +1, to 1e-12);
 *   origin [3] its origin in base coordinates; mass >= 0, com [3]: a rigid platform fixed to the base (the cart or column whose
 *   weight keeps a mobile manipulator upright), its centre of mass in base coordinates; it adds -mass gravity at com.
 * ALWAYS A HOST STRUCT, with or without TPR_DEVICE_PTRS: it travels to the kernels by value.  A NULL mount is the base frame
 * itself without a platform.                                                                                              */
typedef struct tpr_mount {
    double rot[9], origin[3], mass, com[3];
} tpr_mount;
/* ABI guard, as tpr_chain_bytes: bytes of tpr_mount in the library.                                                     */
int tpr_mount_bytes(void);
/* wrench(q, qd, qdd) = [f'; n'], [npoints][6].  With W_i the link frame's rotation and p_i its origin in base coordinates, m_i and
 * c_i the link's mass and centre of mass, and F_i, N_i the net force on link i and its net moment about c_i from the forward
 * recursion of tpr_tree_inverse_dynamics_batch started from a base AT REST (gravity is not in it):
 *   f = sum_i -m_i gravity - mass gravity + sum_i W_i F_i,
 *   n = sum_i (p_i + W_i c_i) x (-m_i gravity) + com x (-mass gravity) + sum_i [W_i (N_i + c_i x F_i) + p_i x (W_i F_i)],
 *   f' = rot' f,   n' = rot' (n - origin x f):
 * the weight is summed in base coordinates, where no rotation touches it, and only the rest goes through the recursion.
 * Forward only, a point's state in registers at any dof; the links are summed in ascending number.  One wave of 64 points per
 * block; dynamic LDS stages a block's inputs and outputs and keeps one bank of 21 doubles per lane and fork (27 in the terms
 * entry): at most 50 688 + 4 * 27 * 512 = 105 984 bytes.  A zero result is +0.  links, parent and their refusals are those of
 * tpr_tree_inverse_dynamics_batch; then: a non-finite entry of the mount, a rot that is not orthonormal with determinant +1 to
 * 1e-12, a negative mass (TPR_E_BADARG); then NULL arrays.                                                                */
int tpr_tree_base_wrench_batch(const tpr_chain *links, const int32_t *parent, const tpr_mount *mount, long long npoints,
                               const double *q, const double *qd, const double *qdd, double *wrench, int flags, void *stream);
/* The three evaluations a second-order constraint on that wrench needs (tpr_second_order_block with p = 6), in one pass over
 * the links: w0 = wrench(q, 0, 0) -- the static reaction, not zero under gravity --, wa = wrench(q, 0, qs),
 * wb = wrench(q, qs, qss), [B][N+1][6].  Each output equals tpr_tree_base_wrench_batch on the same arguments in every bit
 * (products with an exact zero are dropped, no sum is reordered).  Refusals as tpr_tree_torque_terms_batch plus the mount's
 * above.                                                                                                                  */
int tpr_tree_base_wrench_terms_batch(const tpr_chain *links, const int32_t *parent, const tpr_mount *mount, int B, int N,
                                     const double *q, const double *qs, const double *qss, double *w0, double *wa, double *wb,
                                     int flags, void *stream);

/* ---- joint loads: the wrench ACROSS any joint of a chain or tree, for a batch -------------------------------------------------
 * What a gearbox's output bearing, a linear guide's carriage or a link's flange carries beside the joint's own torque: the tilting
 * moment and the axial and radial force.  (f_i, n_i) of the recursion of tpr_tree_inverse_dynamics_batch is the force the parent
 * side exerts ON link i through joint i and its moment about link i's origin, in link i's axes, gravity included (at rest f is the
 * support of the weight of everything that hangs on the joint; for a fork, every child branch).  A SECTION k reports it in a frame
 * fixed to link link[k]:
 *   rot[k] [3][3] row-major, columns = the section frame's axes in link coordinates (orthonormal, determinant +1, to 1e-12);
 *   origin[k] [3] its origin in link coordinates;
 *   w_k = [ rot' f ; rot' (n - origin x f) ]   -- with rot = 1, origin = 0: axis . n (revolute) or axis . f (prismatic) is the
 *   joint's torque or force.
 * A set holds 1 .. TPR_JOINT_MAX_SECTIONS sections, several may share a joint, and each section's output is independent of what
 * else is in the set.  ALWAYS A HOST STRUCT, with or without TPR_DEVICE_PTRS: it travels to the kernels by value.            */
#define TPR_JOINT_MAX_SECTIONS 8
typedef struct tpr_joint_sections {
    int32_t count;
    int32_t link[TPR_JOINT_MAX_SECTIONS];
    double rot[TPR_JOINT_MAX_SECTIONS][9];
    double origin[TPR_JOINT_MAX_SECTIONS][3];
} tpr_joint_sections;
/* ABI guard, as tpr_mount_bytes: bytes of tpr_joint_sections in the library.                                             */
int tpr_joint_sections_bytes(void);
/* wrench(q, qd, qdd), [npoints][count][6] in the set's order.  The plain link-local recursion on the tree kernels' walk (their
 * summation order at a fork), with (f, n) kept; the way down stops at the lowest-numbered section link.  One wave of 64 points per
 * block, the tree kernels' dynamic LDS (per-link state plus one bank per fork: at most 149 504 bytes), outputs by direct stores.
 * A zero result is +0.  links, parent and their refusals are those of tpr_tree_inverse_dynamics_batch; then the sections: NULL,
 * a count outside 1 .. 8, a link outside 0 .. d-1, a non-finite entry, a rot that is not orthonormal with determinant +1 to 1e-12
 * (TPR_E_BADARG); then NULL arrays.                                                                                       */
int tpr_tree_joint_wrench_batch(const tpr_chain *links, const int32_t *parent, const tpr_joint_sections *sections, long long npoints,
                                const double *q, const double *qd, const double *qdd, double *wrench, int flags, void *stream);
/* The three evaluations a second-order constraint on those wrenches needs (tpr_second_order_block with p = 6 count), in one
 * launch: w0 = wrench(q, 0, 0) -- the static load, not zero under gravity --, wa = wrench(q, 0, qs), wb = wrench(q, qs, qss),
 * [B][N+1][count][6].  One pass over the links where the fused per-link state fits the LDS (a chain to 18 dof, one fork to 17),
 * otherwise the three evaluations one after another in the same launch.  Each output equals tpr_tree_joint_wrench_batch on the
 * same arguments in every bit.  Refusals: B, N first, then as above.                                                       */
int tpr_tree_joint_wrench_terms_batch(const tpr_chain *links, const int32_t *parent, const tpr_joint_sections *sections, int B, int N,
                                      const double *q, const double *qs, const double *qss, double *w0, double *wa, double *wb,
                                      int flags, void *stream);

/* ---- momentum and kinetic energy: how much motion a set of a robot's links carries, for a batch --------------------------------
 * What a collaborative robot's safety controller caps beside force and speed: the momentum of the moving structure (kg m / s) and
 * the kinetic energy it can transfer on contact.  Both are first order in the path velocity: with qd = q' sd the momentum is
 * h(q, q') sd and the energy 1/2 q'' M(q) q' sd^2, so each limit is an upper bound on x = sd^2 per gridpoint.  Per unit of path
 * velocity (qd = qs), with W_i the link frame's rotation and p_i its origin in base coordinates, v_i and w_i the velocity of that
 * origin and the angular velocity in link axes (the recursion of tpr_chain_tool_velocity_batch), m_i, c_i, I_i the link's mass,
 * centre of mass and inertia about it, and vc_i = v_i + w_i x c_i:
 *   h_i = (W_i vc_i) m_i
 *   P   = sum_i h_i                                           linear momentum, base axes
 *   L   = sum_i [ W_i (I_i w_i) + (p_i + W_i c_i) x h_i ]     angular momentum about the base origin, base axes
 *   T2  = sum_i [ m_i (vc_i . vc_i) + w_i . (I_i w_i) ]       = qs' M(q) qs: twice the kinetic energy per sd^2
 *   P'  = rot' P,   L' = rot' (L - origin x P)                in the mount frame (the mount's mass and com do not move: not read)
 * The sums run over the links of link_mask (bit i = link i) in ascending number, the sum on the left, (((0 + t_0) + t_1) + ...),
 * then the mount frame; every output passes through "+ 0.0": a standstill gives +0.  Links outside the set are skipped, not
 * multiplied by zero, and the walk ends after the highest link of the set; the result equals, in every bit, the full sum on the
 * robot whose other links have mass 0 and inertia 0.
 *   momentum [B][N+1][6] = [P'; L'];   energy2 [B][N+1] = T2;
 *   xbound [B][N+1][2] = (0, min(limit[b][0] / |P'|^2, limit[b][1] / |L'|^2, limit[b][2] / T2)),  |a|^2 = (a_x a_x + a_y a_y) + a_z a_z,
 *   limit [B][3] = (p_max^2, L_max^2, 2 E_max), each > 0 (the caller's responsibility, as for tpr_chain_tool_velocity_batch);
 *   +inf switches a term off.  The divisions are IEEE on the outputs as they leave: a standstill gives +inf -- the array a
 *   TPR_BOUND_X source of tpr_stage_boxes_batch takes, where the box then keeps its 1e8.
 * Any of momentum, energy2, xbound may be NULL, not all; each output is the same whichever others are asked for.  Forward only, a
 * point's state in registers at any dof.  One wave of 64 points per block; dynamic LDS stages a block's q, qs rows and its outputs
 * (one row of 9 doubles per point) and keeps one bank of 18 doubles per lane and fork: at most 33 792 + 4 * 18 * 512 = 70 656 bytes.
 * Refused before any launch, in this order: B, N; what tpr_tree_base_wrench_batch refuses of links, parent and the mount; an empty
 * link_mask, a bit at or above d (TPR_E_BADARG); a NULL q or qs; all three outputs NULL; xbound without limit.
 * T2 bounds what a contact can take up at ANY point and direction at once; the energy at given control points, through the
 * robot's effective (reflected) mass there, is the entry of toppra_hip_contact.h.                                              */
int tpr_tree_momentum_batch(const tpr_chain *links, const int32_t *parent, const tpr_mount *mount, uint32_t link_mask, int B, int N,
                            const double *q, const double *qs, const double *limit, double *momentum, double *energy2,
                            double *xbound, int flags, void *stream);

/* Replaces seidelWrapper.solve_stagewise_optim (cy_seidel_solverwrapper.pyx:549-697) for ONE
 * stage of each of B trajectories (the compatibility entry; 1 LP per call per trajectory).
 *   stage [B]; g [B][2]; xb [B][4] = x_min, x_max, x_next_min, x_next_max (NaN = absent);
 *   active [B][4] = active_c_up[2], active_c_down[2] warm-start state, updated in place;
 *   solve_lp1d: the constructor flag (:425); out [B][2] = [u, x] or NaNs.                        */
int tpr_solve_stagewise_batch(const tpr_problem *p, const int32_t *stage, const double *g,
                              const double *xb, int32_t *active, int solve_lp1d, double *out,
                              void *stream);

/* Replaces solve_lp1d / solve_lp2d (cy_seidel_solverwrapper.pyx:42-87 -> :93-144, :149-390) for n
 * independent LPs of nrows rows each (the known-answer-test entry).
 *   lp1d: v [n][2], a,b [n][nrows], low,high [n]
 *         -> result [n], optval [n], optvar [n], active [n]
 *   lp2d: v [n][3], a,b,c [n][nrows], low,high [n][2], active_in [n][2]
 *         -> result [n], optval [n], optvar [n][2], active_out [n][2]                            */
int tpr_lp1d_batch(int n, int nrows, const double *v, const double *a, const double *b,
                   const double *low, const double *high, int32_t *result, double *optval,
                   double *optvar, int32_t *active, void *stream);
int tpr_lp2d_batch(int n, int nrows, const double *v, const double *a, const double *b,
                   const double *c, const double *low, const double *high, const int32_t *active_in,
                   int32_t *result, double *optval, double *optvar, int32_t *active_out,
                   void *stream);

/* Replaces SplineInterpolator.__init__ -> scipy.interpolate.CubicSpline (interpolator.py:360-421)
 * for B paths: waypoints [B][m][d] at knots [m] (knots_per_path == 0) or [B][m] -> coef
 * [B][4][m-1][d], the layout tpr_problem.coef takes.  Boundary conditions per end:
 * TPR_BC_NOT_A_KNOT, TPR_BC_FIRST_DERIV (value [B][d], NULL = 0: scipy's "clamped"),
 * TPR_BC_SECOND_DERIV (NULL = 0: "natural").  m >= 2 (splines of more than 64 points keep their
 * working arrays in a stream-ordered global workspace of 6 m doubles per spline).  device_ptrs != 0: all
 * pointers are device pointers.                                                                    */
#define TPR_BC_NOT_A_KNOT 0
#define TPR_BC_FIRST_DERIV 1
#define TPR_BC_SECOND_DERIV 2
int tpr_spline_fit_batch(int B, int m, int d, const double *knots, int knots_per_path,
                         const double *waypoints, int bc_start, int bc_end, const double *bc_start_val,
                         const double *bc_end_val, double *coef, int device_ptrs, void *stream);

/* Replaces ParametrizeConstAccel (toppra/parametrizer.py:23-158) for B trajectories of one shape.
 * times:  _process_parametrization -- sd [B][N+1] -> ts [B][N+1] (running sum in the reference's
 *         order), us [B][N] (may be NULL).  Only N, B, flags (TPR_GRID_PER_TRAJ, TPR_DEVICE_PTRS) and
 *         grid of `p` are used.
 * eval:   __call__(t, order) -- times [B][T] -> out [B][T][d] = q(t) (order 0), dq/dt (1), d2q/dt2 (2),
 *         using p->coef/breaks/grid and the sd, ts, us arrays of the same trajectories.            */
int tpr_const_accel_times_batch(const tpr_problem *p, const double *sd, double *ts, double *us, void *stream);
int tpr_const_accel_eval_batch(const tpr_problem *p, const double *sd, const double *ts, const double *us,
                               int T, const double *times, int order, double *out, void *stream);

/* Replaces ParametrizeSpline (toppra/parametrizer.py:161-196), the reference's default output
 * parametrizer (algorithm/algorithm.py:121-125), for B trajectories: the gridpoint time stamps (a running
 * sum; a gridpoint reached in less than TINY = 1e-8 s is dropped, a standing stretch counts 5 s), the
 * waypoints q(s_i) and the cubic spline in time through them, clamped to q'(s) sd at both ends (scipy
 * CubicSpline arithmetic as in tpr_spline_fit_batch).  sd [B][N+1] -> knot_times [B][N+1] (compacted;
 * entries from counts[b] on are padding), counts [B] (gridpoints kept), coef_t [B][4][N][d] (segments from
 * counts[b]-1 on are a constant extension).  Uses p->coef/breaks/grid/flags and p->variant: 0 = auto, 1 = generic (two
 * kernels, any d), 2 = one fused kernel in LAPACK dgtsv's elimination order (d <= 64; the bits of scipy on an FMA-free
 * LAPACK), 3 = knot-parallel (d <= 16, all knots in LDS; cyclic reduction instead of dgtsv: the knot derivatives agree to
 * rounding, q(t) within 1e-10 of the reference's samples like variant 2; twice as fast).  Auto picks 3 where it fits,
 * else 2, else 1.  Time stamps, counts and waypoints are the same bits in every variant.
 * tpr_ppoly_eval_batch evaluates such tables -- SplineInterpolator.__call__(t, order), i.e. scipy PPoly
 * (interpolator.py:423-430) -- at times [B][T] -> out [B][T][d]; breaks [B][nseg+1]; counts may be NULL.   */
/* ParametrizeSpline + SplineInterpolator.__call__ in one launch: what a caller of compute_trajectory() does next
 * (traj(ts), traj(ts, 1), traj(ts, 2): examples/plot_kinematics.py:52-57) without the [B][4][N][d] coefficient table in
 * between -- the knot-parallel fit (variant 3 of tpr_param_spline_batch: d <= 16, knots in LDS) evaluates the samples from
 * its LDS-resident knot derivatives; the same bits as tpr_param_spline_batch(variant 3) + tpr_ppoly_eval_batch.
 * times [B][T] (times_per_traj) or [T]; fractions != 0: times are fractions of each trajectory's duration
 * (linspace(0, 1, T) * duration).  q / qd / qdd [B][T][d] (order 0 / 1 / 2; any may be NULL), duration [B] (may be NULL). */
int tpr_param_spline_sample_batch(const tpr_problem *p, const double *sd, int T, const double *times, int times_per_traj,
                                  int fractions, double *q, double *qd, double *qdd, double *duration, void *stream);
int tpr_param_spline_batch(const tpr_problem *p, const double *sd, double *knot_times, int32_t *counts,
                           double *coef_t, void *stream);
int tpr_ppoly_eval_batch(int B, int nseg, int d, const double *coef, const double *breaks, const int32_t *counts,
                         int T, const double *times, int order, double *out, int device_ptrs, void *stream);

/* Measurement helper used by bench.py: launches the tpr_solve_batch kernel(s) `reps` times on
 * `stream` between two hipEvents recorded on that same stream and returns the average
 * milliseconds per launch (device pointers required).                                            */
int tpr_solve_batch_timed(const tpr_problem *p, const tpr_result *r, void *stream, int reps,
                          float *ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* TOPPRA_HIP_H */

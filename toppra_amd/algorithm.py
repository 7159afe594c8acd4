"""TOPP-RA algorithm layer: the reference's ``toppra.algorithm.TOPPRA`` surface, running on the
MI355X one *pass* at a time, plus ``BatchTOPPRA`` for B trajectories per launch.

Reference: algorithm/algorithm.py:27-215 (ParameterizationData / ReturnCode / base class),
reachabilitybased/reachability_algorithm.py:14-431, time_optimal_algorithm.py:8-92.
Same constructor arguments, same return shapes, same exceptions for bad input, same
"failure is data" convention (NaN / None results + ``problem_data.return_code``).
"""
import enum
import logging
import time

import numpy as np

from . import _capi
from . import batch as _batch
from . import exceptions
from . import interpolator as _interp
from .constants import SMALL
from .solverwrapper import hipDenseSeidelWrapper, hipRobustWrapper, hipSampledSeidelWrapper, hipSeidelWrapper

logger = logging.getLogger(__name__)


class ParameterizationReturnCode(enum.Enum):
    """Return codes of a parameterization attempt (algorithm.py:49-62)."""

    Ok = "Ok: Successful parametrization"
    ErrUnknown = "Error: Unknown issue"
    ErrShortPath = "Error: Input path is very short"
    FailUncontrollable = "Error: Instance is not controllable"
    ErrForwardPassFail = "Error: Forward pass fail. Numerical errors occured"

    def __str__(self):
        return super(ParameterizationReturnCode, self).__repr__()


_STATUS_TO_CODE = {0: ParameterizationReturnCode.Ok, 1: ParameterizationReturnCode.FailUncontrollable,
                   2: ParameterizationReturnCode.ErrUnknown}


class ParameterizationData(object):
    """Internal data and output (algorithm.py:27-46)."""

    def __init__(self):
        self.return_code = ParameterizationReturnCode.ErrUnknown
        self.gridpoints = None
        self.sd_vec = None
        self.sdd_vec = None
        self.K = None
        self.X = None

    def __repr__(self):
        return "ParameterizationData(return_code:={}, N={:d})".format(
            self.return_code, self.gridpoints.shape[0])


class ParameterizationAlgorithm(object):
    """Base class: gridpoint selection and validation (algorithm.py:65-125)."""

    def __init__(self, constraint_list, path, gridpoints=None, parametrizer=None,
                 gridpt_max_err_threshold=1e-3, gridpt_min_nb_points=100):
        self.constraints = constraint_list
        self.path = path
        self._problem_data = ParameterizationData()
        if gridpoints is None:
            gridpoints = _interp.propose_gridpoints(path, max_err_threshold=gridpt_max_err_threshold,
                                                    min_nb_points=gridpt_min_nb_points)
            logger.info("No gridpoint specified. Automatically choose a gridpoint with %d points",
                        len(gridpoints))
        if path.path_interval[0] != gridpoints[0] or path.path_interval[1] != gridpoints[-1]:
            raise ValueError("Invalid manually supplied gridpoints.")
        self.gridpoints = np.array(gridpoints)
        self._problem_data.gridpoints = np.array(gridpoints)
        self._N = len(gridpoints) - 1
        if np.any(np.diff(self.gridpoints) <= 0):
            logger.fatal("Input gridpoints are not monotonically increasing.")
            raise ValueError("Bad input gridpoints.")
        from . import parametrizer as tparam
        if parametrizer is None or parametrizer == "ParametrizeSpline":
            self.parametrizer = tparam.ParametrizeSpline
        elif parametrizer == "ParametrizeConstAccel":
            self.parametrizer = tparam.ParametrizeConstAccel
        else:
            self.parametrizer = parametrizer

    @property
    def problem_data(self):
        return self._problem_data

    def compute_parameterization(self, sd_start, sd_end, return_data=False):
        raise NotImplementedError

    def compute_trajectory(self, sd_start=0, sd_end=0):
        """Time-parameterized joint trajectory, or None when the path cannot be parameterized
        (algorithm.py:163-194)."""
        t0 = time.time()
        self.compute_parameterization(sd_start, sd_end)
        if self.problem_data.return_code != ParameterizationReturnCode.Ok:
            logger.warning("Fail to parametrize path. Return code: %s", self.problem_data.return_code)
            return None
        traj = self.parametrizer(self.path, self.problem_data.gridpoints, self.problem_data.sd_vec)
        logger.info("Finish parametrization in %.3f secs", time.time() - t0)
        return traj


class ReachabilityAlgorithm(ParameterizationAlgorithm):
    """Reachability-analysis algorithms over a solver wrapper
    (reachability_algorithm.py:14-431).  ``solver_wrapper`` may be None, "hip" or "seidel" -- all
    select the HIP seidel wrapper, the only solver of this build."""

    _SOLVERS = ("hip", "seidel")

    def __init__(self, constraint_list, path, gridpoints=None, solver_wrapper=None, parametrizer=None,
                 **kwargs):
        super(ReachabilityAlgorithm, self).__init__(constraint_list, path, gridpoints=gridpoints,
                                                    parametrizer=parametrizer, **kwargs)
        has_conic = any(getattr(c.get_constraint_type(), "value", None) == 1 for c in constraint_list)
        if solver_wrapper is None:
            solver_wrapper = "hip"
        if has_conic:
            # the reference needs ecos / cvxpy here (reachability_algorithm.py:78-84); this build
            # solves the same stage problems exactly on the GPU -- parity unpinned against ECOS, cross-checked at
            # 1e-7 against an independent exact solver
            assert solver_wrapper.lower() in ("hip", "ecos"), \
                "Problem has conic constraints, solver {:} is not suitable".format(solver_wrapper)
            self.solver_wrapper = hipRobustWrapper(self.constraints, self.path, self.gridpoints)
        else:
            assert solver_wrapper.lower() in self._SOLVERS, "Solver {:} not found".format(solver_wrapper)
            try:  # velocity + acceleration limits: rows regenerated on the GPU from the spline table (the fused kernels)
                self.solver_wrapper = hipSeidelWrapper(self.constraints, self.path, self.gridpoints,
                                                       solve_lp1d=True)
            except NotImplementedError:
                try:  # velocity + acceleration limits on a path without a cubic-spline table: the fused passes on its samples
                    self.solver_wrapper = hipSampledSeidelWrapper(self.constraints, self.path, self.gridpoints,
                                                                  solve_lp1d=True)
                except NotImplementedError:
                    # any other canonical-linear list (second-order / torque constraints, the reference's own or hand-written
                    # constraint objects): parameters from the constraints' callbacks, the scans on the dense-row entries
                    self.solver_wrapper = hipDenseSeidelWrapper(self.constraints, self.path, self.gridpoints,
                                                                solve_lp1d=True)

    def compute_feasible_sets(self):
        """X[N+1, 2]: feasible squared velocities per gridpoint (NaN where infeasible)."""
        X = np.array(self.solver_wrapper.feasible_sets())
        self._problem_data.X = X
        return X

    def compute_reachable_sets(self, sdmin, sdmax):
        """L[N+1, 2]: squared velocities reachable from [sdmin^2, sdmax^2] at the start
        (reachability_algorithm.py:409-431; computes and stores the feasible sets on the way, like the
        reference).  A NaN row marks the stage that failed; the rows after it stay zero."""
        assert sdmin <= sdmax and 0 <= sdmin
        L, X = self.solver_wrapper.reachable_sets(sdmin, sdmax)
        self._problem_data.X = np.array(X)
        L = np.array(L)
        if np.isnan(L).any():
            i = int(np.argmax(np.isnan(L).any(axis=1)))
            logger.warning("L[{:d}]={:}. Path not parametrizable.".format(i, L[i]))
        return L

    def compute_controllable_sets(self, sdmin, sdmax):
        """K[N+1, 2]: controllable squared velocities; a NaN row marks the stage that failed and
        the rows above it stay zero, as in the reference."""
        assert sdmin <= sdmax and 0 <= sdmin
        K = np.array(self.solver_wrapper.controllable_sets(sdmin, sdmax))
        if np.isnan(K).any():
            i = int(np.argmax(np.isnan(K).any(axis=1)))
            logger.warning("A numerical error occurs: The controllable set at step "
                           "[{:d} / {:d}] can't be computed.".format(i, self._N + 1))
        return K

    def compute_parameterization(self, sd_start, sd_end, return_data=False):
        """Returns (sdd_vec[N], sd_vec[N+1], v_vec[N,0]) (+ K with return_data); Nones when the
        instance is not controllable (reachability_algorithm.py:240-376)."""
        if sd_end < 0 or sd_start < 0:
            raise exceptions.BadInputVelocities(
                "Negative path velocities: path velocities must be positive: (%s, %s)" % (sd_start, sd_end))
        out = self.solver_wrapper.parameterization(sd_start, sd_end)
        K = np.array(out["K"])
        status = int(out["status"])
        self._problem_data.return_code = _STATUS_TO_CODE[status]
        if status == 1:
            if not np.isnan(K).any():
                self._problem_data.K = K
                logger.warning("The initial velocity is not controllable. {:f} not in ({:f}, {:f})".format(
                    sd_start ** 2, K[0, 0], K[0, 1]))
            else:
                logger.warning("An error occurred when computing controllable velocities. "
                               "The path is not controllable, or is badly conditioned.")
            return (None, None, None, K) if return_data else (None, None, None)
        self._problem_data.K = K
        sd_vec = np.array(out["sd"])
        sdd_vec = np.array(out["u"])
        v_vec = np.zeros((self._N, 0))
        self._problem_data.sd_vec = sd_vec
        self._problem_data.sdd_vec = sdd_vec
        if return_data:
            return sdd_vec, sd_vec, v_vec, K
        return sdd_vec, sd_vec, v_vec


class TOPPRA(ReachabilityAlgorithm):
    """Time-optimal path parameterization by reachability analysis
    (time_optimal_algorithm.py:8-92).

    >>> inst = TOPPRA([pc_vel, pc_acc], path, gridpoints=ss)
    >>> sdd, sd, _ = inst.compute_parameterization(0, 0)
    """


class TOPPRAsd(ReachabilityAlgorithm):
    """TOPP-RA with a specified duration (desired_duration_algorithm.py:21-234): the fastest and the
    slowest parameterizations are computed and a convex combination with the desired duration is
    found by bisection.  Unachievable durations return the fastest / slowest one, as the reference."""

    def set_desired_duration(self, desired_duration):
        self.desired_duration = desired_duration

    def compute_parameterization(self, sd_start, sd_end, return_data=False, atol=1e-5):
        assert sd_end >= 0 and sd_start >= 0, "Path velocities must be positive"
        out = self.solver_wrapper.parameterization_sd(sd_start, sd_end, self.desired_duration, atol)
        K = np.array(out["K"])
        status = int(out["status"])
        self._problem_data.return_code = _STATUS_TO_CODE[status]
        if status == 1:
            if not np.isnan(K).any():
                self._problem_data.K = K
            return (None, None, None, K) if return_data else (None, None, None)
        self._problem_data.K = K
        sd_vec, sdd_vec = np.array(out["sd"]), np.array(out["u"])
        v_vec = np.zeros((self._N, 0))
        self._problem_data.sd_vec = sd_vec
        self._problem_data.sdd_vec = sdd_vec
        return (sdd_vec, sd_vec, v_vec, K) if return_data else (sdd_vec, sd_vec, v_vec)


class BatchTOPPRA(object):
    """B independent TOPP-RA problems of one shape solved in one launch.

    Parameters
    ----------
    coef, breaks : arrays [B, 4, nseg, d] and [nseg+1] (or [B, nseg+1]) -- cubic spline tables
        (``batch.spline_coefficients`` builds them from waypoints), numpy or torch-ROCm tensors.
    gridpoints : [N+1] shared or [B, N+1] per trajectory.
    vlim, alim : [B, d, 2] joint velocity / acceleration limits (either may be None).
    constraints : further constraints, in list order after vlim and alim: ``BatchJointTorqueConstraint`` /
        ``BatchSecondOrderConstraint`` objects with a batched inverse-dynamics callback, or
        ``BatchCartesianAccelerationConstraint`` / ``BatchToolWrenchConstraint`` / ``BatchPointAccelerationConstraint`` (limits on
        a chain's tool acceleration, on the wrench it transmits to a carried object, on the accelerations of control points on
        any links).  Their rows are built on the GPU
        once per object and every pass runs on the dense-row entries; without them nothing changes.
        ``BatchJointVelocityConstraintVarying`` / ``BatchBoundConstraint`` / ``BatchCartesianVelocityNormConstraint`` /
        ``BatchPointSpeedConstraint`` objects
        (first-order: they only tighten the box
        of a stage's variables) may stand anywhere among them: their bounds and vlim are folded into stage boxes on the GPU
        once per object, in list order, and the passes run on the boxed sampled entries (or, with second-order constraints
        in the list too, on the dense-row entries with these boxes).
    """

    def __init__(self, coef, breaks, gridpoints, vlim, alim, interpolation=True, constraints=None):
        self.coef, self.breaks, self.gridpoints = coef, breaks, gridpoints
        self.vlim, self.alim, self.interpolation = vlim, alim, interpolation
        self._set_constraints(constraints)
        self._rows = self._rows_dev = None
        self._pe = self._boxed = self._boxed_dev = None
        self._samples = None  # (q, qs, qss) of from_path_samples: the path as samples at the gridpoints, no spline table
        if self.constraints:
            self._check_constraints()
        if self.first_order and coef is not None:
            self._check_first_order()

    @classmethod
    def from_path_samples(cls, gridpoints, q, qs, qss, vlim, alim, interpolation=True, constraints=None):
        """The batch for ANY geometric paths, given as samples at the gridpoints: ``q = path(grid)`` (may be None where no
        trajectory and no second-order constraint is asked for), ``qs = path(grid, 1)``, ``qss = path(grid, 2)``, each
        [B, N+1, d], numpy or torch-ROCm tensors; ``gridpoints`` [N+1] or [B, N+1].  The reference's constraints and its
        default parametrizer read nothing else of a path, so every pass returns the reference's bits for the path class that
        produced the samples.  The passes run on the fused sampled entries (``batch.solve_sampled_batch`` ...); with
        ``constraints`` their rows come from ``batch.sampled_rows_batch`` and ``inv_dyn`` receives the given samples.
        ``compute_trajectory("ParametrizeSpline")`` works; "ParametrizeConstAccel" and ``compute_trajectory_samples`` need
        the path between the gridpoints and raise NotImplementedError.  Shapes and the row limit (d <= 30 under
        Interpolation, 32 under Collocation) are checked here, before anything is launched."""
        self = cls(None, None, gridpoints, vlim, alim, interpolation=interpolation)
        self._set_constraints(constraints)
        _capi.make_sampled_problem(gridpoints, q, qs, qss, vlim, alim, interpolation=interpolation, solver=not self.constraints)
        self._samples = (q, qs, qss)
        if self.constraints:
            if q is None:
                raise ValueError("second-order constraints evaluate their inverse dynamics at q: give the path positions")
            self._check_constraints()
        if self.first_order:
            if q is None and any(getattr(c, "needs_q", False) for c in self.first_order):
                raise ValueError("a tool or control-point velocity limit evaluates the chain at q: give the path positions")
            self._check_first_order()
        return self

    def _set_constraints(self, constraints):
        """``constraints`` split by what they produce: the second-order ones (rows; ``self.constraints``, in list order) and
        the first-order ones (``self.first_order``: they only tighten the stage boxes, in list order after vlim)."""
        constraints = list(constraints) if constraints else []
        self.first_order = [c for c in constraints if getattr(c, "first_order", False)]
        self.constraints = [c for c in constraints if not getattr(c, "first_order", False)]

    def _sampled_args(self):
        return (self.gridpoints, self._samples[1], self._samples[2], self.vlim, self.alim)

    # -- constraint lists beyond velocity + acceleration limits ------------------------------------------------------
    # ``constraints``: BatchJointTorqueConstraint / BatchSecondOrderConstraint objects (toppra_amd.constraint), after the
    # velocity and acceleration limits in the reference's list order.  Their dense rows are built ONCE per object, on first
    # use (the reference builds them in the wrapper's constructor), by tpr_second_order_rows_batch from the path at the
    # gridpoints and three batched inverse-dynamics calls per constraint, and stay on the device (for numpy inputs: a device
    # copy beside the host arrays that dense_rows() returns); every
    # pass then runs on the dense-row entries (tpr_*_dense_batch: the reference's full Seidel iteration), each from a fresh
    # warm-start state like a fresh reference object.
    def _check_constraints(self):
        """Everything that can be refused from shapes alone, before any launch."""
        B, N, d = self._sizes()
        if len(self.constraints) > _capi.SO_MAX_BLOCKS:
            raise NotImplementedError("%d second-order constraints in one list: the row kernel takes %d"
                                      % (len(self.constraints), _capi.SO_MAX_BLOCKS))
        nC = _capi.sampled_rows_per_stage(d, self.alim, self.interpolation)
        for con in self.constraints:
            if not (hasattr(con, "block") and hasattr(con, "rows_per_stage")):
                raise NotImplementedError("%s is outside BatchTOPPRA (BatchJointTorqueConstraint, BatchSecondOrderConstraint, "
                                          "BatchCartesianAccelerationConstraint, BatchPointAccelerationConstraint, BatchJointLoadConstraint, "
                                          "BatchBaseWrenchConstraint and BatchToolWrenchConstraint are supported)" % type(con).__name__)
            con.check(B, N, d)
            nC += con.rows_per_stage(d) or 0
        _capi.check_row_limit(nC)

    # -- first-order constraints: BatchJointVelocityConstraintVarying / BatchBoundConstraint -------------------------------
    # They add no rows.  The bound sources [vlim (if given), then the first-order constraints in list order] are folded into
    # the stage boxes ONCE per object, on first use, by tpr_stage_boxes_batch, and the boxes stay on the device.  Without
    # second-order constraints the passes run on the boxed sampled entries (tpr_*_sampled_boxed_batch) -- for a spline-table
    # problem on path_eval_batch's q', q'' at the gridpoints, evaluated once; with them the rows are built WITHOUT vlim and
    # the dense entries take the boxes as their low / high.
    def _sizes(self):
        if self._samples is not None:
            return int(self._samples[1].shape[0]), int(self._samples[1].shape[1]) - 1, int(self._samples[1].shape[2])
        if getattr(self.coef, "ndim", 0) != 4:
            raise ValueError("coef must have shape [B, 4, nseg, d]")
        return int(self.coef.shape[0]), int(self.gridpoints.shape[-1]) - 1, int(self.coef.shape[3])

    def _check_first_order(self):
        """Everything that can be refused from shapes alone, before any launch."""
        B, N, d = self._sizes()
        nsrc = (self.vlim is not None) + sum(con.source_count() for con in self.first_order)
        if nsrc > _capi.BOUND_MAX_SOURCES:
            raise NotImplementedError("%d bound sources (vlim and the first-order constraints' bounds) in one list: the box "
                                      "kernel takes %d" % (nsrc, _capi.BOUND_MAX_SOURCES))
        for con in self.first_order:
            con.check(B, N, d)
        if not self.constraints:
            nC = _capi.sampled_rows_per_stage(d, self.alim, self.interpolation)
            if nC > _capi.MAX_DENSE_ROWS:
                raise NotImplementedError("%d dof under Interpolation: %d constraint rows per stage (incl. the two x_next rows), "
                                          "the boxed passes hold %d (30 dof; 32 under Collocation)" % (d, nC, _capi.MAX_DENSE_ROWS))

    def _path_eval(self):
        """q, q', q'' of a spline-table problem at the gridpoints, evaluated once per object."""
        if self._pe is None:
            self._pe = _batch.path_eval_batch(self.coef, self.breaks, self.gridpoints)
        return self._pe

    def stage_boxes(self):
        """(low, high) [B, N+1, 2] of [vlim, first-order constraints ...]: the reference wrapper's ``low_arr`` / ``high_arr``,
        as arrays of the kind the problem was given in.  Built on first use."""
        return self._boxed_state()[4:]

    def _boxed_state(self):
        if self._boxed is None:
            qs, qss = self._samples[1:] if self._samples is not None else (self._path_eval()["qs"], self._path_eval()["qss"])
            B, N, d = self._sizes()
            from .constraint import _like
            grid = _like(self.gridpoints, qs)
            sources = [("vlim", self.vlim)] if self.vlim is not None else []
            for con in self.first_order:
                if getattr(con, "needs_q", False):  # (a constraint on the robot's pose, not only on q')
                    q = self._samples[0] if self._samples is not None else self._path_eval()["q"]
                    sources += con.bound_sources(grid, B, N, d, qs, q=q)
                else:
                    sources += con.bound_sources(grid, B, N, d, qs)
            low, high = _batch.stage_boxes_batch(qs, sources)
            self._boxed = (self.gridpoints, qs, qss, self.alim, low, high)
        return self._boxed

    @staticmethod
    def _device_copy(arrays, like):
        """``arrays`` themselves when ``like`` is a tensor.  A numpy problem: a device copy, made once per object (the passes
        would otherwise upload the samples and boxes, or 3 B (N+1) nC doubles of rows, every time)."""
        if _capi.is_torch_cuda(like):
            return arrays
        import torch
        dev = torch.device("cuda", _capi.init())
        return tuple(None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev) for v in arrays)

    @staticmethod
    def _device_pass(fn, given, device, *args, **kw):
        """``fn`` on ``device``, the device copy of the arrays ``given``; outputs in the kind of ``given``."""
        out = fn(*device, *args, **kw)
        if device is given:
            return out
        host = lambda v: v.cpu().numpy()  # noqa: E731
        if isinstance(out, dict):
            return {k: host(v) for k, v in out.items()}
        return tuple(host(v) for v in out) if isinstance(out, tuple) else host(out)

    def _boxed_pass(self, fn, *args, **kw):
        """One pass on the device-resident samples and boxes; outputs in the kind of the inputs."""
        if self._boxed_dev is None:
            self._boxed_dev = self._device_copy(self._boxed_state(), self._boxed_state()[1])
        return self._device_pass(fn, self._boxed, self._boxed_dev, *args, **kw)

    def dense_rows(self):
        """(a, b, c, low, high, deltas) of the constraint list, as arrays of the kind the problem was given in: the arguments
        of the ``batch.*_dense_batch`` calls.  Built on first use.  A constraint whose F and g are both callables has no
        row count before its callbacks have run: for such a list the 122-row limit is checked here, after the path
        evaluation and the callbacks and before the row kernel is launched, not in the constructor."""
        if self._rows is None:
            vlim = None if self.first_order else self.vlim  # (with first-order constraints the boxes carry vlim too)
            if self._samples is not None:
                blocks = [con.block(*self._samples) for con in self.constraints]
                rows = _batch.sampled_rows_batch(self.gridpoints, self._samples[1], self._samples[2], vlim, self.alim, blocks,
                                                 self.interpolation)
            else:
                pe = self._path_eval()
                blocks = [con.block(pe["q"], pe["qs"], pe["qss"]) for con in self.constraints]
                rows = _batch.second_order_rows_batch(self.coef, self.breaks, self.gridpoints, vlim, self.alim, blocks,
                                                      self.interpolation)
            if self.first_order:
                rows["low"], rows["high"] = self.stage_boxes()
            self._rows = tuple(rows[k] for k in ("a", "b", "c", "low", "high", "deltas"))
            self._rows_dev = self._device_copy(self._rows, rows["a"])
        return self._rows

    def _dense_pass(self, fn, *args, **kw):
        """One pass on the device-resident rows; outputs in the kind of the inputs."""
        self.dense_rows()
        return self._device_pass(fn, self._rows, self._rows_dev, *args, **kw)

    def _pass(self, name, *args, table=(), **kw):
        """The pass ``name`` -- the stem of its ``batch.*`` functions -- on the route this object takes: dense rows (with
        ``constraints``), boxed samples (with first-order constraints), samples, else the spline table.  ``table``: keywords of
        the spline-table function alone."""
        if self.constraints:
            return self._dense_pass(getattr(_batch, name + "_dense_batch"), *args, **kw)
        kw["interpolation"] = self.interpolation
        if self.first_order:
            return self._boxed_pass(getattr(_batch, name + "_sampled_boxed_batch"), *args, **kw)
        if self._samples is not None:
            return getattr(_batch, name + "_sampled_batch")(*self._sampled_args(), *args, **kw)
        if name == "solve_desired_duration":  # (the spline-table TOPPRAsd is not told the discretisation)
            del kw["interpolation"]
        return getattr(_batch, name + "_batch")(self.coef, self.breaks, self.gridpoints, self.vlim, self.alim, *args, **kw, **dict(table))

    @classmethod
    def from_waypoints(cls, knots, waypoints, gridpoints, vlim, alim, bc_type="not-a-knot", gpu_fit=True, **kw):
        """Build the batch from waypoints [B, m, d].  ``gpu_fit`` selects the batched GPU spline fit
        (``batch.spline_fit_batch``, bit-identical to scipy for the supported boundary conditions);
        otherwise one batched scipy ``CubicSpline`` call on the host."""
        if gpu_fit:
            coef, breaks = _batch.spline_fit_batch(knots, waypoints, bc_type)
        else:
            coef, breaks = _batch.spline_coefficients(knots, waypoints, bc_type)
        if not hasattr(gridpoints, "data_ptr"):
            gridpoints = np.asarray(gridpoints, dtype=np.float64)
        return cls(coef, breaks, gridpoints, vlim, alim, **kw)

    def compute_parameterization(self, sd_start=None, sd_end=None, want_sd=True, variant=0, want_K=True, want_u=True):
        """dict(sd2, sd, u, K, status): per-trajectory results; status 0/1/2 = Ok /
        FailUncontrollable / ErrUnknown, failed rows NaN-filled.  ``want_K`` / ``want_u`` = False leave the
        controllable sets / path accelerations in a device workspace (fewer bytes back to a host caller).
        With ``constraints`` the dense-row entry serves the call (``variant`` does not apply; K and u are always returned)."""
        # (the dense, boxed and sampled entries always return K and u; ``variant`` does not apply to them)
        return self._pass("solve", sd_start, sd_end, want_sd=want_sd, table=dict(variant=variant, want_K=want_K, want_u=want_u))

    def compute_parameterization_sd(self, desired_duration, sd_start=None, sd_end=None, atol=1e-5):
        """TOPPRAsd for the batch: dict(sd2, sd, u, K, status, alpha)."""
        return self._pass("solve_desired_duration", desired_duration, sd_start, sd_end, atol)

    def compute_trajectory(self, sd_start=None, sd_end=None, parametrizer="ParametrizeSpline"):
        """``ParameterizationAlgorithm.compute_trajectory`` (algorithm/algorithm.py:174-215) for the batch:
        parameterize, then build the output trajectories q(t) with the reference's parametrizer --
        "ParametrizeSpline" (its default) or "ParametrizeConstAccel" -- entirely on the GPU.  Returns a
        :class:`BatchTrajectory`; trajectories that could not be parameterized have ``status != 0`` and
        NaN durations (the reference returns None for them)."""
        if self._samples is not None:
            if parametrizer == "ParametrizeConstAccel":
                raise NotImplementedError("ParametrizeConstAccel evaluates the path between the gridpoints: a batch given as "
                                          "samples at the gridpoints has ParametrizeSpline only")
            if parametrizer == "ParametrizeSpline" and self._samples[0] is None:
                raise ValueError("ParametrizeSpline needs the path positions q at the gridpoints")
        res = self.compute_parameterization(sd_start, sd_end, want_sd=True, want_K=False, want_u=False)  # retiming reads sd only
        if parametrizer == "ParametrizeSpline" and self._samples is not None:
            sp = _batch.param_spline_samples_batch(self.gridpoints, self._samples[0], self._samples[1], res["sd"])
            return BatchTrajectory("spline", res, self, spline=sp)
        if parametrizer == "ParametrizeSpline":
            sp = _batch.param_spline_batch(self.coef, self.breaks, self.gridpoints, res["sd"])
            return BatchTrajectory("spline", res, self, spline=sp)
        if parametrizer == "ParametrizeConstAccel":
            ts, us = _batch.const_accel_times_batch(self.gridpoints, res["sd"])
            return BatchTrajectory("const_accel", res, self, ts=ts, us=us)
        raise NotImplementedError("parametrizer %r (ParametrizeSpline and ParametrizeConstAccel are available)" % (parametrizer,))


    def compute_trajectory_samples(self, times, sd_start=None, sd_end=None, fractions=True, orders=(0,)):
        """``traj = compute_trajectory(); traj(ts, order)`` (examples/plot_kinematics.py:48-57) for the batch WITHOUT the
        spline's coefficient table in between (2.9 GB at 65536 x 7 x 200): parameterize, then q / dq/dt / d2q/dt2 of the
        reference's default parametrizer (ParametrizeSpline) at ``times`` -- [T] fractions of each trajectory's duration
        (``np.linspace(0, 1, T)``) or [B, T] (fractions, or absolute times with ``fractions=False``).  Returns
        dict(q / qd / qdd [B, T, d] for the requested orders, duration [B], status [B]); the same bits as
        ``compute_trajectory()`` followed by its evaluation.  Up to 16 dof."""
        if self._samples is not None:
            raise NotImplementedError("compute_trajectory_samples fits and evaluates from the spline table: a batch given as "
                                      "samples at the gridpoints has compute_trajectory('ParametrizeSpline')")
        res = self.compute_parameterization(sd_start, sd_end, want_sd=True, want_K=False, want_u=False)
        out = _batch.param_spline_sample_batch(self.coef, self.breaks, self.gridpoints, res["sd"], times, fractions=fractions,
                                               orders=orders)
        out["status"] = res["status"]
        return out

    def compute_controllable_sets(self, sdmin, sdmax):
        return self._pass("controllable_sets", sdmin, sdmax)

    def compute_feasible_sets(self):
        return self._pass("feasible_sets")

    def compute_reachable_sets(self, sdmin, sdmax):
        """L[B, N+1, 2] (reachability_algorithm.py:409-431 per trajectory)."""
        return self._pass("reachable_sets", sdmin, sdmax)

    @staticmethod
    def return_codes(status):
        return [_STATUS_TO_CODE[int(s)] for s in np.asarray(status)]


class BatchTrajectory(object):
    """B output trajectories q_b(t) on the GPU (``AbstractGeometricPath`` surface, batched):
    ``duration`` [B], ``__call__(times [B, T], order) -> [B, T, d]``, ``status`` [B]."""

    def __init__(self, kind, result, problem, spline=None, ts=None, us=None):
        self.kind, self.result, self._p = kind, result, problem
        self.status = result["status"]
        self._sp, self._ts, self._us = spline, ts, us

    @property
    def duration(self):
        """[B] seconds (NaN where the parameterization failed)."""
        status = self.status
        if self.kind == "spline":
            tk, cnt = self._sp["knot_times"], self._sp["counts"]
            if hasattr(tk, "gather"):  # torch
                dur = tk.gather(1, (cnt.long() - 1).clamp(min=0)[:, None])[:, 0]
                return dur.masked_fill(status.to(dur.device) != 0, float("nan"))
            dur = tk[np.arange(tk.shape[0]), np.maximum(cnt - 1, 0)]
        else:
            dur = self._ts[:, -1]
            if hasattr(dur, "masked_fill"):
                return dur.masked_fill(status.to(dur.device) != 0, float("nan"))
        return np.where(np.asarray(status) != 0, np.nan, dur)

    def __call__(self, times, order=0):
        if self.kind == "spline":
            return _batch.ppoly_eval_batch(self._sp["coef"], self._sp["knot_times"], times, order, self._sp["counts"])
        return _batch.const_accel_eval_batch(self._p.coef, self._p.breaks, self._p.gridpoints, self.result["sd"],
                                             self._ts, self._us, times, order)

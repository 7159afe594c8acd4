"""Constraint classes of the hot path: joint velocity and joint acceleration limits.

Same class names, constructor arguments and error behaviour as toppra/constraint/
(linear_joint_velocity.py:8-53, linear_joint_acceleration.py:8-104, constraint.py:10-103).
``compute_constraint_params`` returns the reference's 7-tuple ``(a, b, c, F, g, ubound, xbound)``
but the numbers come from the HIP library (``tpr_constraint_params_batch``), not from numpy.
"""
from enum import Enum

import numpy as np

from . import _capi
from . import batch as _batch
from . import contact as _contact
from .chain import KinematicTree, SerialChain
from .interpolator import path_samples, spline_tables


class ConstraintType(Enum):
    Unknown = -1
    CanonicalLinear = 0
    CanonicalConic = 1


class DiscretizationType(Enum):
    Collocation = 0
    Interpolation = 1


class Constraint(object):
    """Base class (constraint.py:34-103)."""

    constraint_type = ConstraintType.Unknown
    discretization_type = DiscretizationType.Collocation
    n_extra_vars = 0
    dof = -1
    _format_string = ""

    def __repr__(self):
        return "%s(\n    Type: %s\n    Discretization Scheme: %s\n%s)" % (
            self.__class__.__name__, self.constraint_type, self.discretization_type, self._format_string)

    def get_dof(self):
        return self.dof

    def get_no_extra_vars(self):
        return self.n_extra_vars

    def get_constraint_type(self):
        return self.constraint_type

    def get_discretization_type(self):
        return self.discretization_type

    def set_discretization_type(self, discretization_type):
        if discretization_type in (0, DiscretizationType.Collocation):
            self.discretization_type = DiscretizationType.Collocation
        elif discretization_type in (1, DiscretizationType.Interpolation):
            self.discretization_type = DiscretizationType.Interpolation
        elif getattr(discretization_type, "value", None) in (0, 1):  # the reference's own enum
            self.discretization_type = DiscretizationType(discretization_type.value)
        else:
            raise NotImplementedError("Discretization type: %s not implemented!" % (discretization_type,))

    def compute_constraint_params(self, path, gridpoints, *args, **kwargs):
        raise NotImplementedError


class LinearConstraint(Constraint):
    """Canonical linear constraint a u + b x + c in {F v <= g} (linear_constraint.py:9-81)."""

    def __init__(self):
        self.constraint_type = ConstraintType.CanonicalLinear
        self.discretization_type = DiscretizationType.Collocation
        self.n_extra_vars = 0
        self.dof = -1
        self.identical = False


def _limits(lim, what):
    lim = np.array(lim, dtype=float)
    if np.isnan(lim).any():
        raise ValueError("Bad %s given: %s" % (what, lim))
    if lim.ndim == 1:
        lim = np.vstack((-lim, lim)).T
    assert lim.shape[1] == 2, "Wrong input shape."
    return lim


def _check_dof(constraint, path):
    if path.dof != constraint.get_dof():
        raise ValueError("Wrong dimension: constraint dof ({:d}) not equal to path dof ({:d})".format(
            constraint.get_dof(), path.dof))


def _params_on_device(path, gridpoints, vlim=None, alim=None, interpolation=True):
    vlim, alim = None if vlim is None else vlim[None], None if alim is None else alim[None]
    try:
        coef, breaks = spline_tables(path)
    except NotImplementedError:
        # any other geometric path: path(gridpoints, 1) and path(gridpoints, 2) evaluated on the host, as the reference
        # evaluates them (linear_joint_velocity.py:48, linear_joint_acceleration.py:72-73), and the same rows from the samples
        qs, qss = path_samples(path, gridpoints)
        return _batch.sampled_rows_batch(np.asarray(gridpoints, dtype=np.float64), qs[None], qss[None], vlim, alim,
                                         interpolation=interpolation)
    return _batch.constraint_params_batch(coef[None], breaks, np.asarray(gridpoints, dtype=np.float64), vlim, alim, interpolation)


class JointVelocityConstraint(LinearConstraint):
    """vlim[j, 0] <= qdot_j <= vlim[j, 1]; becomes a bound on x = sd^2 at every gridpoint."""

    def __init__(self, vlim):
        super(JointVelocityConstraint, self).__init__()
        self.vlim = _limits(vlim, "velocity")
        self.dof = self.vlim.shape[0]
        for i in range(self.dof):
            if self.vlim[i, 0] >= self.vlim[i, 1]:
                raise ValueError("Bad velocity limits: {:} (lower limit) > {:} (higher limit)".format(
                    self.vlim[i, 0], self.vlim[i, 1]))
        self._format_string = "    Velocity limit: \n" + "".join(
            "      J{:d}: {:}\n".format(i + 1, self.vlim[i]) for i in range(self.dof))

    def compute_constraint_params(self, path, gridpoints, *args, **kwargs):
        _check_dof(self, path)
        out = _params_on_device(path, gridpoints, vlim=self.vlim)
        return None, None, None, None, None, None, np.array(out["xbound"][0])


class JointAccelerationConstraint(LinearConstraint):
    """alim[j, 0] <= q'_j u + q''_j x <= alim[j, 1] (Interpolation scheme by default)."""

    def __init__(self, alim, discretization_scheme=DiscretizationType.Interpolation):
        super(JointAccelerationConstraint, self).__init__()
        self.alim = _limits(alim, "velocity")  # sic: the reference's message says "velocity" too
        self.dof = self.alim.shape[0]
        self.set_discretization_type(discretization_scheme)
        self._format_string = "    Acceleration limit: \n" + "".join(
            "      J{:d}: {:}\n".format(i + 1, self.alim[i]) for i in range(self.dof))
        self.identical = True

    def compute_constraint_params(self, path, gridpoints, *args, **kwargs):
        _check_dof(self, path)
        interp = self.discretization_type == DiscretizationType.Interpolation
        out = _params_on_device(path, gridpoints, alim=self.alim, interpolation=interp)
        d = self.dof
        eye = np.vstack([np.eye(d), -np.eye(d)])
        g1 = np.concatenate([self.alim[:, 1], -self.alim[:, 0]])
        if not interp:
            a, b = out["a"][0, :, 2:2 + d], out["b"][0, :, 2:2 + d]
            return a, b, np.zeros_like(a), eye, g1, None, None
        # wrapper rows are [ +a_i | -a_i | +a~ | -a~ ]; the constraint-level a is [ a_i | a~ ]
        pick = np.r_[2:2 + d, 2 + 2 * d:2 + 3 * d]
        a, b = out["a"][0][:, pick], out["b"][0][:, pick]
        F = np.zeros((4 * d, 2 * d))
        F[:2 * d, :d] = eye
        F[2 * d:, d:] = eye
        return a, b, np.zeros_like(a), F, np.concatenate([g1, g1]), None, None


class JointVelocityConstraintVarying(LinearConstraint):
    """Joint velocity limits that vary along the path: ``vlim_func(s) -> [dof, 2]`` (linear_joint_velocity.py:55-87).
    Only ``xbound`` is produced.  Evaluated on the host (a Python callback per gridpoint, as in the reference) with the
    reference's arithmetic: the running bounds sdmin / sdmax are C floats (``_CythonUtils.pyx:60-101`` -- every min / max
    is rounded to fp32 on assignment, the upper bound is squared in fp32), the quotients are doubles.  Lists holding it
    run on the dense-row entries (hipDenseSeidelWrapper)."""

    def __init__(self, vlim_func):
        super(JointVelocityConstraintVarying, self).__init__()
        self.dof = np.shape(vlim_func(0))[0]
        self.vlim_func = vlim_func
        self._format_string = "    Varying Velocity limit: \n"

    def compute_constraint_params(self, path, gridpoints, *args, **kwargs):
        _check_dof(self, path)
        gridpoints = np.asarray(gridpoints, dtype=float)
        qs = np.asarray(path(gridpoints, 1), dtype=float)
        xbound = np.zeros((len(gridpoints), 2))
        for i, s in enumerate(gridpoints):
            vlim = np.asarray(self.vlim_func(s), dtype=float)
            sdmin, sdmax = np.float32(-1e8), np.float32(1e8)  # MAXSD
            for k in range(self.dof):
                if qs[i, k] > 0:
                    hi, lo = vlim[k, 1] / qs[i, k], vlim[k, 0] / qs[i, k]
                elif qs[i, k] < 0:
                    hi, lo = vlim[k, 0] / qs[i, k], vlim[k, 1] / qs[i, k]
                else:
                    continue
                sdmax = np.float32(hi if hi < float(sdmax) else float(sdmax))
                sdmin = np.float32(lo if lo > float(sdmin) else float(sdmin))
            lower = float(sdmin) if float(sdmin) > 0.0 else 0.0
            xbound[i] = lower * lower, float(sdmax * sdmax)
        return None, None, None, None, None, None, xbound


def colloc_to_interpolate(a, b, c, F, g, xbound, ubound, gridpoints, identical=False):
    """First-order interpolation form of canonical-linear parameters (linear_constraint.py:84-192): the constraint of
    stage i is imposed at gridpoint i and, through x_{i+1} = x_i + 2 delta_i u_i, at gridpoint i + 1 -- the row blocks
    [a_i | a_{i+1} + 2 delta_i b_{i+1}], [b_i | b_{i+1}], [c_i | c_{i+1}] against blkdiag(F_i, F_{i+1}), [g_i | g_{i+1}];
    the last stage repeats itself.  ``identical``: one F (m x d) and g (m) for every gridpoint.  Host numpy, like the
    reference: these parameters come from user callbacks (inverse dynamics) and feed the dense-row entries
    (tpr_*_dense_batch)."""
    if a is None:
        return None, None, None, None, None, xbound, ubound
    a, b, c = (np.asarray(v, dtype=float) for v in (a, b, c))
    two_delta = 2 * np.diff(np.asarray(gridpoints, dtype=float)).reshape(-1, 1)
    nxt = lambda v: np.concatenate((v[1:], v[-1:]), axis=0)  # noqa: E731  (gridpoint i + 1; the last one repeats itself)
    a_next = np.concatenate((a[1:] + two_delta * b[1:], a[-1:]), axis=0)
    a2, b2, c2 = np.hstack((a, a_next)), np.hstack((b, nxt(b))), np.hstack((c, nxt(c)))
    F, g = np.asarray(F, dtype=float), np.asarray(g, dtype=float)
    if identical:
        m, d = F.shape
        F2 = np.zeros((2 * m, 2 * d))
        F2[:m, :d] = F
        F2[m:, d:] = F
        g2 = np.concatenate((g, g))
    else:
        n1, m, d = F.shape
        F2 = np.zeros((n1, 2 * m, 2 * d))
        F2[:, :m, :d] = F
        F2[:, m:, d:] = nxt(F)
        g2 = np.hstack((g, nxt(g)))
    return a2, b2, c2, F2, g2, xbound, ubound


def _second_order_coefficients(inv_dyn, q, qs, qss):
    """(a, b, c)[N+1, m] of  w = a(s) sdd + b(s) sd^2 + c(s)  from an inverse-dynamics callback by substitution:
    c = tau(q, 0, 0), a = tau(q, 0, q') - c, b = tau(q, q', q'') - c (linear_second_order.py:154-162)."""
    zero = np.zeros(q.shape[1])
    c = np.array([inv_dyn(q_i, zero, zero) for q_i in q], dtype=float)
    a = np.array([inv_dyn(q_i, zero, qs_i) for q_i, qs_i in zip(q, qs)], dtype=float) - c
    b = np.array([inv_dyn(q_i, qs_i, qss_i) for q_i, qs_i, qss_i in zip(q, qs, qss)], dtype=float) - c
    return a, b, c


class SecondOrderConstraint(LinearConstraint):
    """General second-order constraint  A(q) qdd + qd^T B(q) qd + C(q) = w,  F(q) w <= g(q)  given by an inverse-dynamics
    callback ``inv_dyn(q, qd, qdd) -> w`` and callbacks ``constraint_F(q)``, ``constraint_g(q)``
    (linear_second_order.py:11-173); ``custom_term(path, s)`` is added to c (joint friction).  The parameters are
    evaluated on the host, through the user's callbacks, as in the reference; the solve runs on the dense-row entries
    (hipDenseSeidelWrapper)."""

    def __init__(self, inv_dyn, constraint_F, constraint_g, dof, custom_term=None,
                 discretization_scheme=DiscretizationType.Interpolation):
        super(SecondOrderConstraint, self).__init__()
        self.set_discretization_type(discretization_scheme)
        self.inv_dyn = inv_dyn
        self.constraint_F = constraint_F
        self.constraint_g = constraint_g
        self.dof = dof
        self.custom_term = custom_term
        self._format_string = "    Kind: Generalized Second-order constraint\n    Dimension:\n        F in R^({:d}, {:d})\n".format(
            *np.shape(constraint_F(np.zeros(dof))))

    @classmethod
    def joint_torque_constraint(cls, inv_dyn, taulim, joint_friction, **kwargs):
        """Joint torque bounds taulim [dof, 2] with dry friction joint_friction [dof] (sign(q') * friction added to c)."""
        taulim = np.asarray(taulim, dtype=float)
        dof = taulim.shape[0]
        F = np.vstack((np.eye(dof), -np.eye(dof)))
        g = np.concatenate((taulim[:, 1], -taulim[:, 0]))
        return cls(inv_dyn, lambda _q: F, lambda _q: g, dof,
                   lambda path, s: np.sign(path(s, 1)) * joint_friction, **kwargs)

    def compute_constraint_params(self, path, gridpoints, *args, **kwargs):
        _check_dof(self, path)
        gridpoints = np.asarray(gridpoints, dtype=float)
        q = np.asarray(path(gridpoints))
        a, b, c = _second_order_coefficients(self.inv_dyn, q, np.asarray(path(gridpoints, 1)), np.asarray(path(gridpoints, 2)))
        F = np.array([self.constraint_F(q_i) for q_i in q], dtype=float)
        g = np.array([self.constraint_g(q_i) for q_i in q], dtype=float)
        if self.custom_term is not None:
            for i, s in enumerate(gridpoints):
                c[i] = c[i] + self.custom_term(path, s)
        if self.discretization_type == DiscretizationType.Collocation:
            return a, b, c, F, g, None, None
        return colloc_to_interpolate(a, b, c, F, g, None, None, gridpoints)


class JointTorqueConstraint(LinearConstraint):
    """Joint torque bounds  tau_lim[:, 0] <= inv_dyn(q, qd, qdd) + fs_coef * sign(qd) <= tau_lim[:, 1]
    (joint_torque.py:10-116): one F = [I; -I], g = [tau_max; -tau_min] for every gridpoint (``identical``)."""

    def __init__(self, inv_dyn, tau_lim, fs_coef, discretization_scheme=DiscretizationType.Collocation):
        super(JointTorqueConstraint, self).__init__()
        self.inv_dyn = inv_dyn
        self.tau_lim = np.array(tau_lim, dtype=float)
        assert self.tau_lim.ndim == 2 and self.tau_lim.shape[1] == 2, "Wrong input shape."
        self.fs_coef = np.array(fs_coef, dtype=float)
        self.dof = self.tau_lim.shape[0]
        self.set_discretization_type(discretization_scheme)
        self.identical = True
        self._format_string = "    Torque limit: \n" + "".join(
            "      J{:d}: {:}\n".format(i + 1, lim) for i, lim in enumerate(self.tau_lim))

    def compute_constraint_params(self, path, gridpoints, *args, **kwargs):
        _check_dof(self, path)
        gridpoints = np.asarray(gridpoints, dtype=float)
        qs = np.asarray(path(gridpoints, 1))
        a, b, c = _second_order_coefficients(self.inv_dyn, np.asarray(path(gridpoints)), qs, np.asarray(path(gridpoints, 2)))
        for k in range(self.dof):  # dry friction
            c[:, k] += self.fs_coef[k] * np.sign(qs[:, k])
        eye = np.eye(self.dof)
        F = np.vstack((eye, -eye))
        g = np.concatenate((self.tau_lim[:, 1], -self.tau_lim[:, 0]))
        if self.discretization_type == DiscretizationType.Collocation:
            return a, b, c, F, g, None, None
        return colloc_to_interpolate(a, b, c, F, g, None, None, gridpoints, identical=True)


# ---- batched second-order / torque constraints: rows built on the GPU (BatchTOPPRA(..., constraints=[...])) ----------------

def _like(x, like):
    """`x` as a float64 array of the kind of `like`: numpy, or a torch tensor on like's device."""
    if _capi.is_torch_cuda(like):
        import torch
        return torch.as_tensor(x, dtype=torch.float64, device=like.device)
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def _shape_of(x):
    return tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x, dtype=np.float64)


def _zeros_like(x):
    return np.zeros_like(x) if isinstance(x, np.ndarray) else x.new_zeros(tuple(x.shape))


def _check_chain_dof(inv_dyn, d):
    if isinstance(inv_dyn, (SerialChain, KinematicTree)) and inv_dyn.dof != d:
        raise ValueError("Wrong dimension: the {:s} has {:d} joints, the path {:d} dof".format(
            "tree" if isinstance(inv_dyn, KinematicTree) else "chain", inv_dyn.dof, d))


def _check_leading(F_shape, g_shape, B, N):
    """The axes of rows F [..., m, p] and g [..., m] before those (a shape; None = not an array): none, [B] or [B, N+1]."""
    for name, shape, tail in (("F", F_shape, 2), ("g", g_shape, 1)):
        if shape is not None and tuple(shape[:-tail]) not in ((), (B,), (B, N + 1)):
            raise ValueError("%s has leading shape %s: one for the batch, [B] = [%d] or [B, N+1] = [%d, %d] is expected"
                             % (name, tuple(shape[:-tail]), B, B, N + 1))


class _BatchSecondOrder(LinearConstraint):
    """Shared part of the batched second-order constraints: the three batched inverse-dynamics evaluations of the
    reference's substitution (linear_second_order.py:154-162) and the block description that
    :func:`toppra_amd.batch.second_order_rows_batch` takes."""

    def _evaluate(self, q, qs, qss):
        """w0 = tau(q, 0, 0), wa = tau(q, 0, q'), wb = tau(q, q', q''): exactly three calls, each checked -- or, for a
        :class:`toppra_amd.chain.SerialChain` or :class:`toppra_amd.chain.KinematicTree`, one launch that evaluates the three
        (the values of the three calls)."""
        if isinstance(self.inv_dyn, (SerialChain, KinematicTree)):
            return list(self.inv_dyn.torque_terms(q, qs, qss))
        zero = _zeros_like(q)
        out = []
        for what, args in (("(q, 0, 0)", (q, zero, zero)), ("(q, 0, q')", (q, zero, qs)), ("(q, q', q'')", (q, qs, qss))):
            w = self.inv_dyn(*args)
            if type(w) is not type(q) and not (isinstance(w, np.ndarray) and isinstance(q, np.ndarray)):
                raise ValueError("inv_dyn%s must return %s like its arguments, got %s" % (what, type(q).__name__, type(w).__name__))
            if w.ndim != 3 or tuple(w.shape[:2]) != tuple(q.shape[:2]) or (out and tuple(w.shape) != tuple(out[0].shape)):
                raise ValueError("inv_dyn%s must return an array [B, N+1, p] = [%d, %d, p], got %s"
                                 % (what, q.shape[0], q.shape[1], tuple(w.shape)))
            out.append(w)
        return out

    def _interp(self):
        return self.discretization_type == DiscretizationType.Interpolation

    def rows_per_stage(self, d):
        """Rows this constraint adds to a stage (None while they depend on a callback's output)."""
        raise NotImplementedError

    def check(self, B, N, d):
        """Shape errors that can be told from the problem's sizes alone (ValueError), before any launch."""
        raise NotImplementedError

    def block(self, q, qs, qss):
        raise NotImplementedError

    def compute_constraint_params(self, path, gridpoints, *args, **kwargs):
        raise NotImplementedError("%s serves BatchTOPPRA(..., constraints=[...]); the single-path classes take %s"
                                  % (type(self).__name__, type(self).__name__.replace("Batch", "")))


class BatchJointTorqueConstraint(_BatchSecondOrder):
    """``JointTorqueConstraint`` (joint_torque.py:10-116) for a batch:  tau_lim[..., 0] <= inv_dyn(q, qd, qdd) + fs_coef *
    sign(qd) <= tau_lim[..., 1].

    ``inv_dyn(q, qd, qdd)`` is BATCHED: three arrays [B, N+1, d] in, [B, N+1, d] out -- numpy arrays when the problem was
    given as numpy, torch tensors on the problem's device otherwise -- and is called exactly three times.  A
    :class:`toppra_amd.chain.SerialChain` -- or, for a branched robot, a :class:`toppra_amd.chain.KinematicTree` -- may stand in
    its place: the robot's inverse dynamics then run on the GPU, the three evaluations in one launch (the values of
    ``inv_dyn=chain.inverse_dynamics``).  ``tau_lim``:
    [d, 2] or [B, d, 2]; ``fs_coef``: [d] or [B, d].  Defaults are the reference's (Collocation)."""

    def __init__(self, inv_dyn, tau_lim, fs_coef, discretization_scheme=DiscretizationType.Collocation):
        super(BatchJointTorqueConstraint, self).__init__()
        self.inv_dyn = inv_dyn
        self.tau_lim, self.fs_coef = tau_lim, fs_coef
        shape = _shape_of(tau_lim)
        if len(shape) not in (2, 3) or shape[-1] != 2:
            raise ValueError("tau_lim must have shape [d, 2] or [B, d, 2], got %s" % (shape,))
        self.dof = int(shape[-2])
        fshape = _shape_of(fs_coef)
        if len(fshape) not in (1, 2) or fshape[-1] != self.dof:
            raise ValueError("fs_coef must have shape [d] or [B, d] with d = %d, got %s" % (self.dof, fshape))
        self._tau_batch = shape[0] if len(shape) == 3 else None
        self._fs_batch = fshape[0] if len(fshape) == 2 else None
        self.set_discretization_type(discretization_scheme)
        self.identical = True
        self._format_string = "    Batched torque limit, %d dof\n" % self.dof

    def rows_per_stage(self, d):
        return (2 if self._interp() else 1) * 2 * self.dof

    def check(self, B, N, d):
        if self.dof != d:
            raise ValueError("Wrong dimension: constraint dof ({:d}) not equal to path dof ({:d})".format(self.dof, d))
        _check_chain_dof(self.inv_dyn, d)
        for name, n in (("tau_lim", self._tau_batch), ("fs_coef", self._fs_batch)):
            if n is not None and n != B:
                raise ValueError("%s is given per trajectory for %d trajectories, the problem has %d" % (name, n, B))

    def block(self, q, qs, qss):
        B, d = int(q.shape[0]), int(q.shape[2])
        self.check(B, int(q.shape[1]) - 1, d)
        w0, wa, wb = self._evaluate(q, qs, qss)
        if int(w0.shape[2]) != d:
            raise ValueError("inv_dyn must return joint torques [B, N+1, d] = [%d, %d, %d], got %s" % (B, q.shape[1], d, tuple(w0.shape)))
        lim, fs = _like(self.tau_lim, q), _like(self.fs_coef, q)
        cat = np.concatenate if isinstance(lim, np.ndarray) else __import__("torch").cat
        g = cat((lim[..., 1], -lim[..., 0]), -1)  # [tau_max; -tau_min]
        if fs.ndim == 1:
            fs = np.broadcast_to(fs, (B, d)) if isinstance(fs, np.ndarray) else fs.expand(B, d)
        return {"w0": w0, "wa": wa, "wb": wb, "F": None, "g": g, "friction": fs, "interpolation": self._interp()}


class BatchSecondOrderConstraint(_BatchSecondOrder):
    """``SecondOrderConstraint`` (linear_second_order.py:11-173) for a batch:  F w <= g  on  w = inv_dyn(q, qd, qdd).

    ``inv_dyn(q, qd, qdd)`` is BATCHED: three arrays [B, N+1, d] in, [B, N+1, p] out -- numpy arrays when the problem was
    given as numpy, torch tensors on the problem's device otherwise -- and is called exactly three times; or a
    :class:`toppra_amd.chain.SerialChain` or :class:`toppra_amd.chain.KinematicTree` (p = d: its joint torques, the three
    evaluations in one launch).  ``F``: [m, p],
    [B, m, p], [B, N+1, m, p], a batched callable of q returning [B, N+1, m, p], or None for the signed identity [I; -I]
    (what :meth:`joint_torque_constraint` builds: m = 2 p); ``g``: [m], [B, m], [B, N+1, m] or a batched callable of q.
    ``friction``: dry friction [d] or [B, d], friction * sign(q') is added to c (the ``custom_term`` of the reference's
    ``joint_torque_constraint``; needs p == d).  A general ``custom_term(path, s)`` beyond dry friction is out of scope: the
    reference evaluates it through a Python callback per gridpoint.  A dense F row is summed in index order k = 0 .. p-1
    (include/toppra_hip.h).  Defaults are the reference's (Interpolation)."""

    def __init__(self, inv_dyn, F, g, friction=None, discretization_scheme=DiscretizationType.Interpolation):
        super(BatchSecondOrderConstraint, self).__init__()
        self.inv_dyn = inv_dyn
        self.F, self.g, self.friction = F, g, friction
        self.set_discretization_type(discretization_scheme)
        if F is not None and not callable(F):
            shape = _shape_of(F)
            if len(shape) not in (2, 3, 4):
                raise ValueError("F must have shape [m, p], [B, m, p] or [B, N+1, m, p], got %s" % (shape,))
        if not callable(g):
            gshape = _shape_of(g)
            if len(gshape) not in (1, 2, 3):
                raise ValueError("g must have shape [m], [B, m] or [B, N+1, m], got %s" % (gshape,))
            if F is not None and not callable(F) and gshape[-1] != shape[-2]:
                raise ValueError("g has %d entries per gridpoint, F has %d rows" % (gshape[-1], shape[-2]))
        if friction is not None:
            fshape = _shape_of(friction)
            if len(fshape) not in (1, 2):
                raise ValueError("friction must have shape [d] or [B, d], got %s" % (fshape,))
        self._format_string = "    Kind: Batched generalized second-order constraint\n"

    @classmethod
    def joint_torque_constraint(cls, inv_dyn, taulim, joint_friction, **kwargs):
        """Joint torque bounds taulim [d, 2] or [B, d, 2] with dry friction joint_friction [d] or [B, d]
        (linear_second_order.py:100-140): the signed identity with g = [tau_max; -tau_min]."""
        shape = _shape_of(taulim)
        if len(shape) not in (2, 3) or shape[-1] != 2:
            raise ValueError("taulim must have shape [d, 2] or [B, d, 2], got %s" % (shape,))
        if hasattr(taulim, "detach"):
            import torch
            g = torch.cat((taulim[..., 1], -taulim[..., 0]), -1)
        else:
            taulim = np.asarray(taulim, dtype=np.float64)
            g = np.concatenate((taulim[..., 1], -taulim[..., 0]), -1)
        return cls(inv_dyn, None, g, friction=joint_friction, **kwargs)

    def _shape(self, x):
        return None if x is None or callable(x) else _shape_of(x)

    def rows_per_stage(self, d):
        F, g = self._shape(self.F), self._shape(self.g)
        m = F[-2] if F is not None else (g[-1] if g is not None else None)
        return None if m is None else (2 if self._interp() else 1) * int(m)

    def check(self, B, N, d):
        _check_chain_dof(self.inv_dyn, d)
        _check_leading(self._shape(self.F), self._shape(self.g), B, N)
        fr = self._shape(self.friction)
        if fr is not None and (fr[-1] != d or (len(fr) == 2 and fr[0] != B)):
            raise ValueError("friction must have shape [d] or [B, d] = [%d, %d], got %s" % (B, d, fr))

    def block(self, q, qs, qss):
        B, n1, d = (int(v) for v in q.shape)
        self.check(B, n1 - 1, d)
        w0, wa, wb = self._evaluate(q, qs, qss)
        p = int(w0.shape[2])
        F = self.F(q) if callable(self.F) else self.F
        g = self.g(q) if callable(self.g) else self.g
        F = None if F is None else _like(F, q)
        g = _like(g, q)
        if callable(self.F) and (F.ndim != 4 or tuple(F.shape[:2]) != (B, n1)):
            raise ValueError("the F callback must return [B, N+1, m, p] = [%d, %d, m, %d], got %s" % (B, n1, p, tuple(F.shape)))
        if callable(self.g) and (g.ndim != 3 or tuple(g.shape[:2]) != (B, n1)):
            raise ValueError("the g callback must return [B, N+1, m] = [%d, %d, m], got %s" % (B, n1, tuple(g.shape)))
        if F is not None and int(F.shape[-1]) != p:
            raise ValueError("F has %d columns, inv_dyn returns p = %d" % (int(F.shape[-1]), p))
        m = 2 * p if F is None else int(F.shape[-2])
        if int(g.shape[-1]) != m:
            raise ValueError("g has %d entries per gridpoint, F has %d rows" % (int(g.shape[-1]), m))
        fr = self.friction
        if fr is not None:
            if p != d:
                raise ValueError("dry friction needs inv_dyn to return joint torques (p == d = %d), got p = %d" % (d, p))
            fr = _like(fr, q)
            if fr.ndim == 1:
                fr = np.broadcast_to(fr, (B, d)) if isinstance(fr, np.ndarray) else fr.expand(B, d)
        return {"w0": w0, "wa": wa, "wb": wb, "F": F, "g": g, "friction": fr, "interpolation": self._interp()}


def _need_chain(chain):
    _batch._need(chain, "chain", "SerialChain")


def _need_robot(robot):
    _batch._need(robot, "robot", "SerialChain", "KinematicTree")


def _need_points(points, chain):
    _batch._need(points, "points", "ControlPoints").on(chain)  # (a link outside the chain: ValueError)


def _row_limits(F, g, width, shapes):
    """Limits given as rows F, g on a quantity ``width`` wide (``shapes``: the shapes of F in words): (F, g, None)."""
    if F is None or g is None:
        raise ValueError("F and g are given together")
    fshape, gshape = _shape_of(F), _shape_of(g)
    if len(fshape) not in (2, 3, 4) or fshape[-1] != width:
        raise ValueError("F must have shape %s, got %s" % (shapes, list(fshape)))
    if len(gshape) not in (1, 2, 3):
        raise ValueError("g must have shape [m], [B, m] or [B, N+1, m], got %s" % (list(gshape),))
    if gshape[-1] != fshape[-2]:
        raise ValueError("g has %d entries per gridpoint, F has %d rows" % (gshape[-1], fshape[-2]))
    for name, arr in (("F", F), ("g", g)):
        if not np.all(np.isfinite(_host(arr))):
            raise ValueError("%s holds a value that is not finite" % name)
    return F, g, None


def _box_limits(count, width, parts, letter, F, g):
    """The limits of a constraint on ``count`` units of ``width`` numbers each, unit-major -- one tool point or one wrench, S
    sections, P points -- given either as boxes on 3-wide parts of a unit or as rows F, g: (F, g, the B of boxes given per
    trajectory or None).  ``parts``: (name, limit, the part's first column in its unit) each; a limit is None, a scalar, [K] (a
    magnitude per unit), [K, 3, 2] or [B, K, 3, 2] (lower, upper).  ``letter`` names K in the messages (S, P); None = a lone unit,
    whose boxes are [3, 2] or [B, 3, 2] without the unit's axis and without the [K] spelling.  Each part given adds six rows per
    unit, the signed identity [+I; -I] on that part with g = [upper; -lower]: the rows are unit-major, within a unit the parts
    follow in their order, and g is laid out as the rows are."""
    names = tuple(name for name, _, _ in parts)
    boxes, rows = any(lim is not None for _, lim, _ in parts), F is not None or g is not None
    if boxes and rows:
        raise ValueError("give the limits either as %s or as F and g, not both" % " / ".join(names))
    if not boxes and not rows:
        raise ValueError("no limit given: %s%s, or F with g, is required" % ("one of " if len(names) > 1 else "", ", ".join(names)))
    if not boxes:
        wide = "%d" % width if letter is None else "%d %s" % (width, letter)
        shapes = "[m, %s], [B, m, %s] or [B, N+1, m, %s]" % (wide, wide, wide)
        return _row_limits(F, g, width * count, shapes if letter is None else "%s with %s = %d" % (shapes, wide, width * count))
    limit_batch, given = None, []
    for name, lim, at in parts:
        if lim is None:
            continue
        lim = _host(lim)
        shape = lim.shape
        if lim.ndim == 0 or (letter is not None and shape == (count,)):  # a magnitude: for every unit, or one per unit
            lim = np.broadcast_to(lim, (count,))
            lim = np.stack([np.repeat(-lim[:, None], 3, 1), np.repeat(lim[:, None], 3, 1)], -1)
        elif letter is None and lim.ndim >= 2:
            lim = lim.reshape(shape[:-2] + (1,) + shape[-2:])
        if lim.ndim not in (3, 4) or lim.shape[-3:] != (count, 3, 2):
            raise ValueError("%s must be a scalar or have shape %s, got %s" % (name, "[3, 2] or [B, 3, 2]" if letter is None else
                             "[%s], [%s, 3, 2] or [B, %s, 3, 2] with %s = %d" % (letter, letter, letter, letter, count), list(shape)))
        if not np.all(np.isfinite(lim)):
            raise ValueError("%s holds a limit that is not finite" % name)
        if np.any(lim[..., 0] > lim[..., 1]):
            raise ValueError("%s holds a lower limit above its upper limit" % name)
        if lim.ndim == 4:
            if limit_batch not in (None, lim.shape[0]):
                raise ValueError("%s and %s are given per trajectory for %d and %d trajectories" % (names + (limit_batch, lim.shape[0])))
            limit_batch = int(lim.shape[0])
        given.append((at, np.concatenate((lim[..., 1], -lim[..., 0]), -1)))  # [..., K, 6] = [upper; -lower] per unit
    per = 6 * len(given)  # rows per unit
    Fm = np.zeros((per * count, width * count))
    for k in range(count):
        for j, (at, _) in enumerate(given):
            r, c = per * k + 6 * j, width * k + at
            Fm[r:r + 3, c:c + 3], Fm[r + 3:r + 6, c:c + 3] = np.eye(3), -np.eye(3)
    lead = () if limit_batch is None else (limit_batch,)
    gm = np.concatenate([np.broadcast_to(gp, lead + (count, 6)) for _, gp in given], -1)  # [..., K, per]
    return Fm, np.ascontiguousarray(gm.reshape(lead + (per * count,))), limit_batch


class _BatchChainRows(_BatchSecondOrder):
    """Shared part of the constraints  F w <= g  on a quantity w(q, qd, qdd) that a chain kernel evaluates: the limits
    (``F``, ``g``, and the B of limits given per trajectory), the checks against a problem's sizes and the block.  A subclass
    is its constructor and :meth:`_terms`."""

    def __init__(self, chain, limits, discretization_scheme, what):
        super(_BatchChainRows, self).__init__()
        self.chain = chain
        self.dof = chain.dof
        self.F, self.g, self._limit_batch = limits
        self.set_discretization_type(discretization_scheme)
        self.identical = True
        self._format_string = "    Batched %s, %d rows\n" % (what, _shape_of(self.F)[-2])

    def _terms(self, q, qs, qss):
        """(w(q, 0, 0) -- None for an exact zero --, w(q, 0, q'), w(q, q', q'')), each [B, N+1, width]: one launch."""
        raise NotImplementedError

    def rows_per_stage(self, d):
        return (2 if self._interp() else 1) * int(_shape_of(self.F)[-2])

    def check(self, B, N, d):
        if self.dof != d:
            raise ValueError("Wrong dimension: the chain has {:d} joints, the path {:d} dof".format(self.dof, d))
        if self._limit_batch is not None and self._limit_batch != B:
            raise ValueError("the limits are given per trajectory for %d trajectories, the problem has %d" % (self._limit_batch, B))
        _check_leading(_shape_of(self.F), _shape_of(self.g), B, N)

    def block(self, q, qs, qss):
        B, n1, d = (int(v) for v in q.shape)
        self.check(B, n1 - 1, d)
        w0, wa, wb = self._terms(q, qs, qss)
        return {"w0": _zeros_like(wa) if w0 is None else w0, "wa": wa, "wb": wb, "F": _like(self.F, q), "g": _like(self.g, q),
                "friction": None, "interpolation": self._interp()}


class BatchCartesianAccelerationConstraint(_BatchChainRows):
    """A limit on the tool point's acceleration for a batch (the reference's example examples-old/cartesian_accel.py: a
    ``SecondOrderConstraint`` whose ``inv_dyn`` returns the link's acceleration):  F acc <= g  on  acc(q, qd, qdd) =
    [linear; angular] of ``chain``'s tool point in world axes -- the classical acceleration of the point and the last link's
    angular acceleration (:meth:`toppra_amd.chain.SerialChain.tool_acceleration`; kinematics, no gravity).  The two
    evaluations the rows need come from one launch of the chain kernel; acc(q, 0, 0) is an exact zero.

    ``chain``: a :class:`toppra_amd.chain.SerialChain`.  The limits are given in one of two spellings:

    ``linear`` / ``angular`` (either or both): a scalar ``amax`` (-amax <= component <= amax on each world axis), [3, 2] or
    [B, 3, 2] (lower, upper).  Each part given adds six rows, the signed identity on that part with g = [upper; -lower]; with
    both, the linear part's rows come first: F = [I 0; -I 0; 0 I; 0 -I] (12 rows).

    ``F`` [m, 6], [B, m, 6] or [B, N+1, m, 6] with ``g`` [m], [B, m] or [B, N+1, m], as ``BatchSecondOrderConstraint`` takes
    them: a polyhedral stand-in for a norm limit, or limits in a tilted frame.

    Defaults are the reference's for ``SecondOrderConstraint`` (Interpolation).  Needs the path positions: a
    ``from_path_samples`` batch must be given ``q``.  A true norm (conic) limit is out of scope; points on other links than
    the last are :class:`BatchPointAccelerationConstraint`'s."""

    def __init__(self, chain, linear=None, angular=None, F=None, g=None, discretization_scheme=DiscretizationType.Interpolation):
        _need_chain(chain)
        super(BatchCartesianAccelerationConstraint, self).__init__(
            chain, _box_limits(1, 6, (("linear", linear, 0), ("angular", angular, 3)), None, F, g), discretization_scheme,
            "tool acceleration limit, %d dof" % chain.dof)
        self.linear, self.angular = linear, angular

    def _terms(self, q, qs, qss):
        return (None,) + tuple(self.chain.tool_acceleration_terms(q, qs, qss))


class BatchToolWrenchConstraint(_BatchChainRows):
    """A limit on the wrench a chain's last link transmits to a carried object, for a batch:  F w <= g  on
    w(q, qd, qdd) = [force; moment] of ``chain`` on ``payload`` -- the force on the body and its moment about the contact
    frame's origin, in contact-frame axes, gravity included (:meth:`toppra_amd.chain.SerialChain.tool_wrench`).  It is the
    reference's ``SecondOrderConstraint`` with an ``inv_dyn`` that returns that wrench instead of joint torques; the three
    evaluations the rows need come from one launch of the chain kernel.

    ``chain``: a :class:`toppra_amd.chain.SerialChain`; ``payload``: a :class:`toppra_amd.chain.Payload`.  The limits are given
    in one of three spellings (mixing them is a ValueError):

    ``force`` / ``moment`` (either or both): a scalar ``wmax`` (-wmax <= component <= wmax on each contact-frame axis), [3, 2]
    or [B, 3, 2] (lower, upper) -- the overload box of a force/torque sensor.  Each part given adds six rows, the signed
    identity on that part with g = [upper; -lower]; with both, the force's rows come first.

    ``F`` [m, 6], [B, m, 6] or [B, N+1, m, 6] with ``g`` [m], [B, m] or [B, N+1, m], as ``BatchSecondOrderConstraint`` takes
    them.

    :meth:`surface_contact`: the contact wrench cone of a flat rectangular patch with Coulomb friction.

    The constraint is INFEASIBLE unless F w(q, 0, 0) <= g holds at every gridpoint: standing still must satisfy it (the
    static wrench is the body's weight, and it enters every stage's rows).  Defaults are the reference's for
    ``SecondOrderConstraint`` (Interpolation).  Needs the path positions: a ``from_path_samples`` batch must be given ``q``.
    Per-trajectory payloads, a true (conic) friction cone and a body on another link than the last are out of scope."""

    def __init__(self, chain, payload, force=None, moment=None, F=None, g=None, discretization_scheme=DiscretizationType.Interpolation):
        _need_chain(chain)
        _batch._need(payload, "payload", "Payload")
        super(BatchToolWrenchConstraint, self).__init__(
            chain, _box_limits(1, 6, (("force", force, 0), ("moment", moment, 3)), None, F, g), discretization_scheme,
            "tool wrench limit, %d dof" % chain.dof)
        self.payload = payload
        self.force, self.moment = force, moment

    @staticmethod
    def surface_contact_rows(mu, half_extents, normal_force_min=0.0):
        """(F [16 or 17, 6], g) of :meth:`surface_contact` on w = [fx, fy, fz, tx, ty, tz]."""
        mu, fmin = float(mu), float(normal_force_min)
        ext = np.array(half_extents, dtype=np.float64)
        if ext.shape != (2,) or not np.all(np.isfinite(ext)) or np.any(ext <= 0):
            raise ValueError("half_extents must be two finite lengths > 0, got %r" % (half_extents,))
        if not np.isfinite(mu) or mu <= 0:
            raise ValueError("mu must be finite and > 0, got %r" % (mu,))
        if not np.isfinite(fmin) or fmin < 0:
            raise ValueError("normal_force_min must be finite and >= 0, got %r" % (normal_force_min,))
        X, Y = ext
        rows = [[1, 0, -mu, 0, 0, 0], [-1, 0, -mu, 0, 0, 0], [0, 1, -mu, 0, 0, 0], [0, -1, -mu, 0, 0, 0],
                [0, 0, -Y, 1, 0, 0], [0, 0, -Y, -1, 0, 0], [0, 0, -X, 0, 1, 0], [0, 0, -X, 0, -1, 0]]
        for s1 in (1.0, -1.0):
            for s2 in (1.0, -1.0):
                rows.append([s1 * Y, s2 * X, -mu * (X + Y), s1 * mu, s2 * mu, 1.0])
                rows.append([s1 * Y, s2 * X, -mu * (X + Y), -s1 * mu, -s2 * mu, -1.0])
        g = [0.0] * 16
        if fmin > 0:
            rows.append([0, 0, -1, 0, 0, 0])
            g.append(-fmin)
        return np.array(rows, dtype=np.float64), np.array(g)

    @classmethod
    def surface_contact(cls, chain, payload, mu, half_extents, normal_force_min=0.0, **kwargs):
        """The object rests on a flat rectangular patch [-X, X] x [-Y, Y] (``half_extents`` = (X, Y)) in the contact frame's
        xy-plane, normal +z, centred at the frame's origin, with Coulomb friction ``mu`` linearised as a 4-sided pyramid at
        the corners.  The contact wrench cone in closed form, 16 rows F w <= 0 on w = [fx, fy, fz, tx, ty, tz]:
        +-fx - mu fz <= 0, +-fy - mu fz <= 0 (sliding); +-tx - Y fz <= 0, +-ty - X fz <= 0 (tipping); and for s1, s2 = +-1
        s1 Y fx + s2 X fy - mu (X + Y) fz +- (s1 mu tx + s2 mu ty + tz) <= 0 (twisting).  ``normal_force_min`` > 0 adds the
        row -fz <= -normal_force_min."""
        F, g = cls.surface_contact_rows(mu, half_extents, normal_force_min)
        return cls(chain, payload, F=F, g=g, **kwargs)

    def _terms(self, q, qs, qss):
        return self.chain.tool_wrench_terms(q, qs, qss, self.payload)


class BatchBaseWrenchConstraint(_BatchChainRows):
    """A limit on the base reaction of a robot, for a batch:  F w <= g  on  w(q, qd, qdd) = [force; moment], the wrench the
    mount exerts ON the robot -- every link of every root summed, gravity included; the moment about the origin of ``mount``'s
    frame, both parts in its axes (:meth:`toppra_amd.chain.SerialChain.base_wrench`).  It is what a pedestal, a linear axis, a
    ceiling plate or a machine frame limits at its flange, and what keeps a mobile manipulator from tipping, sliding or spinning
    on its footprint.  It is the reference's ``SecondOrderConstraint`` with an ``inv_dyn`` that returns that wrench instead of
    joint torques; the three evaluations the rows need come from one launch.

    ``robot``: a :class:`toppra_amd.chain.SerialChain` or a :class:`toppra_amd.chain.KinematicTree` (two arms on a torso: the
    reaction is the sum over both); ``mount``: a :class:`toppra_amd.chain.Mount`, None = the base frame without a platform.  The
    limits are given in one of three spellings (mixing them is a ValueError):

    ``force`` / ``moment`` (either or both): a scalar ``wmax`` (-wmax <= component <= wmax on each mount-frame axis), [3, 2] or
    [B, 3, 2] (lower, upper) -- the data-sheet box of a flange.  Each part given adds six rows, the signed identity on that part
    with g = [upper; -lower]; with both, the force's rows come first.

    ``F`` [m, 6], [B, m, 6] or [B, N+1, m, 6] with ``g`` [m], [B, m] or [B, N+1, m], as ``BatchSecondOrderConstraint`` takes
    them.

    :meth:`surface_contact`: the contact wrench cone of a flat rectangular footprint with Coulomb friction.

    The constraint is INFEASIBLE unless F w(q, 0, 0) <= g holds at every gridpoint: standing still must satisfy it (the static
    reaction carries the robot's and the platform's weight, and it enters every stage's rows).  Defaults are the reference's for
    ``SecondOrderConstraint`` (Interpolation).  Needs the path positions: a ``from_path_samples`` batch must be given ``q``.
    Per-trajectory mounts, a floating base, a true (conic) friction cone and non-rectangular footprints are out of scope."""

    def __init__(self, robot, mount=None, force=None, moment=None, F=None, g=None, discretization_scheme=DiscretizationType.Interpolation):
        _need_robot(robot)
        mount = _batch._mount(mount)
        super(BatchBaseWrenchConstraint, self).__init__(
            robot, _box_limits(1, 6, (("force", force, 0), ("moment", moment, 3)), None, F, g), discretization_scheme,
            "base wrench limit, %d dof" % robot.dof)
        self.robot, self.mount = robot, mount
        self.force, self.moment = force, moment

    @classmethod
    def surface_contact(cls, robot, mu, half_extents, mount=None, normal_force_min=0.0, **kwargs):
        """The robot (and its platform) stands on a flat rectangular footprint [-X, X] x [-Y, Y] (``half_extents`` = (X, Y)) in
        the mount frame's xy-plane, normal +z, centred at the frame's origin, with Coulomb friction ``mu``: the contact wrench
        cone of :meth:`BatchToolWrenchConstraint.surface_contact`, its rows unchanged, on the floor -> robot wrench -- no tipping
        over an edge, no sliding, no spinning."""
        F, g = BatchToolWrenchConstraint.surface_contact_rows(mu, half_extents, normal_force_min)
        return cls(robot, mount, F=F, g=g, **kwargs)

    def _terms(self, q, qs, qss):
        return self.robot.base_wrench_terms(q, qs, qss, self.mount)


class BatchJointLoadConstraint(_BatchChainRows):
    """A limit on the loads ACROSS joints of a robot, for a batch:  F w <= g  on  w(q, qd, qdd) = the wrenches of ``sections``,
    [6 S] section-major, per section [force; moment] -- what the parent side exerts ON the section's link through its joint, the
    moment about the section's origin, both parts in the section's axes, gravity included
    (:meth:`toppra_amd.chain.SerialChain.joint_wrenches`).  It is what a gearbox's output bearing (tilting moment, axial and
    radial force), a linear guide's carriage or a slender link's flange limits beside the joint's rated torque, and what a light
    arm with a heavy tool oversteps first.  It is the reference's ``SecondOrderConstraint`` with an ``inv_dyn`` that returns those
    wrenches instead of joint torques; the three evaluations the rows need come from one launch for the whole set.

    ``robot``: a :class:`toppra_amd.chain.SerialChain` or a :class:`toppra_amd.chain.KinematicTree`; ``sections``: a
    :class:`toppra_amd.chain.JointSections` (1 .. 8; several constraints may be listed).  The limits are given in one of three
    spellings (mixing them is a ValueError):

    ``force`` / ``moment`` (either or both): a scalar (-max <= component <= max on each section axis, every section), [S] (a
    magnitude per section), [S, 3, 2] or [B, S, 3, 2] (lower, upper per component).  Each part given adds six rows per section,
    the signed identity on that part with g = [upper; -lower]; the force's rows come first within a section, the sections follow
    in order.

    ``F`` [m, 6 S], [B, m, 6 S] or [B, N+1, m, 6 S] with ``g`` [m], [B, m] or [B, N+1, m], as ``BatchSecondOrderConstraint``
    takes them.

    :meth:`bearing`: a bearing's data-sheet limits -- tilting moment, axial and radial force -- as inscribed polygons.

    The constraint is INFEASIBLE unless F w(q, 0, 0) <= g holds at every gridpoint: standing still must satisfy it (the static
    load carries the weight of everything beyond the joint, and it enters every stage's rows).  Defaults are the reference's for
    ``SecondOrderConstraint`` (Interpolation).  Needs the path positions: a ``from_path_samples`` batch must be given ``q``.  The
    cap on the rows of one stage over all listed constraints applies as for every dense-row constraint (``BatchTOPPRA`` refuses a
    list above it).  True (conic) norm limits, frames fixed to the parent side of a joint and per-trajectory sections are out of
    scope."""

    def __init__(self, robot, sections, force=None, moment=None, F=None, g=None, discretization_scheme=DiscretizationType.Interpolation):
        _need_robot(robot)
        _batch._need(sections, "sections", "JointSections").on(robot)  # (a joint outside the robot: ValueError)
        super(BatchJointLoadConstraint, self).__init__(
            robot, _box_limits(sections.count, 6, (("force", force, 0), ("moment", moment, 3)), "S", F, g), discretization_scheme,
            "joint load limit, %d dof, %d sections" % (robot.dof, sections.count))
        self.robot, self.sections = robot, sections
        self.force, self.moment = force, moment

    @staticmethod
    def bearing_rows(count, tilting=None, axial=None, radial=None, sides=8):
        """(F [m, 6 count], g [m]) of :meth:`bearing`: per section, in this order, ``sides`` rows
        cos(t_j) n_x + sin(t_j) n_y <= tilting cos(pi / sides), t_j = 2 pi j / sides (when ``tilting`` is given); the same
        polygon on (f_x, f_y) for ``radial``; +f_z <= axial, -f_z <= axial.  Each limit: None, a scalar or [count], > 0."""
        count, sides = int(count), int(sides)
        if count < 1:
            raise ValueError("count must be >= 1")
        if sides < 3:
            raise ValueError("sides must be >= 3: a polygon")
        lims = {}
        for name, lim in (("tilting", tilting), ("axial", axial), ("radial", radial)):
            if lim is None:
                continue
            lim = _host(lim)
            if lim.ndim == 0:
                lim = np.full(count, float(lim))
            if lim.shape != (count,):
                raise ValueError("%s must be a scalar or have shape [S] = [%d], got %s" % (name, count, list(lim.shape)))
            if not np.all(np.isfinite(lim)) or np.any(lim <= 0):
                raise ValueError("%s must be finite and > 0" % name)
            lims[name] = lim
        if not lims:
            raise ValueError("no limit given: one of tilting, axial, radial is required")
        t = 2.0 * np.pi * np.arange(sides) / sides
        shrink = np.cos(np.pi / sides)
        F_rows, g_rows = [], []
        for k in range(count):
            for name, at in (("tilting", 3), ("radial", 0)):
                if name in lims:
                    part = np.zeros((sides, 6 * count))
                    part[:, 6 * k + at], part[:, 6 * k + at + 1] = np.cos(t), np.sin(t)
                    F_rows.append(part)
                    g_rows.append(np.full(sides, lims[name][k] * shrink))
            if "axial" in lims:
                part = np.zeros((2, 6 * count))
                part[0, 6 * k + 2], part[1, 6 * k + 2] = 1.0, -1.0
                F_rows.append(part)
                g_rows.append(np.full(2, lims["axial"][k]))
        return np.concatenate(F_rows, 0), np.concatenate(g_rows)

    @classmethod
    def bearing(cls, robot, sections, tilting=None, axial=None, radial=None, sides=8, **kwargs):
        """A bearing's data-sheet limits on every section, whose z-axis is taken as the bearing axis
        (:meth:`toppra_amd.chain.JointSections.on_axes`): the tilting moment |(n_x, n_y)| <= ``tilting`` and the radial force
        |(f_x, f_y)| <= ``radial`` as the polygon with ``sides`` sides INSCRIBED in the circle -- the rows never allow more than
        the data sheet does --, and the axial force -``axial`` <= f_z <= ``axial``.  Each limit: None, a scalar or [S].  The moment
        about the axis is the joint's torque and is left to the torque limit."""
        _batch._need(sections, "sections", "JointSections")
        F, g = cls.bearing_rows(sections.count, tilting, axial, radial, sides)
        return cls(robot, sections, F=F, g=g, **kwargs)

    def _terms(self, q, qs, qss):
        w0, wa, wb = self.robot.joint_wrench_terms(q, qs, qss, self.sections)
        flat = tuple(q.shape[:2]) + (6 * self.sections.count,)
        return w0.reshape(flat), wa.reshape(flat), wb.reshape(flat)


class BatchPointAccelerationConstraint(_BatchChainRows):
    """A limit on the accelerations of control points on ANY links of a chain, for a batch -- an elbow, a camera bracket, a
    cable carrier:  F acc <= g  on  acc(q, qd, qdd) = the linear accelerations of ``points`` in world axes, [3 P], point-major
    (:meth:`toppra_amd.chain.SerialChain.point_accelerations`; kinematics, no gravity).  It is
    :class:`BatchCartesianAccelerationConstraint` for points that need not sit on the last link; the two evaluations the rows
    need come from ONE launch of the chain kernel for the whole set, acc(q, 0, 0) is an exact zero.

    ``chain``: a :class:`toppra_amd.chain.SerialChain`; ``points``: a :class:`toppra_amd.chain.ControlPoints` (1 .. 16 points;
    several constraints may be listed).  The limits are given in one of two spellings:

    ``linear``: a scalar ``amax`` (-amax <= component <= amax on each world axis, every point), [P] (amax per point),
    [P, 3, 2] or [B, P, 3, 2] (lower, upper).  Six rows per point, the signed identity on that point's three components with
    g = [upper; -lower], the points in order.

    ``F`` [m, 3 P], [B, m, 3 P] or [B, N+1, m, 3 P] with ``g`` [m], [B, m] or [B, N+1, m], as ``BatchSecondOrderConstraint``
    takes them.

    Defaults are the reference's for ``SecondOrderConstraint`` (Interpolation).  Needs the path positions: a
    ``from_path_samples`` batch must be given ``q``.  Angular limits at interior links, a true norm (conic) limit and
    branched chains are out of scope."""

    def __init__(self, chain, points, linear=None, F=None, g=None, discretization_scheme=DiscretizationType.Interpolation):
        _need_chain(chain)
        _need_points(points, chain)
        super(BatchPointAccelerationConstraint, self).__init__(
            chain, _box_limits(points.count, 3, (("linear", linear, 0),), "P", F, g), discretization_scheme,
            "control-point acceleration limit, %d dof, %d points" % (chain.dof, points.count))
        self.points = points
        self.linear = linear

    def _terms(self, q, qs, qss):
        wa, wb = self.chain.point_acceleration_terms(q, qs, qss, self.points)
        flat = tuple(q.shape[:2]) + (3 * self.points.count,)
        return None, wa.reshape(flat), wb.reshape(flat)


# ---- batched first-order constraints: they only tighten a stage's variable box (BatchTOPPRA(..., constraints=[...])) -------

class _BatchFirstOrder(LinearConstraint):
    """Shared part of the batched constraints that produce only ``ubound`` / ``xbound``: they become bound sources of
    :func:`toppra_amd.batch.stage_boxes_batch`, folded into the stage boxes in list order on the GPU."""
    first_order = True

    def source_count(self):
        """Bound sources this constraint hands to the box kernel."""
        raise NotImplementedError

    def check(self, B, N, d):
        """Shape errors that can be told from the problem's sizes alone (ValueError), before any launch."""
        raise NotImplementedError

    def bound_sources(self, gridpoints, B, N, d, like):
        """[(kind, array)] for ``stage_boxes_batch``; arrays of the kind of ``like``."""
        raise NotImplementedError

    def compute_constraint_params(self, path, gridpoints, *args, **kwargs):
        raise NotImplementedError("%s serves BatchTOPPRA(..., constraints=[...]); a single path takes "
                                  "JointVelocityConstraintVarying or a LinearConstraint of its own" % type(self).__name__)


class BatchJointVelocityConstraintVarying(_BatchFirstOrder):
    """``JointVelocityConstraintVarying`` (linear_joint_velocity.py:56-87) for a batch: joint velocity limits that depend on
    the position along the path.

    ``vlim``: an array [B, N+1, d, 2] -- the limits of every trajectory at its gridpoints -- or a callable ``vlim_func(s)``.
    The callable is BATCHED, the convention of ``inv_dyn``: it is called ONCE, with the problem's gridpoints ([N+1], or
    [B, N+1] when they are given per trajectory; a numpy array or a torch tensor like the problem), and returns [..., d, 2].
    A 3-D array is refused: [B, d, 2] and [N+1, d, 2] cannot be told apart -- constant limits are BatchTOPPRA's ``vlim``, and
    one grid of limits for the whole batch is given as a callable or broadcast by the caller."""

    def __init__(self, vlim):
        super(BatchJointVelocityConstraintVarying, self).__init__()
        self.vlim_func = vlim if callable(vlim) else None
        self.vlim_grid = None if callable(vlim) else vlim
        if self.vlim_grid is not None:
            shape = _shape_of(self.vlim_grid)
            if len(shape) == 3:
                raise ValueError("a 3-D vlim %s is ambiguous between [B, d, 2] and [N+1, d, 2]: give [B, N+1, d, 2], or a "
                                 "callable vlim_func(s)" % (shape,))
            if len(shape) != 4 or shape[-1] != 2:
                raise ValueError("vlim must have shape [B, N+1, d, 2] or be a callable, got %s" % (shape,))
            self.dof = shape[2]
        self._format_string = "    Batched varying velocity limit\n"

    def source_count(self):
        return 1

    def check(self, B, N, d):
        if self.vlim_grid is not None and _shape_of(self.vlim_grid) != (B, N + 1, d, 2):
            raise ValueError("vlim must have shape [B, N+1, d, 2] = [%d, %d, %d, 2], got %s" % (B, N + 1, d, _shape_of(self.vlim_grid)))

    def bound_sources(self, gridpoints, B, N, d, like):
        self.check(B, N, d)
        if self.vlim_func is None:
            return [("vlim_grid", _like(self.vlim_grid, like))]
        lim = self.vlim_func(gridpoints)  # once, with every gridpoint
        want = _shape_of(gridpoints) + (d, 2)
        if not hasattr(lim, "shape") or _shape_of(lim) != want:
            raise ValueError("vlim_func(gridpoints) must return an array %s for gridpoints %s, got %s"
                             % (list(want), list(_shape_of(gridpoints)), _shape_of(lim) if hasattr(lim, "shape") else type(lim).__name__))
        return [("vlim_grid", _like(lim, like))]


class BatchBoundConstraint(_BatchFirstOrder):
    """A constraint that is only a bound on x = sd^2 and / or u = sdd at every gridpoint -- a ``LinearConstraint`` whose
    ``compute_constraint_params`` returns ``(None, None, None, None, None, ubound, xbound)``: a Cartesian tool-speed limit
    x <= v^2 / |J q'|^2, a cap on the path acceleration, a slow zone.  ``xbound``, ``ubound``: [B, N+1, 2] (lower, upper),
    or [N+1, 2] for the whole batch; either may be None.  +-inf means no bound; NaN is refused for host arrays."""

    def __init__(self, xbound=None, ubound=None):
        super(BatchBoundConstraint, self).__init__()
        if xbound is None and ubound is None:
            raise ValueError("BatchBoundConstraint needs xbound or ubound")
        for name, arr in (("xbound", xbound), ("ubound", ubound)):
            if arr is not None:
                shape = _shape_of(arr)
                if len(shape) not in (2, 3) or shape[-1] != 2:
                    raise ValueError("%s must have shape [B, N+1, 2] or [N+1, 2], got %s" % (name, shape))
        self.xbound, self.ubound = xbound, ubound
        self._format_string = "    Batched bound on the stage variables\n"

    def source_count(self):
        return (self.xbound is not None) + (self.ubound is not None)

    def check(self, B, N, d):
        for name, arr in (("xbound", self.xbound), ("ubound", self.ubound)):
            if arr is not None and _shape_of(arr) not in ((B, N + 1, 2), (N + 1, 2)):
                raise ValueError("%s must have shape [B, N+1, 2] = [%d, %d, 2] or [N+1, 2], got %s" % (name, B, N + 1, _shape_of(arr)))

    def bound_sources(self, gridpoints, B, N, d, like):
        self.check(B, N, d)
        # (the reference folds a constraint's ubound before its xbound: cy_seidel_solverwrapper.pyx:512-520)
        return [(kind, _like(arr, like)) for kind, arr in (("ubound", self.ubound), ("xbound", self.xbound)) if arr is not None]


class _BatchChainBound(_BatchFirstOrder):
    """Shared part of the first-order constraints that a chain kernel evaluates at the path positions: one ``xbound`` source
    from ``chain``, ``limit`` and the ``_limit_batch`` of a limit given per trajectory."""
    needs_q = True
    no_q = None  # the refusal of a batch without path positions

    def source_count(self):
        return 1

    def check(self, B, N, d):
        if self.dof != d:
            raise ValueError("Wrong dimension: the chain has {:d} joints, the path {:d} dof".format(self.dof, d))
        if self._limit_batch is not None and self._limit_batch != B:
            raise ValueError("limit is given per trajectory for %d trajectories, the problem has %d" % (self._limit_batch, B))

    def _limit_like(self, B, N, d, like, q):
        """The checks of a ``bound_sources`` call; the limit as an array of the kind of ``like``."""
        self.check(B, N, d)
        if q is None:
            raise ValueError(self.no_q)
        return self.limit if hasattr(self.limit, "is_cuda") and self.limit.is_cuda else _like(self.limit, like)


class BatchCartesianVelocityNormConstraint(_BatchChainBound):
    """A limit on the tool point's velocity for a batch (the C++ twin's ``CartesianVelocityNorm``,
    constraint/cartesian_velocity_norm.hpp):  v' S v * x <= limit  at every gridpoint, x = sd^2, where [v; w] are the linear
    and angular velocity of ``chain``'s tool point per unit of path velocity (qd = q'), in world axes.

    ``chain``: a :class:`toppra_amd.chain.SerialChain`; ``S``: [6, 6] symmetric positive semi-definite, None selects the linear
    part (v' S v = |v|^2).  ``limit``: > 0, a scalar or [B].  It bounds v' S v * sd^2 -- with the default ``S`` that is the SQUARE of a tool speed: a limit
    of 0.25 holds the tool to 0.5 length units per second.  The bound (0, limit / v' S v) comes from the chain kernel and is one
    ``xbound`` source of the stage boxes; where the tool stands still it is +inf and the box keeps its 1e8.  Needs the path
    positions: a ``from_path_samples`` batch must be given ``q``."""
    no_q = "a tool velocity limit evaluates the chain at q: give the path positions"

    def __init__(self, chain, limit, S=None):
        super(BatchCartesianVelocityNormConstraint, self).__init__()
        _need_chain(chain)
        self.chain, self.limit, self.S = chain, limit, S
        self.dof = chain.dof
        lshape = _shape_of(limit)
        if len(lshape) > 1:
            raise ValueError("limit must be a scalar or have shape [B], got %s" % (lshape,))
        self._limit_batch = lshape[0] if lshape else None
        if not np.all(_host(limit) > 0):
            raise ValueError("limit must be > 0 (NaN is refused; 0 / 0 at a standstill would be a NaN bound)")
        if S is not None:
            if _shape_of(S) != (6, 6):
                raise ValueError("S must have shape [6, 6], got %s" % (_shape_of(S),))
            _capi.check_weight(S)
        self._format_string = "    Batched tool velocity limit, %d dof\n" % self.dof

    def bound_sources(self, gridpoints, B, N, d, like, q=None):
        limit = self._limit_like(B, N, d, like, q)
        S = None if self.S is None else _like(self.S, like)
        return [("xbound", _batch.chain_tool_bound_batch(self.chain, q, like, limit, S)[1])]


class BatchPointSpeedConstraint(_BatchChainBound):
    """A limit on the speeds of control points on ANY links of a chain, for a batch:  |v_p|^2 * x <= limit_p  at every
    gridpoint and for every point p of ``points``, x = sd^2, where v_p is the point's velocity per unit of path velocity
    (qd = q').  It is :class:`BatchCartesianVelocityNormConstraint` (with its default ``S``) for points that need not sit on
    the last link.

    ``chain``: a :class:`toppra_amd.chain.SerialChain`; ``points``: a :class:`toppra_amd.chain.ControlPoints` (1 .. 16 points).
    ``limit``: > 0, a scalar, [P] or [B, P].  It bounds |v_p|^2 sd^2 -- it is the SQUARE of a speed, as the tool constraint's is:
    a limit of 0.25 holds a point to 0.5 length units per second.  The bound (0, min_p limit_p / |v_p|^2) comes from one launch
    of the chain kernel and is ONE ``xbound`` source of the stage boxes however many points the set has; a point that stands
    still drops out of the minimum, and where all of them do the box keeps its 1e8.  Needs the path positions: a
    ``from_path_samples`` batch must be given ``q``.  Angular and S-weighted limits stay with the tool constraint."""
    no_q = "a control-point speed limit evaluates the chain at q: give the path positions"

    def __init__(self, chain, points, limit):
        super(BatchPointSpeedConstraint, self).__init__()
        _need_chain(chain)
        _need_points(points, chain)
        self.chain, self.points, self.limit = chain, points, limit
        self.dof = chain.dof
        lshape = _shape_of(limit)
        if lshape not in ((), (points.count,)) and not (len(lshape) == 2 and lshape[1] == points.count):
            raise ValueError("limit must be a scalar or have shape [P] or [B, P] with P = %d, got %s" % (points.count, lshape))
        self._limit_batch = lshape[0] if len(lshape) == 2 else None
        if not np.all(_host(limit) > 0):
            raise ValueError("limit must be > 0 (NaN is refused; 0 / 0 at a standstill would be a NaN bound)")
        self._format_string = "    Batched control-point speed limit, %d dof, %d points\n" % (self.dof, points.count)

    def bound_sources(self, gridpoints, B, N, d, like, q=None):
        limit = self._limit_like(B, N, d, like, q)
        return [("xbound", _batch.chain_points_speed_batch(self.chain, q, like, self.points, limit)[1])]


class BatchMomentumConstraint(_BatchChainBound):
    """Limits on how much motion a robot carries, for a batch -- what a collaborative robot's safety controller caps beside
    force and point speeds:  |P| sd <= linear,  |L| sd <= angular,  1/2 q'' M(q) q' sd^2 <= energy  at every gridpoint, where
    P and L are the linear and the angular momentum per unit of path velocity (qd = q') of the links of ``links``, L about the
    origin of ``mount``'s frame (:meth:`toppra_amd.chain.SerialChain.momentum`, ``kinetic_energy``).  The kinetic energy bounds
    what the structure can transfer on contact for every contact point and direction at once.

    ``robot``: a :class:`toppra_amd.chain.SerialChain` or :class:`toppra_amd.chain.KinematicTree`; ``mount``: a
    :class:`toppra_amd.chain.Mount`, None = the base frame (its platform does not move and plays no part); ``links``: an iterable
    of link numbers, -1 = the last ("everything beyond the shoulder", "the left arm"), None = every link.

    ``linear``, ``angular``, ``energy``: each None (no limit), a scalar or [B], > 0; at least one is given.  They are in PHYSICAL
    UNITS, the way a safety configuration states them -- kg m / s, kg m^2 / s and J: ``linear=5`` holds the momentum to
    5 kg m / s.  This is unlike the speed constraints (:class:`BatchCartesianVelocityNormConstraint`,
    :class:`BatchPointSpeedConstraint`), whose ``limit`` is the SQUARE of a speed; here the class squares and doubles on the host
    (``linear * linear``, ``angular * angular``, ``2.0 * energy``) and hands the kernel what it divides.

    The bound (0, min(linear^2 / |P|^2, angular^2 / |L|^2, 2 energy / q'' M q')) comes from one launch and is ONE ``xbound`` source
    of the stage boxes; a term that vanishes drops out of the minimum, and where the robot stands still the box keeps its 1e8.
    Needs the path positions: a ``from_path_samples`` batch must be given ``q``.  The energy a contact at a given point can
    transfer -- the robot's effective mass there -- is :class:`BatchContactEnergyConstraint`; this one is its upper envelope.
    Per-trajectory robots or mounts, a floating base and power limits are out of scope."""
    no_q = "a momentum or energy limit evaluates the robot at q: give the path positions"

    def __init__(self, robot, linear=None, angular=None, energy=None, mount=None, links=None):
        super(BatchMomentumConstraint, self).__init__()
        _need_robot(robot)
        mount = _batch._mount(mount)
        if linear is None and angular is None and energy is None:
            raise ValueError("no limit given: one of linear, angular, energy is required")
        if links is not None:
            links = tuple(links) if hasattr(links, "__iter__") and not isinstance(links, (str, bytes)) else links
        _batch.link_mask(robot, links)  # (ValueError for a set that is not one of this robot's)
        self.robot, self.mount, self.links = robot, mount, links
        self.linear, self.angular, self.energy = linear, angular, energy
        self.dof = robot.dof
        self._limit_batch, parts = None, []
        for name, value, scale in (("linear", linear, None), ("angular", angular, None), ("energy", energy, 2.0)):
            if value is None:
                parts.append(np.array(np.inf))
                continue
            host = _host(value)
            if host.ndim > 1:
                raise ValueError("%s must be a scalar or have shape [B], got %s" % (name, list(host.shape)))
            if not np.all(host > 0):
                raise ValueError("%s must be > 0 (NaN is refused; 0 / 0 at a standstill would be a NaN bound)" % name)
            if host.ndim == 1:
                if self._limit_batch not in (None, host.shape[0]):
                    raise ValueError("the limits are given per trajectory for %d and %d trajectories" % (self._limit_batch, host.shape[0]))
                self._limit_batch = int(host.shape[0])
            parts.append(host * host if scale is None else scale * host)
        lead = () if self._limit_batch is None else (self._limit_batch,)
        # what the kernel divides: (p_max^2, L_max^2, 2 E_max), [3] or [B, 3]
        self.limit = np.ascontiguousarray(np.stack([np.broadcast_to(part, lead) for part in parts], -1))
        self._format_string = "    Batched momentum / kinetic-energy limit, %d dof\n" % self.dof

    def bound_sources(self, gridpoints, B, N, d, like, q=None):
        limit = self._limit_like(B, N, d, like, q)
        return [("xbound", _batch.momentum_bound_batch(self.robot, q, like, limit, self.mount, self.links))]


class BatchContactEnergyConstraint(_BatchChainBound):
    """A cap on the energy a contact at control points of a robot can transfer, for a batch -- what ISO/TS 15066 power and force
    limiting sets per body region:  1/2 mu_p v_p^2 <= energy_p  at every gridpoint and for every point p of ``points``, where v_p is
    the point's speed, mu_p = (1 / m_body + 1 / m_R)^-1 the reduced mass of the body part and the robot, and m_R the robot's
    effective (reflected) mass at the point along its velocity, 1 / m_R = u' J M(q)^-1 J' u
    (:meth:`toppra_amd.chain.SerialChain.effective_mass`, ``contact_energy``).  The total kinetic energy that
    :class:`BatchMomentumConstraint` bounds is this quantity's upper envelope: at equal ``energy`` this limit is never slower.

    ``robot``: a :class:`toppra_amd.chain.SerialChain` or :class:`toppra_amd.chain.KinematicTree`; ``points``: a
    :class:`toppra_amd.chain.ControlPoints` (1 .. 16 points on any links).  ``energy``: in J -- a scalar, [P] or [B, P], > 0.
    ``body_mass``: in kg -- a scalar or [P], > 0; None or ``inf`` = a clamped or fixed body part, 1 / m = 0.  Both are in PHYSICAL
    UNITS, as :class:`BatchMomentumConstraint`'s are (not squares): the class forms ``2.0 * energy`` and ``1.0 / body_mass`` on the
    host and hands the kernel what it multiplies and divides.  No table of body regions is shipped; :meth:`from_force` turns a
    region's force limit and stiffness into its energy.

    The bound (0, min_p 2 energy_p (1 / m_body + 1 / m_R) / |v_p|^2) comes from one launch and is ONE ``xbound`` source of the
    stage boxes however many points the set has; a point that stands still drops out of the minimum, and where all of them do
    the box keeps its 1e8.  Needs the path positions: a ``from_path_samples`` batch must be given ``q``.  A robot whose mass
    matrix is singular (a weightless leaf link) gives a non-finite bound: the caller's responsibility.  Directions in world axes,
    a true friction or conic model, per-trajectory robots, a floating base and the ISO tables of body-region limits are out of
    scope."""
    no_q = "a contact-energy limit evaluates the robot at q: give the path positions"

    def __init__(self, robot, points, energy, body_mass=None):
        super(BatchContactEnergyConstraint, self).__init__()
        _need_robot(robot)
        _need_points(points, robot)
        P = points.count
        host = _host(energy)
        if host.shape not in ((), (P,)) and not (host.ndim == 2 and host.shape[1] == P):
            raise ValueError("energy must be a scalar or have shape [P] or [B, P] with P = %d, got %s" % (P, list(host.shape)))
        if not np.all(host > 0):
            raise ValueError("energy must be > 0 (NaN is refused; 0 / 0 at a standstill would be a NaN bound)")
        inv = _contact.inverse_body_mass(body_mass, P)
        self.robot, self.points, self.energy, self.body_mass = robot, points, energy, body_mass
        self.dof = robot.dof
        self._limit_batch = int(host.shape[0]) if host.ndim == 2 else None
        lead = () if self._limit_batch is None else (self._limit_batch,)
        # what the kernel multiplies and divides: (2 E_max, 1 / m_body), [P, 2] or [B, P, 2]
        self.limit = np.ascontiguousarray(np.stack([np.broadcast_to(2.0 * host, lead + (P,)), np.broadcast_to(inv, lead + (P,))], -1))
        self._format_string = "    Batched contact-energy limit, %d dof, %d points\n" % (self.dof, P)

    @classmethod
    def from_force(cls, robot, points, force, stiffness, body_mass=None):
        """The limit a body region's force limit implies: a contact that compresses a region of stiffness k (N / m) up to the
        force F (N) has stored E = F^2 / (2 k) -- the relation ISO/TS 15066 derives its energy limits with.  ``force`` and
        ``stiffness``: each a scalar, [P] or [B, P], > 0."""
        F, k = _host(force), _host(stiffness)
        if not (np.all(F > 0) and np.all(k > 0)):
            raise ValueError("force and stiffness must be > 0 (NaN is refused)")
        return cls(robot, points, F * F / (2.0 * k), body_mass)

    def bound_sources(self, gridpoints, B, N, d, like, q=None):
        limit = self._limit_like(B, N, d, like, q)
        return [("xbound", _contact.effective_mass_bound_batch(self.robot, q, like, self.points, limit))]


class ConicConstraint(Constraint):
    """Base class of canonical conic constraints (conic_constraint.py:6-44)."""

    def __init__(self):
        self.constraint_type = ConstraintType.CanonicalConic
        self.discretization_type = DiscretizationType.Collocation
        self.n_extra_vars = 0
        self.dof = -1
        self._format_string = ""


class RobustLinearConstraint(ConicConstraint):
    """Robustified canonical linear constraint (conic_constraint.py:47-124):
    ``a u + b x + c + ||diag(ru, rx, rc) [u, x, 1]||_2 <= 0`` for every row of the base constraint.

    ``compute_constraint_params`` returns the reference's 6-tuple
    ``(a, b, c, P, ubound, xbound)``; the rows come from the HIP library.  The second-order-cone
    stage problems (ECOS in the reference) are solved exactly on the GPU by
    ``solverwrapper.hipRobustWrapper`` -- parity unpinned against ECOS, cross-checked at 1e-7 against an
    independent exact solver.
    """

    def __init__(self, cnst, ellipsoid_axes_lengths, discretization_scheme=DiscretizationType.Collocation):
        super(RobustLinearConstraint, self).__init__()
        self.dof = cnst.get_dof()
        assert getattr(cnst.get_constraint_type(), "value", None) == 0  # CanonicalLinear
        self.set_discretization_type(discretization_scheme)
        if np.any(np.r_[ellipsoid_axes_lengths] < 0):
            raise ValueError("Perturbation must be non-negative. Input {:}".format(ellipsoid_axes_lengths))
        self.base_constraint = cnst
        self.ellipsoid_axes_lengths = ellipsoid_axes_lengths
        self._format_string += "    Robust constraint generated from a canonical linear constraint\n"

    def compute_constraint_params(self, path, gridpoints):
        base = self.base_constraint
        base.set_discretization_type(self.discretization_type)  # the reference mutates the base too
        if not hasattr(base, "alim"):
            raise NotImplementedError("robustification of %s is outside the HIP path" % type(base).__name__)
        _check_dof(base, path)
        interp = self.discretization_type == DiscretizationType.Interpolation
        out = _params_on_device(path, gridpoints, alim=np.ascontiguousarray(base.alim, dtype=np.float64),
                                interpolation=interp)
        # F a, F b, F c - g are the wrapper's dense rows 2.. (cy_seidel_solverwrapper.pyx:490-499)
        a, b, c = (np.array(out[k][0][:, 2:]) for k in ("a", "b", "c"))
        rows = a.shape[1]
        P = np.zeros((len(gridpoints), rows + 2, 3, 3))
        P[:] = np.diag(self.ellipsoid_axes_lengths)
        return a, b, c, P, None, None

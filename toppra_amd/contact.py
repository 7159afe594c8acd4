"""Contact-energy limits: the effective (reflected) mass of a robot at control points, for a batch.

The entry of include/toppra_hip_contact.h, ``tpr_tree_effective_mass_batch``, and the two batch functions on it.  What a
collaborative robot's safety configuration caps per body region (ISO/TS 15066, power and force limiting) is the energy a contact
at a point of the arm can transfer, E = 1/2 mu v^2 with mu = (1 / m_body + 1 / m_R)^-1 and 1 / m_R = u' J M(q)^-1 J' u the robot's
mobility at the point along the contact direction u.  Per unit of path velocity the kernel gives, per point, the squared speed
``speed2`` and the mobility ``g = tau' M^-1 tau`` along the contact force (tau = J' f; f = the point's velocity, or a direction
given in the point's link axes), in one walk over the robot, O(d) per gridpoint; M^-1 is never formed.

The model objects are :class:`toppra_amd.chain.SerialChain` / ``KinematicTree`` and :class:`toppra_amd.chain.ControlPoints`; the
constraint is :class:`toppra_amd.constraint.BatchContactEnergyConstraint`.  No table of body regions is shipped: the caller
supplies energies (J) and body masses (kg).  A robot whose mass matrix is singular (a weightless leaf link) gives non-finite
results by IEEE rules: nothing is refused on that ground.
"""
import ctypes as C

import numpy as np

from . import _capi
from . import batch as _batch

# the entries of include/toppra_hip_contact.h (toppra_amd._capi.EXPORTS holds those of include/toppra_hip.h)
EXPORTS = ("tpr_tree_effective_mass_batch",)
_ARGTYPES = {"tpr_tree_effective_mass_batch": [C.POINTER(_capi.tpr_chain), C.c_void_p, C.POINTER(_capi.tpr_chain_points), C.c_void_p,
                                               C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]}
_declared = None


def load():
    """The library of :func:`toppra_amd._capi.load` with this header's entries declared on it (no GPU needed for this step)."""
    global _declared
    lib = _capi.load()
    if _declared is not lib:
        for name in EXPORTS:
            entry = getattr(lib, name)
            entry.restype, entry.argtypes = C.c_int, _ARGTYPES[name]
        _declared = lib
    return lib


def _directions(directions, P):
    """``directions`` as a contiguous host array [P, 3] (a device tensor is read back: 3 P doubles), None = the velocity mode."""
    if directions is None:
        return None
    if hasattr(directions, "detach"):
        directions = directions.detach().cpu().numpy()
    try:
        u = np.ascontiguousarray(np.array(directions, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("directions is not an array of numbers")
    if u.shape != (P, 3):
        raise ValueError("directions must have shape [P, 3] = [%d, 3] (unit vectors in the points' link axes), got %s" % (P, list(u.shape)))
    if not np.all(np.isfinite(u)):
        raise ValueError("directions holds a value that is not finite")
    return u


def inverse_body_mass(body_mass, P):
    """1 / m_body as a host array [P] from ``body_mass`` in kg: a scalar or [P], > 0; None or inf = a clamped or fixed body part,
    1 / m = 0.  ValueError for anything else (NaN is refused)."""
    if body_mass is None:
        return np.zeros(P)
    try:
        m = np.array(body_mass, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("body_mass is not an array of numbers")
    if m.shape not in ((), (P,)):
        raise ValueError("body_mass must be a scalar or have shape [P] = [%d], got %s" % (P, list(m.shape)))
    if not np.all(m > 0):
        raise ValueError("body_mass must be > 0 (NaN is refused; inf or None = a clamped body part)")
    return np.ascontiguousarray(np.broadcast_to(1.0 / m, (P,)))


def _call(robot, q, qs, points, limit, directions, want):
    """One call of tpr_tree_effective_mass_batch; ``want`` = which of (speed2, mobility, xbound) are asked for."""
    load()
    _batch._need(robot, "robot", "SerialChain", "KinematicTree")
    pts = _batch._control_points(robot, points)
    P = int(pts.count)
    u = _directions(directions, P)
    if qs is None and (u is None or want[0] or want[2]):
        raise ValueError("qs is required: only the mobility along given directions does without the path's first derivative")
    tails = [(P,) if want[0] else None, (P,) if want[1] else None, (2,) if want[2] else None]

    def limits(q, shape, npoints):
        more = () if qs is not None else (None,)
        if limit is None:
            return (npoints, 0), more + (None,), tails
        if len(shape) != 3:
            raise ValueError("with a limit, q must have shape [B, N+1, d], got %s" % (list(shape),))
        B, N = shape[0], shape[1] - 1
        lim = _batch._per_traj_limit("limit", limit, q, B, ((P, 2),),
                                     "have shape [P, 2] = [%d, 2] or [B, P, 2] = [%d, %d, 2] (2 E_max, 1 / m_body)" % (P, B, P))
        if isinstance(lim, np.ndarray) and not (np.all(lim[..., 0] > 0) and np.all(lim[..., 1] >= 0)):
            # (device limits are not read back: the caller's, as NaN limits are)
            raise ValueError("limit must hold 2 E_max > 0 and 1 / m_body >= 0 (a NaN bound is dropped silently by the box fold)")
        return (B, N), more + (lim,), tails

    arrays, names = ((q, qs), ("q", "qs")) if qs is not None else ((q,), ("q",))
    return _batch._rigid_call(robot, "tpr_tree_effective_mass_batch", arrays, names, None, structs=[pts], by_grid=True, limits=limits,
                              host=[u])


def effective_mass_batch(robot, q, qs, points, limit=None, directions=None):
    """What a contact at each point of ``points`` (a :class:`toppra_amd.chain.ControlPoints`, 1 .. 16 points on any links) of
    ``robot`` (a :class:`toppra_amd.chain.SerialChain` or ``KinematicTree``) meets, per unit of path velocity (qd = qs):
    ``(speed2, mobility, xbound)``, the first two of the shape of q with P in place of d, the points in their order
    (include/toppra_hip_contact.h: tpr_tree_effective_mass_batch).  numpy in -> numpy out, torch-ROCm tensors in -> tensors out on
    the current stream; views are accepted.

    Velocity mode (``directions`` None): the contact force is along the point's velocity n_p; ``speed2`` = |n_p|^2 and ``mobility``
    = g = tau' M(q)^-1 tau with tau = J_p' n_p, so the effective mass is speed2 / mobility (kg).  Direction mode (``directions``
    [P, 3]: UNIT vectors in the points' link axes, a host array): the force is along u_p; ``speed2`` = (n_p . u_p)^2 and
    ``mobility`` = u' J M^-1 J' u = 1 / m_R; ``qs`` may then be None, and ``speed2`` is None with it.

    With ``limit`` ([P, 2] or [B, P, 2] = (2 E_max, 1 / m_body): twice the energy cap in J, > 0, and the reciprocal of the body
    part's mass in 1 / kg, >= 0, 0 = a clamped body part; q must be [B, N+1, d] then) also the one bound on x = sd^2 the set
    implies: ``xbound`` [B, N+1, 2] = (0, min_p (limit_0 (limit_1 + 1 / m_R)) / speed2_p) -- +inf where every point stands still
    -- the array a ``("xbound", ...)`` source of :func:`toppra_amd.batch.stage_boxes_batch` takes; None without a limit."""
    speed2, mobility, xbound = _call(robot, q, qs, points, limit, directions, (qs is not None, True, limit is not None))
    return speed2, mobility, xbound


def effective_mass_bound_batch(robot, q, qs, points, limit):
    """``xbound`` [B, N+1, 2] of :func:`effective_mass_batch` alone (velocity mode) -- the same launch with the other two outputs
    left out, the same bits: what :class:`toppra_amd.constraint.BatchContactEnergyConstraint` hands to the stage boxes."""
    if limit is None:
        raise ValueError("the bound needs limit: [P, 2] or [B, P, 2] = (2 E_max, 1 / m_body)")
    return _call(robot, q, qs, points, limit, None, (False, False, True))[2]

"""Plain numpy reference for the momentum entry of include/toppra_hip.h (tpr_tree_momentum_batch): the linear and angular
momentum and twice the kinetic energy a set of a robot's links carries, per unit of path velocity.  Written the textbook way in
WORLD coordinates on tests/chain_ref.py's way up (``forward``: per link its world rotation R, origin p, angular velocity w and
origin velocity v) -- the kernel works in link-local frames: nothing but the model is shared.  ``dtype`` and ``absolute`` as in
tests/chain_ref.py.

A robot is a tree dict (tests/tree_ref.py), or a chain dict (tests/chain_ref.py; no "parent": the tree -1, 0, 1, ...).  A mount is
a dict: rot [3, 3] (columns = the mount frame's axes in base coordinates), origin [3] (mass and com, if any, are not read: the
platform does not move); None = the base frame.  ``links``: the link numbers of the sum, None = every link.
"""
import numpy as np

from tests.chain_ref import _add, _cross, _dot, _mtv, _mv, _scale, forward

NO_MOUNT = {"rot": np.eye(3), "origin": np.zeros(3)}


def link_set(robot, links=None):
    """The sorted link numbers of a link set on a robot dict: None = all, negative numbers count from the end."""
    d = len(robot["joint_type"])
    return list(range(d)) if links is None else sorted(set(int(i) % d for i in links))


def _sums(robot, q, qd, mount, links, dtype, absolute):
    mount = NO_MOUNT if mount is None else mount
    state, ar = forward(robot, q, qd, None, dtype, absolute)
    mass = np.asarray(robot["mass"], dtype=dtype)
    P, L, T2 = [ar.zero] * 3, [ar.zero] * 3, ar.zero
    for i in link_set(robot, links):
        K = state[i]
        c = _mv(K["R"], ar.vec(robot["com"][i]))
        inertia = ar.inertia(K["R"], robot["inertia"][i])
        m = ar.wrap(mass[i])
        vc = _add(K["v"], _cross(K["w"], c))
        h, Iw = _scale(vc, m), inertia(K["w"])
        P = _add(P, h)
        L = _add(L, _add(Iw, _cross(_add(K["p"], c), h)))
        T2 = T2 + (m * _dot(vc, vc) + _dot(K["w"], Iw))
    Rm = ar.mat(mount["rot"])
    shift = _cross(ar.vec(mount["origin"]), P)
    return ar, _mtv(Rm, P) + _mtv(Rm, [L[k] - shift[k] for k in range(3)]), T2


def momentum(robot, q, qd, mount=None, links=None, dtype=np.float64, absolute=False):
    """[..., 6] = [linear; angular about the mount's origin] in mount-frame axes for joint velocities qd; arrays [..., d]."""
    ar, h, _ = _sums(robot, q, qd, mount, links, dtype, absolute)
    return ar.stack(h)


def energy2(robot, q, qd, mount=None, links=None, dtype=np.float64, absolute=False):
    """[...] = qd' M(q) qd of the link set: twice its kinetic energy (``mount`` plays no part: one signature for both)."""
    ar, _, T2 = _sums(robot, q, qd, mount, links, dtype, absolute)
    return ar.stack([T2])[..., 0]


def xbound(momentum6, e2, limit):
    """The bound on x = sd^2 of the header, made on the host from an entry's outputs [B, N+1, 6], [B, N+1] and limit [B, 3] =
    (p_max^2, L_max^2, 2 E_max): IEEE divisions, |a|^2 = (a_x a_x + a_y a_y) + a_z a_z; [B, N+1, 2] = (0, the minimum)."""
    h, lim = np.asarray(momentum6), np.broadcast_to(np.asarray(limit, dtype=np.float64), (np.shape(momentum6)[0], 3))
    pp = (h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1]) + h[..., 2] * h[..., 2]
    ll = (h[..., 3] * h[..., 3] + h[..., 4] * h[..., 4]) + h[..., 5] * h[..., 5]
    with np.errstate(divide="ignore"):
        best = np.minimum(np.minimum(lim[:, None, 0] / pp, lim[:, None, 1] / ll), lim[:, None, 2] / np.asarray(e2))
    return np.stack([np.zeros_like(best), best], -1)


def xbound_tolerance(momentum6, momentum_mag, e2, e2_mag, limit, bound_m, bound_e):
    """How far the upper bound of :func:`xbound` may move, [B, N+1], when ``momentum6`` and ``e2`` are each known to their accuracy
    bound: |error| <= bound x the all-absolute magnitude, composed through the division.  Per term a_k = limit_k / s_k with
    |ds_k| <= e_k (s = |P|^2, |L|^2: e = sum_j 2 |h_j| dh_j + dh_j^2; s = e2: e = de2) the quotient moves by at most
    da_k = a_k e_k / (s_k - e_k); the minimum of the three moves by at most the largest da_k among the terms that can be the
    minimum at all -- those with a_k - da_k <= min_j (a_j + da_j): the reference's own smallest term is one of them, and so is
    whichever term is smallest after the disturbance.  A term that is switched off (+inf) or stands still (s = 0: +inf on both
    sides, the magnitude is zero there too) moves by nothing.  Plus 4 ulp of the value for the division itself."""
    h, hm = np.asarray(momentum6, dtype=np.float64), np.asarray(momentum_mag, dtype=np.float64)
    lim = np.broadcast_to(np.asarray(limit, dtype=np.float64), (h.shape[0], 3))
    dh = bound_m * hm
    parts = [((h[..., k:k + 3] ** 2).sum(-1), (2.0 * np.abs(h[..., k:k + 3]) * dh[..., k:k + 3] + dh[..., k:k + 3] ** 2).sum(-1)) for k in (0, 3)]
    parts.append((np.asarray(e2, dtype=np.float64), bound_e * np.asarray(e2_mag, dtype=np.float64)))
    a, da = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, (s, e) in enumerate(parts):
            ak = lim[:, None, k] / s
            live = np.isfinite(ak) & (e > 0)
            assert np.all(s[live] > e[live]), "a term's error reaches its value: the quotient is not bounded"
            a.append(ak)
            da.append(np.where(live, ak * e / np.where(live, s - e, 1.0), 0.0))
    a, da = np.stack(a), np.stack(da)
    with np.errstate(invalid="ignore"):
        can_win = (a - da) <= np.min(a + da, 0)
    best = np.min(a, 0)
    return np.max(np.where(can_win, da, 0.0), 0) + 4 * np.finfo(float).eps * np.where(np.isfinite(best), best, 0.0)

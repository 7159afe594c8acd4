"""Plain numpy references for the effective-mass entry of include/toppra_hip_contact.h (tpr_tree_effective_mass_batch): the squared
speed s2 of control points per unit of path velocity and the robot's mobility g = tau' M(q)^-1 tau along the contact force there.

Two routes that share nothing but the model:

``walk``    a restatement of the kernel's walk in the kernel's frames (link axes, spatial vectors (angular; linear) about the link's
            origin): the way up for v, w, the way down for the articulated inertias IA, U = IA S, D = S' U and every point's bias
            wrench.  Written with 6 x 6 matrices and numpy products, so its rounding is its own.  ``dtype``: float64 or longdouble.
``dense``   the textbook route in WORLD coordinates: the mass matrix from tests/chain_ref.py's ``mass_matrix`` (columns of inverse
            dynamics), the point's Jacobian columns from its ``forward``, and ``np.linalg.solve``.  float64 only.

A robot is a chain dict or a tree dict (tests/chain_ref.py, tests/tree_ref.py).  ``links`` [P] and ``offsets`` [P, 3] are the
points; ``directions`` [P, 3] (link axes, unit) selects the direction mode, None the velocity mode.  Both return
(speed2, mobility), each [..., P].
"""
import numpy as np

from tests import chain_ref
from tests.chain_ref import parents_of


def _skew(r):
    """[r]x of r [..., 3]: [..., 3, 3]."""
    z = np.zeros_like(r[..., 0])
    return np.stack([np.stack([z, -r[..., 2], r[..., 1]], -1), np.stack([r[..., 2], z, -r[..., 0]], -1),
                     np.stack([-r[..., 1], r[..., 0], z], -1)], -2)


def _frames(robot, q, dtype):
    """Per link (E, r): the link frame's axes in parent coordinates as columns [..., 3, 3] and its origin there [..., 3]."""
    q = np.asarray(q, dtype=dtype)
    out = []
    for i in range(q.shape[-1]):
        k = np.asarray(robot["axis"][i], dtype=dtype)
        rot, trans = np.asarray(robot["rot"][i], dtype=dtype), np.asarray(robot["trans"][i], dtype=dtype)
        qi = q[..., i]
        if int(robot["joint_type"][i]) == 1:
            E = np.broadcast_to(rot, qi.shape + (3, 3))
            r = trans + (rot @ k) * qi[..., None]
        else:
            s, c = np.sin(qi)[..., None, None], np.cos(qi)[..., None, None]
            R = c * np.eye(3, dtype=dtype) + s * _skew(k) + (1 - c) * np.outer(k, k)
            E = rot @ R
            r = np.broadcast_to(trans, qi.shape + (3,))
        out.append((E, r))
    return out


def _motion_axis(robot, i, dtype):
    z = np.asarray(robot["axis"][i], dtype=dtype)
    zero = np.zeros(3, dtype=dtype)
    return np.concatenate([zero, z]) if int(robot["joint_type"][i]) == 1 else np.concatenate([z, zero])


def _body_inertia(robot, i, dtype):
    """The link's own spatial inertia about its origin, link axes: [[Ic + m (c.c 1 - c c'), m [c]x], [(m [c]x)', m 1]]."""
    m, c = np.asarray(robot["mass"], dtype=dtype)[i], np.asarray(robot["com"][i], dtype=dtype)
    I = np.asarray(robot["inertia"][i], dtype=dtype)
    Ic = np.array([[I[0], I[3], I[4]], [I[3], I[1], I[5]], [I[4], I[5], I[2]]], dtype=dtype)
    H = m * _skew(c)
    top = np.concatenate([Ic + m * (np.dot(c, c) * np.eye(3, dtype=dtype) - np.outer(c, c)), H], -1)
    return np.concatenate([top, np.concatenate([H.T, m * np.eye(3, dtype=dtype)], -1)], -2)


def _to_parent(E, r):
    """Xf [..., 6, 6]: a wrench (n; f) of a link, in its axes about its origin, as its parent sees it: (E n + r x E f; E f)."""
    top = np.concatenate([E, _skew(r) @ E], -1)
    return np.concatenate([top, np.concatenate([np.zeros_like(E), E], -1)], -2)


def walk(robot, links, offsets, q, qs, directions=None, dtype=np.float64):
    """(speed2, mobility) [..., P] by the kernel's walk; qs may be None in the direction mode (speed2 is None then)."""
    q = np.asarray(q, dtype=dtype)
    lead, d = q.shape[:-1], q.shape[-1]
    parents, frames = parents_of(robot), _frames(robot, q, dtype)
    offsets = np.asarray(offsets, dtype=dtype)
    P = len(links)
    on_path = [[] for _ in range(d)]  # the points whose path to the root passes link i
    for p, k in enumerate(links):
        i = int(k)
        while i >= 0:
            on_path[i].append(p)
            i = parents[i]
    f, s2 = [None] * P, [None] * P
    if qs is not None:  # the way up
        qs = np.asarray(qs, dtype=dtype)
        vel = []
        for i in range(d):
            E, r = frames[i]
            v, w = (np.zeros(lead + (3,), dtype=dtype),) * 2 if parents[i] < 0 else vel[parents[i]]
            S = _motion_axis(robot, i, dtype)
            Et = np.swapaxes(E, -1, -2)
            vel.append(((Et @ (v + np.cross(w, r))[..., None])[..., 0] + S[3:] * qs[..., i, None],
                        (Et @ w[..., None])[..., 0] + S[:3] * qs[..., i, None]))
        for p, k in enumerate(links):
            v, w = vel[int(k)]
            n = v + np.cross(w, offsets[p])
            if directions is None:
                f[p], s2[p] = n, (n * n).sum(-1)
            else:
                u = np.asarray(directions[p], dtype=dtype)
                f[p], s2[p] = np.broadcast_to(u, lead + (3,)), (n * u).sum(-1) ** 2
    else:
        assert directions is not None, "the velocity mode needs qs"
        for p in range(P):
            f[p] = np.broadcast_to(np.asarray(directions[p], dtype=dtype), lead + (3,))
    # the way down
    handed = [None] * d
    b, g = [None] * P, [np.zeros(lead, dtype=dtype) for _ in range(P)]
    for i in range(d - 1, -1, -1):
        IA = np.broadcast_to(_body_inertia(robot, i, dtype), lead + (6, 6))
        if handed[i] is not None:
            IA = IA + handed[i]
        S = _motion_axis(robot, i, dtype)
        U = IA @ S
        D = U @ S
        E, r = frames[i]
        X = _to_parent(E, r)
        for p in on_path[i]:
            if int(links[p]) == i:
                b[p] = -np.concatenate([np.cross(offsets[p], f[p]), f[p]], -1)
            u = -(b[p] @ S)
            g[p] = g[p] + u * u / D
            b[p] = (X @ (b[p] + U * (u / D)[..., None])[..., None])[..., 0]
        if parents[i] >= 0:
            Ia = IA - U[..., :, None] * U[..., None, :] / D[..., None, None]
            give = X @ Ia @ np.swapaxes(X, -1, -2)
            handed[parents[i]] = give if handed[parents[i]] is None else handed[parents[i]] + give
    return (None if qs is None else np.stack(s2, -1)), np.stack(g, -1)


def point_velocities(robot, links, offsets, q, qs, dtype=np.float64):
    """n_p [..., P, 3]: the points' velocities per unit of path velocity in their links' axes, by the dense route's Jacobians
    rotated back into link axes."""
    J, Rs = jacobians(robot, links, offsets, q)
    n = (J @ np.asarray(qs, dtype=np.float64)[..., None, :, None])[..., 0]
    return np.stack([(np.swapaxes(Rs[p], -1, -2) @ n[..., p, :, None])[..., 0] for p in range(len(links))], -2).astype(dtype)


def jacobians(robot, links, offsets, q):
    """The points' world-frame Jacobians [..., P, 3, d] and their links' world rotations [P][..., 3, 3], float64."""
    q = np.asarray(q, dtype=np.float64)
    state, _ = chain_ref.forward(robot, q, np.zeros_like(q))
    parents = parents_of(robot)
    vec = lambda a: np.stack(a, -1)  # noqa: E731
    mat = lambda R: np.stack([np.stack(row, -1) for row in R], -2)  # noqa: E731
    Js, Rs = [], []
    for p, k in enumerate(links):
        k = int(k)
        Rk = mat(state[k]["R"])
        x = vec(state[k]["p"]) + (Rk @ np.asarray(offsets[p], dtype=np.float64)[..., None])[..., 0]
        J = np.zeros(q.shape[:-1] + (3, q.shape[-1]))
        i = k
        while i >= 0:
            z = vec(state[i]["z"])
            J[..., :, i] = z if state[i]["prismatic"] else np.cross(z, x - vec(state[i]["p"]))
            i = parents[i]
        Js.append(J)
        Rs.append(Rk)
    return np.stack(Js, -3), Rs


def mass_matrix(robot, q):
    """M(q) [..., d, d] of tests/chain_ref.py on the robot without gravity (M does not depend on it; with it every column would be
    a difference of two torques that both carry the weight)."""
    return chain_ref.mass_matrix(dict(robot, gravity=np.zeros(3)), q)


def dense(robot, links, offsets, q, qs, directions=None):
    """(speed2, mobility) [..., P] by the dense route: tau = J' f, g = tau' solve(M, tau)."""
    q = np.asarray(q, dtype=np.float64)
    M = mass_matrix(robot, q)
    J, Rs = jacobians(robot, links, offsets, q)
    s2, g = [], []
    for p in range(len(links)):
        n = None if qs is None else (J[..., p, :, :] @ np.asarray(qs, dtype=np.float64)[..., None])[..., 0]
        if directions is None:
            f, s = n, (n * n).sum(-1)
        else:
            f = (Rs[p] @ np.asarray(directions[p], dtype=np.float64)[..., None])[..., 0]
            s = None if n is None else (n * f).sum(-1) ** 2
        tau = (np.swapaxes(J[..., p, :, :], -1, -2) @ f[..., None])[..., 0]
        g.append((tau * np.linalg.solve(M, tau[..., None])[..., 0]).sum(-1))
        s2.append(s)
    return (None if qs is None else np.stack(s2, -1)), np.stack(g, -1)


def energy2(robot, q, qs):
    """qs' M(q) qs by the dense route, [...]: what the Cauchy-Schwarz check s2^2 <= g * energy2 compares with."""
    q, qs = np.asarray(q, dtype=np.float64), np.asarray(qs, dtype=np.float64)
    return (qs * (mass_matrix(robot, q) @ qs[..., None])[..., 0]).sum(-1)


def xbound(speed2, mobility, limit, directed=False):
    """The bound on x = sd^2 of the header, made on the host from an entry's outputs [B, N+1, P] and limit [B, P, 2] =
    (2 E_max, 1 / m_body): x_p = (limit_0 (limit_1 + winv)) / s2_p, winv = g_p / s2_p (g_p in the direction mode), +inf where
    s2_p == 0; the minimum from +inf with ``<`` in the set's order.  [B, N+1, 2] = (0, the minimum)."""
    s2, g = np.asarray(speed2, dtype=np.float64), np.asarray(mobility, dtype=np.float64)
    lim = np.broadcast_to(np.asarray(limit, dtype=np.float64), (s2.shape[0], s2.shape[-1], 2))
    best = np.full(s2.shape[:-1], np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(s2.shape[-1]):
            winv = g[..., p] if directed else g[..., p] / s2[..., p]
            x = (lim[:, None, p, 0] * (lim[:, None, p, 1] + winv)) / s2[..., p]
            x = np.where(s2[..., p] == 0.0, np.inf, x)
            best = np.where(x < best, x, best)
    return np.stack([np.zeros_like(best), best], -1)


def xbound_tolerance(speed2, mobility, limit, bound_s2, bound_g):
    """How far the upper bound of :func:`xbound` (velocity mode) may move, [B, N+1], when ``speed2`` and ``mobility`` are each known
    to their RELATIVE accuracy bound.  Per point x_p = l0 l1 / s2 + l0 g / s2^2: with s2 within (1 +- bs) and g within (1 +- bg) of
    their values the two terms move by at most  l0 l1 / s2 * bs / (1 - bs)  and  l0 g / s2^2 * ((1 + bg) / (1 - bs)^2 - 1).  The
    minimum over the points moves by at most the largest such dx_p among the points that can be the minimum at all -- those with
    x_p - dx_p <= min_j (x_j + dx_j).  A point that stands still (s2 = 0: +inf on both sides) moves by nothing.  Plus 8 ulp of the
    value for the divisions, the product and the sum themselves."""
    s2, g = np.asarray(speed2, dtype=np.float64), np.asarray(mobility, dtype=np.float64)
    lim = np.broadcast_to(np.asarray(limit, dtype=np.float64), (s2.shape[0], s2.shape[-1], 2))
    l0, l1 = lim[:, None, :, 0], lim[:, None, :, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(s2 == 0, np.inf, (l0 * (l1 + g / s2)) / s2)
        dx = np.where(s2 == 0, 0.0, l0 * l1 / s2 * (bound_s2 / (1 - bound_s2)) + l0 * g / (s2 * s2) * ((1 + bound_g) / (1 - bound_s2) ** 2 - 1))
        can_win = (x - dx) <= np.min(x + dx, -1, keepdims=True)
    best = np.min(x, -1)
    return np.max(np.where(can_win, dx, 0.0), -1) + 8 * np.finfo(float).eps * np.where(np.isfinite(best), best, 0.0)

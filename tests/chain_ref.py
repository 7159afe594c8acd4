"""Plain numpy reference for the serial chain of include/toppra_hip.h (tpr_chain): recursive Newton-Euler inverse dynamics and
the tool point's velocity, written from the textbook recursion in WORLD coordinates (the kernels work in link-local frames:
nothing but the model is shared).  Every function takes ``dtype`` and runs in np.longdouble as well, and ``absolute=True``
evaluates the same expression with every product and sum taken in absolute value -- the magnitude against which the GPU
tests measure an error.

The recursion exists once, here: ``forward`` (the way up, over a parent table: the chain is the tree -1, 0, 1, ...) and
``backward`` (the way down).  tests/tree_ref.py, tool_accel_ref.py, tool_wrench_ref.py, base_wrench_ref.py and joint_load_ref.py
add only what is their own to it, so one correction reaches every accuracy bound of the family.

A chain is a dict: joint_type [d] (0 revolute, 1 prismatic), axis [d, 3], rot [d, 3, 3], trans [d, 3], mass [d], com [d, 3],
inertia [d, 6] = xx, yy, zz, xy, xz, yz, gravity [3], tool [3].
"""
import numpy as np


class _Mag(object):
    """A non-negative array under an arithmetic in which nothing cancels: a + b, a - b -> |a| + |b|, a * b -> |a| |b|."""
    __array_priority__ = 1000

    def __init__(self, v):
        self.v = np.abs(v)

    @staticmethod
    def _of(x):
        return x.v if isinstance(x, _Mag) else np.abs(x)

    def __add__(self, o):
        return _Mag(self.v + _Mag._of(o))
    __radd__ = __sub__ = __rsub__ = __add__

    def __mul__(self, o):
        return _Mag(self.v * _Mag._of(o))
    __rmul__ = __mul__

    def __neg__(self):
        return self


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _add(a, b):
    return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]


def _scale(a, s):
    return [a[0] * s, a[1] * s, a[2] * s]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _mv(M, v):
    return [_dot(M[r], v) for r in range(3)]


def _mtv(M, v):
    return [M[0][c] * v[0] + M[1][c] * v[1] + M[2][c] * v[2] for c in range(3)]


def _mm(A, B):
    return [[A[r][0] * B[0][c] + A[r][1] * B[1][c] + A[r][2] * B[2][c] for c in range(3)] for r in range(3)]


def _rodrigues(k, s, c):
    t = 1 - c
    return [[c + t * k[0] * k[0], t * k[0] * k[1] - s * k[2], t * k[0] * k[2] + s * k[1]],
            [t * k[0] * k[1] + s * k[2], c + t * k[1] * k[1], t * k[1] * k[2] - s * k[0]],
            [t * k[0] * k[2] - s * k[1], t * k[1] * k[2] + s * k[0], c + t * k[2] * k[2]]]


class _Arith(object):
    """The arithmetic of one evaluation over the leading shape ``lead``: ``dtype``, and plain or (``absolute``) nothing-cancels."""

    def __init__(self, lead, dtype, absolute):
        self.dtype, self.absolute = dtype, absolute
        self.wrap = (lambda x: _Mag(x)) if absolute else (lambda x: x)
        self.one, self.zero = self.wrap(np.ones(lead, dtype=dtype)), self.wrap(np.zeros(lead, dtype=dtype))

    def scalar(self, x):
        return self.wrap(np.asarray(x, dtype=self.dtype)) * self.one

    def vec(self, x):
        x = np.asarray(x, dtype=self.dtype)
        return [self.wrap(x[j]) * self.one for j in range(3)]

    def mat(self, M):
        M = np.asarray(M, dtype=self.dtype)
        return [[self.wrap(M[r, c]) * self.one for c in range(3)] for r in range(3)]

    def inertia(self, R, I):
        """x -> R I R' x for I = xx, yy, zz, xy, xz, yz in the frame R."""
        I = [self.wrap(x) for x in np.asarray(I, dtype=self.dtype)]
        Il = [[I[0], I[3], I[4]], [I[3], I[1], I[5]], [I[4], I[5], I[2]]]
        return lambda x: _mv(R, _mv(Il, _mtv(R, x)))

    def stack(self, parts):
        return np.stack([t.v if self.absolute else t for t in parts], -1)


def parents_of(robot):
    """The parent table of a robot dict: a tree's own, the chain's -1, 0, 1, ..."""
    return [int(p) for p in robot["parent"]] if "parent" in robot else list(range(-1, len(robot["joint_type"]) - 1))


def forward(robot, q, qd, qdd=None, dtype=np.float64, absolute=False, dynamics=False):
    """The way up in world coordinates, over the robot's parent table; arrays [..., d], qdd None = zero.  Returns (links, ar):
    per link its parent, rotation R, origin p, axis z, angular velocity w, origin velocity v, angular acceleration wd, origin
    acceleration a (the base accelerates by -gravity) and prismatic; with ``dynamics`` also the inertial force F on the link, the
    inertial moment N about its centre of mass and that centre c from the link's origin.  ``ar`` is the evaluation's _Arith."""
    qa, qda = np.asarray(q, dtype=dtype), np.asarray(qd, dtype=dtype)
    qdda = np.zeros_like(qa) if qdd is None else np.asarray(qdd, dtype=dtype)
    ar = _Arith(qa.shape[:-1], dtype, absolute)
    wrap, one, zero = ar.wrap, ar.one, ar.zero
    gravity = np.asarray(robot["gravity"], dtype=dtype)
    base = {"R": [[one if r == c else zero for c in range(3)] for r in range(3)], "p": [zero] * 3, "w": [zero] * 3, "v": [zero] * 3,
            "wd": [zero] * 3, "a": [zero - wrap(gravity[k]) * one for k in range(3)]}
    links = []
    for i, parent in enumerate(parents_of(robot)):
        assert -1 <= parent < i, (i, parent)
        up = base if parent < 0 else links[parent]
        R, w, wd, a = up["R"], up["w"], up["wd"], up["a"]
        qi, qdi, qddi = wrap(qa[..., i]), wrap(qda[..., i]), wrap(qdda[..., i])
        k = ar.vec(robot["axis"][i])
        Rj = _mm(R, ar.mat(robot["rot"][i]))
        z = _mv(Rj, k)
        r = _mv(R, ar.vec(robot["trans"][i]))
        prismatic = int(robot["joint_type"][i]) == 1
        if prismatic:
            Rl = Rj
            r = _add(r, _scale(z, qi))
        else:
            Rl = _mm(Rj, _rodrigues(k, wrap(np.sin(qa[..., i])), wrap(np.cos(qa[..., i]))))
        v_new = _add(up["v"], _cross(w, r))
        a_new = _add(_add(a, _cross(wd, r)), _cross(w, _cross(w, r)))
        if prismatic:
            v_new = _add(v_new, _scale(z, qdi))
            w_new, wd_new = w, wd
            a_new = _add(_add(a_new, _scale(z, qddi)), _scale(_cross(w, z), 2 * qdi))
        else:
            w_new = _add(w, _scale(z, qdi))
            wd_new = _add(_add(wd, _scale(z, qddi)), _scale(_cross(w, z), qdi))
        L = {"parent": parent, "R": Rl, "p": _add(up["p"], r), "z": z, "w": w_new, "v": v_new, "wd": wd_new, "a": a_new,
             "prismatic": prismatic}
        if dynamics:
            com = _mv(Rl, ar.vec(robot["com"][i]))
            ac = _add(_add(a_new, _cross(wd_new, com)), _cross(w_new, _cross(w_new, com)))
            inertia = ar.inertia(Rl, robot["inertia"][i])
            L["F"] = _scale(ac, wrap(np.asarray(robot["mass"], dtype=dtype)[i]))
            L["N"] = _add(inertia(wd_new), _cross(w_new, inertia(w_new)))
            L["c"] = com
        links.append(L)
    return links, ar


def backward(links, ar):
    """The way down: per link the (f, n) its parent exerts on it through its joint, in world axes, n about the link's own origin.
    A link hands (f, n about the parent's origin) down; a parent adds its children in descending child number."""
    d = len(links)
    handed, out = [None] * d, [None] * d
    for i in range(d - 1, -1, -1):
        L = links[i]
        f, n = handed[i] if handed[i] is not None else ([ar.zero] * 3, [ar.zero] * 3)
        f = _add(L["F"], f)
        n = _add(_add(L["N"], _cross(L["c"], L["F"])), n)
        out[i] = (f, n)
        p = L["parent"]
        if p >= 0:
            lever = [L["p"][k] - links[p]["p"][k] for k in range(3)]
            give = (f, _add(n, _cross(lever, f)))
            handed[p] = give if handed[p] is None else (_add(handed[p][0], give[0]), _add(handed[p][1], give[1]))
    return out


def rnea(robot, q, qd, qdd, dtype=np.float64, absolute=False):
    """tau(q, qd, qdd), arrays [..., d]; a chain or a tree dict."""
    links, ar = forward(robot, q, qd, qdd, dtype, absolute, dynamics=True)
    return ar.stack([_dot(L["z"], f) if L["prismatic"] else _dot(L["z"], n) for L, (f, n) in zip(links, backward(links, ar))])


def tool_velocity(chain, q, qd, dtype=np.float64, absolute=False):
    """(v, w) [..., 3] each: the tool point's linear and angular velocity in world axes for joint velocities qd."""
    links, ar = forward(chain, q, qd, None, dtype, absolute)
    L = links[-1]
    v = _add(L["v"], _cross(L["w"], _mv(L["R"], ar.vec(chain["tool"]))))
    return v, L["w"]


def tool_vsv(chain, q, qd, S=None, dtype=np.float64, absolute=False):
    """[v; w]' S [v; w] of the tool point, shape [...]; S None = v' v."""
    v, w = tool_velocity(chain, q, qd, dtype, absolute)
    if S is None:
        out = _dot(v, v)
    else:
        x = v + w
        S = np.asarray(S, dtype=dtype)
        wrap = (lambda y: _Mag(y)) if absolute else (lambda y: y)
        out = None
        for r in range(6):
            row = None
            for c in range(6):
                term = wrap(S[r, c]) * x[c]
                row = term if row is None else row + term
            out = x[r] * row if out is None else out + x[r] * row
    return out.v if absolute else out


def mass_matrix(chain, q, dtype=np.float64):
    """M(q) [..., d, d] from columns tau(q, 0, e_j) - tau(q, 0, 0)."""
    q = np.asarray(q, dtype=dtype)
    d = q.shape[-1]
    zero = np.zeros_like(q)
    base = rnea(chain, q, zero, zero, dtype)
    cols = []
    for j in range(d):
        e = np.zeros_like(q)
        e[..., j] = 1
        cols.append(rnea(chain, q, zero, e, dtype) - base)
    return np.stack(cols, -1)


def random_rotation(rng):
    A = rng.standard_normal((3, 3))
    Q, _ = np.linalg.qr(A)
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    # one Newton step towards the nearest orthonormal matrix: orthonormal to rounding
    return 0.5 * (Q + np.linalg.inv(Q).T)


def random_chain(d, seed, gravity=True, massless=None, prismatic_every=3):
    """A chain with mixed joint types, tilted axes, rotated joint frames, offsets, full inertias; link ``massless`` weighs
    nothing.  The inertias are positive definite (A A' + a multiple of the identity)."""
    rng = np.random.default_rng(seed)
    types = np.array([1 if (prismatic_every and i % prismatic_every == 1) else 0 for i in range(d)], dtype=np.int32)
    axis = rng.standard_normal((d, 3))
    axis /= np.sqrt((axis ** 2).sum(-1, keepdims=True))
    axis /= np.sqrt((axis ** 2).sum(-1, keepdims=True))
    rot = np.stack([random_rotation(rng) for _ in range(d)])
    trans = rng.uniform(-0.3, 0.3, (d, 3))
    mass = rng.uniform(0.5, 3.0, d)
    com = rng.uniform(-0.1, 0.1, (d, 3))
    A = rng.uniform(-0.1, 0.1, (d, 3, 3))
    full = A @ np.swapaxes(A, 1, 2) + 0.01 * np.eye(3)
    inertia = np.stack([full[:, 0, 0], full[:, 1, 1], full[:, 2, 2], full[:, 0, 1], full[:, 0, 2], full[:, 1, 2]], -1)
    if massless is not None and massless < d:
        mass[massless] = 0.0
        inertia[massless] = 0.0
    return {"joint_type": types, "axis": axis, "rot": rot, "trans": trans, "mass": mass, "com": com, "inertia": inertia,
            "gravity": np.array([0.3, -0.2, -9.81]) if gravity else np.zeros(3), "tool": rng.uniform(-0.2, 0.2, 3)}


def serial_chain(chain):
    """The toppra_amd.chain.SerialChain of a chain dict."""
    from toppra_amd.chain import SerialChain
    return SerialChain(chain["joint_type"], chain["axis"], chain["rot"], chain["trans"], chain["mass"], chain["com"],
                       chain["inertia"], gravity=chain["gravity"], tool=chain["tool"])

"""What the control-point tests share: the point sets on the chains of tests/chain_cases.py, the chain cut after a point's link
(the yardstick of the bit-for-bit tests: the existing tool kernels run on it), the float64 references and the accuracy bound.

Point sets (the issue's): "a" one point on link 0; "b" three points, two on one middle link and one on the last link (given as
-1) at the chain's own tool -- listed middle, last, middle, so that the outputs' order is not the links' order; "c" sixteen
points spread over the links in a shuffled order (at 32 dof, where the acceleration kernels stage the links in several passes,
and at 1 dof, where the output area is many times the input area); "d" at 9 dof, the deepest point on link 2: the recursion
stops early.

The bound is that of tests/chain_cases.py, by its method and with its factor: the metric is |got - ref| / (the reference
evaluated with every product and sum in absolute value), the yardstick is the error the float64 reference itself shows against
the same recursion in np.longdouble on these very inputs, per case, point set and quantity, and the bound is BOUND_FACTOR (16)
times that.  The quantities: "speed2" (the squared speed for qd = q'), "wa" = acc(q, 0, q'), "wb" = acc(q, q', q'') (the single
evaluation's reference too), stacked over the points of the set.
"""
import functools

import numpy as np

from tests import chain_cases as cc, chain_ref, tool_accel_ref

DOFS, B, N, BOUND_FACTOR = cc.DOFS, cc.B, cc.N, cc.BOUND_FACTOR
LINK_KEYS = ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia")


def point_set(d, which, chain=None):
    """(links [P] with -1 for the last link, offsets [P, 3]) of set ``which`` on the dof-d case."""
    chain = cc.case(d)[0] if chain is None else chain
    rng = np.random.default_rng(300 + 7 * d + ord(which))
    if which == "a":
        links = [0]
    elif which == "b":
        mid = (d - 1) // 2
        links = [mid, -1, mid]
    elif which == "c":
        links = list(rng.permutation(np.round(np.linspace(0, d - 1, 16)).astype(int)))
    elif which == "d":
        links = [1, 2, 0, 2]
    else:
        raise KeyError(which)
    offsets = rng.uniform(-0.25, 0.25, (len(links), 3))
    if which == "b":
        offsets[1] = chain["tool"]
    return np.array(links, dtype=np.int64), offsets


# every (dof, set) the GPU tests run
CASES = tuple((d, w) for d in DOFS for w in "ab") + ((32, "c"), (1, "c"), (9, "d"))


def ControlPoints(links, offsets):
    from toppra_amd import chain
    return chain.ControlPoints(links, offsets)


def control_points(d, which):
    return ControlPoints(*point_set(d, which))


def resolved(d, links):
    return [int(k) if k >= 0 else d - 1 for k in links]


def truncated(chain, k, r):
    """The chain dict cut after link k, with tool = r: what a point (k, r) is the tool of."""
    out = {key: np.asarray(chain[key])[:k + 1] for key in LINK_KEYS}
    out["gravity"], out["tool"] = np.asarray(chain["gravity"]), np.asarray(r, dtype=np.float64)
    return out


def evaluations(q, qs, qss):
    zero = np.zeros_like(q)
    return {"wa": (q, zero, qs), "wb": (q, qs, qss)}


def point_accelerations(chain, links, offsets, q, qd, qdd, dtype=np.float64, absolute=False):
    """[..., P, 3]: the numpy tool acceleration (linear part) of every point's cut chain."""
    d = len(chain["joint_type"])
    out = []
    for k, r in zip(resolved(d, links), offsets):
        cut = truncated(chain, k, r)
        out.append(tool_accel_ref.tool_acceleration(cut, q[..., :k + 1], qd[..., :k + 1], qdd[..., :k + 1], dtype, absolute)[..., :3])
    return np.stack(out, -2)


def point_speeds(chain, links, offsets, q, qs, dtype=np.float64, absolute=False):
    """[..., P]: the numpy squared tool speed of every point's cut chain."""
    d = len(chain["joint_type"])
    out = []
    for k, r in zip(resolved(d, links), offsets):
        out.append(chain_ref.tool_vsv(truncated(chain, k, r), q[..., :k + 1], qs[..., :k + 1], None, dtype, absolute))
    return np.stack(out, -1)


def reference_of(chain, links, offsets, q, qs, qss):
    """float64 references of speed2, wa, wb with their magnitudes (name + "_mag") and, under "yardstick", the error each shows
    against np.longdouble in the metric."""
    quantities = {"speed2": (point_speeds, (chain, links, offsets, q, qs))}
    quantities.update({name: (point_accelerations, (chain, links, offsets) + args) for name, args in evaluations(q, qs, qss).items()})
    return cc.references(quantities)


@functools.lru_cache(maxsize=None)
def reference(d, which):
    chain, q, qs, qss = cc.case(d)
    return reference_of(chain, *point_set(d, which), q, qs, qss)


def bound(d, which, name):
    return BOUND_FACTOR * reference(d, which)["yardstick"][name]


def accuracy_table():
    """{"<dof><set>": {quantity: {"yardstick", "bound"}}}: what profiles/control_points_accuracy.json records."""
    return cc.table({"%d%s" % (d, w): reference(d, w)["yardstick"] for d, w in CASES})

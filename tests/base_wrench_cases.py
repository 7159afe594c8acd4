"""What the base-reaction tests share: inputs that exist already -- the chains of tests/chain_cases.py (one per dof of DOFS,
B = 5 trajectories of N + 1 = 41 gridpoints: 205 points) and the trees of tests/tree_cases.py (vee, skip, nested, roots, torso,
y17, y18, comb32; B = 3, N + 1 = 23: 69 points) --, ONE fixed random mount (a tilted frame, its origin away from the base's, a
platform mass beside the base), the float64 references computed once, and the accuracy bound.

The shapes are the smallest that exercise one block and a partial one, every fork pattern (a second child that is not j + 1, a
child after a whole sub-chain, a fork inside a branch with three children), several roots, and the LDS maximum (32 dof, 4 forks).

The bound is that of tests/chain_cases.py, by its method and with its factor: the metric is |got - ref| / (the reference
evaluated with every product and sum in absolute value), the yardstick is the error the float64 reference itself shows against
the same recursion in np.longdouble on these very inputs, per case and per quantity, and the bound is BOUND_FACTOR (16) times
that.  The quantities: "w0" = w(q, 0, 0), "wa" = w(q, 0, q'), "wb" = w(q, q', q'') of the fused entry, and "wrench" = the single
entry on (q, q', q''), whose reference is wb's.  profiles/base_wrench_accuracy.json holds the yardsticks and bounds
(accuracy_table) and the fractions of them the kernels used on the GPU.

A case is named by its dof (a chain) or by its shape's name (a tree): CASES lists them all.
"""
import functools

import numpy as np

from tests import base_wrench_ref, chain_cases as cc, chain_ref, tree_cases as tc

BOUND_FACTOR, metric = cc.BOUND_FACTOR, cc.metric
DOFS, NAMES = cc.DOFS, tc.NAMES
CASES = tuple(DOFS) + tuple(NAMES)
QUANTITIES = ("w0", "wa", "wb", "wrench")


def _mount():
    rng = np.random.default_rng(5151)
    m = {"rot": chain_ref.random_rotation(rng), "origin": rng.uniform(-0.4, 0.4, 3), "mass": 23.0, "com": rng.uniform(-0.3, 0.3, 3)}
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return m


MOUNT = _mount()


def case(key):
    """(robot dict, q, qs, qss [B, N+1, d]) of a case: a chain for a dof, a tree for a shape's name."""
    return tc.case(key) if isinstance(key, str) else cc.case(key)


def still(key):
    """The trajectory of the case that stands still in joint space."""
    return 1 if isinstance(key, str) else 2


def evaluations(q, qs, qss):
    """The arguments of w0, wa, wb and the single evaluation."""
    zero = np.zeros_like(q)
    return {"w0": (q, zero, zero), "wa": (q, zero, qs), "wb": (q, qs, qss), "wrench": (q, qs, qss)}


def reference_of(robot, mount, q, qs, qss):
    """float64 references of w0, wa, wb, wrench with their magnitudes (name + "_mag") and, under "yardstick", the error each
    shows against np.longdouble in the metric."""
    fn, ev = functools.partial(base_wrench_ref.base_wrench, mount=mount), evaluations(q, qs, qss)
    return cc.alias(cc.references({name: (fn, (robot,) + ev[name]) for name in ("w0", "wa", "wb")}), "wrench", "wb")


@functools.lru_cache(maxsize=None)
def reference(key):
    return reference_of(case(key)[0], MOUNT, *case(key)[1:])


def bound(key, name):
    return BOUND_FACTOR * reference(key)["yardstick"][name]


def accuracy_table():
    """{case: {quantity: {"yardstick", "bound"}}}: what profiles/base_wrench_accuracy.json records."""
    return cc.table({str(k): reference(k)["yardstick"] for k in CASES})

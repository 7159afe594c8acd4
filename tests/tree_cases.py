"""The inputs the tree tests share, their references (computed once) and the accuracy bound.

Shapes, each the smallest for the thing it can get wrong (SHAPES): the smallest fork, whose second child is not j + 1 (vee); a
fork whose later child comes after a whole sub-chain (skip); a fork inside a branch, with three children so that its bank is
stored to once and added to once (nested: trunk 0-1, a branch 2-3-4 off link 0, and off that branch's first link the branches
5-6 and 7-8); a forest of two 9-link chains on the base (roots); a torso joint carrying two 7-dof arms (torso: the fused state);
one fork at 17 and at 18 dof (y17, y18: both sides of the fused / one-after-the-other switch); 32 dof with 4 forks (comb32: the
LDS maximum and TPR_TREE_MAX_FORKS).  The links are chain_ref.random_chain's: mixed revolute / prismatic joints, tilted axes,
rotated joint frames, full inertias, one massless link; gravity on, and off in NO_GRAVITY.  B = 3 trajectories of N + 1 = 23
gridpoints: 69 points, two blocks with the second one partial; one trajectory stands still.

The accuracy metric and bound are those of tests/chain_cases.py: |got - ref| over the all-absolute magnitude, against 16 x the
error the float64 reference itself shows against np.longdouble on the same inputs, per case and per quantity;
profiles/tree_dynamics_accuracy.json holds the yardsticks and bounds (accuracy_table).
"""
import functools

import numpy as np

from tests import chain_cases as cc, tree_ref
from tests.chain_cases import BOUND_FACTOR, evaluations, metric  # noqa: F401  (the tests take them from here)

B, N = 3, 22


def _y(trunk, d):
    arm = (d - trunk) // 2
    return [i - 1 for i in range(trunk + arm)] + [trunk - 1] + [i - 1 for i in range(trunk + arm + 1, d)]


SHAPES = {
    "vee": [-1, 0, 0],
    "skip": [-1, 0, 1, 0],
    "nested": [-1, 0, 0, 2, 3, 2, 5, 2, 7],
    "roots": [-1] + list(range(8)) + [-1] + list(range(9, 17)),
    "torso": [-1] + list(range(7)) + [0] + list(range(8, 14)),
    "y17": _y(5, 17),
    "y18": _y(6, 18),
    "comb32": [i - 1 for i in range(12)] + sum(([j] + [t + k for k in range(4)] for j, t in ((2, 12), (4, 17), (6, 22), (8, 27))), []),
}
FORKS = {"vee": 1, "skip": 1, "nested": 2, "roots": 0, "torso": 1, "y17": 1, "y18": 1, "comb32": 4}
NAMES = tuple(SHAPES)
NO_GRAVITY = ("skip", "roots", "y17")  # (w0 is then an exact zero: the metric asks for equality)


def forks_of(parents):
    """The forks of a parent table: the links j that are the parent of some link i != j + 1."""
    return sorted(set(p for i, p in enumerate(parents) if p >= 0 and p != i - 1))


def leaves_of(parents):
    return [i for i in range(len(parents)) if i not in set(parents)]


def path_to(parents, link):
    path = []
    while link >= 0:
        path.append(link)
        link = parents[link]
    return path[::-1]


@functools.lru_cache(maxsize=None)
def case(name):
    """(tree dict, q, qs, qss [B, N+1, d]) of a shape."""
    parents = SHAPES[name]
    d, k = len(parents), NAMES.index(name)
    tree = tree_ref.random_tree(parents, seed=300 + k, gravity=name not in NO_GRAVITY, massless=d // 2 if d > 2 else None)
    rng = np.random.default_rng(400 + k)
    q = rng.uniform(-3.0, 3.0, (B, N + 1, d))
    qs = rng.standard_normal((B, N + 1, d))
    qss = 2.0 * rng.standard_normal((B, N + 1, d))
    qs[1] = 0.0  # a trajectory standing still in joint space
    for a in (q, qs, qss):
        a.flags.writeable = False
    return tree, q, qs, qss


def reference_of(tree, q, qs, qss):
    """float64 references of w0, wa, wb with their magnitudes (name + "_mag"), and under "yardstick" the error each shows
    against the same recursion in np.longdouble, in the metric."""
    return cc.references({name: (tree_ref.rnea, (tree,) + args) for name, args in evaluations(q, qs, qss).items()})


@functools.lru_cache(maxsize=None)
def reference(name):
    return reference_of(*case(name))


def bound(name, quantity):
    """The accuracy bound of a quantity in a shape's case: BOUND_FACTOR times the float64 reference's own error there."""
    return BOUND_FACTOR * reference(name)["yardstick"][quantity]


def accuracy_table():
    """{shape: {quantity: {"yardstick", "bound"}}}: what profiles/tree_dynamics_accuracy.json records."""
    return cc.table({n: reference(n)["yardstick"] for n in NAMES})

"""What the effective-mass tests share: inputs that exist already -- the path samples of tests/chain_cases.py (one chain per dof of
DOFS, B = 5 trajectories of N + 1 = 41 gridpoints: 205 points, three blocks and a partial one) and of tests/tree_cases.py (every fork
pattern, several roots, comb32 at the LDS maximum; B = 3, N + 1 = 23: 69 points), one trajectory of each standing still --, robots
drawn from the same seeds WITHOUT a weightless link (a weightless leaf makes the mass matrix singular; the entry documents that
as the caller's responsibility), the point sets, the references computed once, and the accuracy bound.

Point sets, fixed per case (point_set):
  "set"   the last link, a middle link twice (two points on one link, not adjacent in the set), link 0; on a tree also one point
          on every leaf (one per branch) and one on the first fork (below the branches) -- at most 16, in an order that is not
          the links';
  "full"  sixteen points spread over the links in a shuffled order, on the cases of FULL (1 dof: all sixteen on one link; 32 dof
          and comb32: the LDS maximum; 7 dof and torso: the shapes the timings quote).

The metric is the RELATIVE error of speed2 and mobility against the restatement of the kernel's walk in np.longdouble
(tests/effective_mass_ref.py: walk) on the same inputs; where that reference is zero (the trajectory standing still) the values
must be zero.  The yardstick, per case, point set and quantity, is the larger of two distances to that reference: the float64
restatement's and the float64 dense route's (mass matrix and solve) -- both from references alone.  The bound is BOUND_FACTOR
(the family's 16) times the yardstick.  profiles/effective_mass_accuracy.json holds the yardsticks and bounds (accuracy_table)
and the fractions of them the kernel used on the GPU.

A case is named by its dof (a chain) or by its shape's name (a tree): CASES lists them all; the names of a case's table are
"speed2", "mobility" and, on the cases of FULL, "speed2_full", "mobility_full".
"""
import functools

import numpy as np

from tests import chain_cases as cc, chain_ref, effective_mass_ref as er, tree_cases as tc, tree_ref

BOUND_FACTOR = cc.BOUND_FACTOR
DOFS, NAMES = cc.DOFS, tc.NAMES
CASES = tuple(DOFS) + tuple(NAMES)
FULL = (1, 7, 32, "torso", "comb32")
QUANTITIES = ("speed2", "mobility")
SETS = ("set", "full")


@functools.lru_cache(maxsize=None)
def case(key):
    """(robot dict, q, qs [B, N+1, d]) of a case: the siblings' path samples on a robot of the same seed with no weightless link."""
    if isinstance(key, str):
        _, q, qs, _ = tc.case(key)
        robot = tree_ref.random_tree(tc.SHAPES[key], seed=300 + NAMES.index(key), gravity=key not in tc.NO_GRAVITY, massless=None)
    else:
        _, q, qs, _ = cc.case(key)
        robot = chain_ref.random_chain(key, seed=100 + key, gravity=(DOFS.index(key) % 2 == 0), massless=None)
    assert np.all(np.asarray(robot["mass"]) > 0)
    return robot, q, qs


def robot_of(key):
    """The toppra_amd robot of a case."""
    robot = case(key)[0]
    return tree_ref.kinematic_tree(robot) if isinstance(key, str) else chain_ref.serial_chain(robot)


def sets_of(key):
    return SETS if key in FULL else SETS[:1]


@functools.lru_cache(maxsize=None)
def point_set(key, which):
    """(links [P] resolved to 0 .. d-1, offsets [P, 3]) of set ``which`` on a case."""
    robot = case(key)[0]
    d = len(robot["joint_type"])
    rng = np.random.default_rng(900 + 13 * CASES.index(key) + SETS.index(which))
    if which == "full":
        links = [int(k) for k in rng.permutation(np.round(np.linspace(0, d - 1, 16)).astype(int))]
    else:
        mid = (d - 1) // 2
        links = [d - 1, mid, 0, mid]
        if isinstance(key, str):
            parents = tc.SHAPES[key]
            extra = [i for i in tc.leaves_of(parents) if i != d - 1] + tc.forks_of(parents)[:1]
            links = (links[:2] + extra + links[2:])[:16]
    offsets = rng.uniform(-0.25, 0.25, (len(links), 3))
    offsets.flags.writeable = False
    return tuple(links), offsets


def control_points(key, which):
    from toppra_amd import chain
    links, offsets = point_set(key, which)
    return chain.ControlPoints(list(links), offsets)


def name_of(quantity, which):
    return quantity if which == "set" else quantity + "_full"


def relative_error(got, ref):
    """The largest |got - ref| / |ref|; where the reference is zero the values must be zero."""
    got, ref = np.asarray(got, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    dead = ref == 0
    assert np.all(got[dead] == 0), "values differ from zero where the reference is zero"
    return float(np.max(np.abs(got - ref)[~dead] / np.abs(ref)[~dead])) if (~dead).any() else 0.0


@functools.lru_cache(maxsize=None)
def reference(key):
    """{name: the longdouble restatement [B, N+1, P], "yardstick": {name: ...}, "dense": {name: the float64 dense route}} of a
    case, both point sets under the table's names.  The arrays are read-only."""
    robot, q, qs = case(key)
    out = {"yardstick": {}, "dense": {}}
    for which in sets_of(key):
        links, offsets = point_set(key, which)
        exact = er.walk(robot, links, offsets, q, qs, dtype=np.longdouble)
        plain = er.walk(robot, links, offsets, q, qs)
        dense = er.dense(robot, links, offsets, q, qs)
        for k, quantity in enumerate(QUANTITIES):
            name = name_of(quantity, which)
            out[name], out["dense"][name] = exact[k], dense[k]
            out["yardstick"][name] = max(relative_error(plain[k], exact[k]), relative_error(dense[k], exact[k]))
            exact[k].flags.writeable = dense[k].flags.writeable = False
    return out


def bound(key, name):
    return BOUND_FACTOR * reference(key)["yardstick"][name]


def accuracy_table():
    """{case: {quantity: {"yardstick", "bound"}}}: what profiles/effective_mass_accuracy.json records."""
    return cc.table({str(k): reference(k)["yardstick"] for k in CASES})

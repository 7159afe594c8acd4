"""What the momentum tests share: inputs that exist already -- the chains of tests/chain_cases.py (one per dof of DOFS, B = 5
trajectories of N + 1 = 41 gridpoints: 205 points, three blocks and a partial one) and the trees of tests/tree_cases.py (every
fork pattern, several roots, comb32 at the LDS maximum; B = 3, N + 1 = 23: 69 points) --, the mount frame of
tests/base_wrench_cases.py (a tilted frame, its origin away from the base's), the float64 references computed once, and the
accuracy bound.

Link sets.  Every case is evaluated on all of its links ("all") and on ONE fixed subset ("set"): for a chain the upper half of
its links, d // 2 .. d - 1; for a tree one branch -- the whole sub-tree that hangs on BRANCH[name], a link that does not follow
its parent in the numbering (asserted, not assumed: link_set()).  "nested"'s branch ends below the tree's last link, so the walk
ends early there; the others' sets begin in the middle of the walk.

The bound is that of tests/chain_cases.py, by its method and with its factor: the metric is |got - ref| / (the reference
evaluated with every product and sum in absolute value), the yardstick is the error the float64 reference itself shows against
the same expressions in np.longdouble on these very inputs, per case, link set and quantity, and the bound is BOUND_FACTOR (16)
times that.  The quantities: "momentum" [..., 6] and "energy2" [...], each under "all" and "set" -- the names of a case's table
are "momentum", "energy2", "momentum_set", "energy2_set".  profiles/momentum_accuracy.json holds the yardsticks and bounds
(accuracy_table) and the fractions of them the kernel used on the GPU.

A case is named by its dof (a chain) or by its shape's name (a tree): CASES lists them all.
"""
import functools

from tests import base_wrench_cases as bc, chain_cases as cc, momentum_ref, tree_cases as tc

BOUND_FACTOR, metric = cc.BOUND_FACTOR, cc.metric
DOFS, NAMES = cc.DOFS, tc.NAMES
CASES = tuple(DOFS) + tuple(NAMES)
QUANTITIES = ("momentum", "energy2")
SETS = ("all", "set")
MOUNT = bc.MOUNT
case, still = bc.case, bc.still

# the first link of each tree's branch, and the branch itself as it is expected to come out
BRANCH = {"vee": 2, "skip": 3, "nested": 5, "roots": 9, "torso": 8, "y17": 11, "y18": 12, "comb32": 27}
BRANCH_LINKS = {"vee": (2,), "skip": (3,), "nested": (5, 6), "roots": tuple(range(9, 18)), "torso": tuple(range(8, 15)),
                "y17": tuple(range(11, 17)), "y18": tuple(range(12, 18)), "comb32": tuple(range(27, 32))}


def link_set(key, which):
    """The link numbers of a case's link set: None for "all"; for "set" a chain's upper half, or a tree's branch."""
    if which == "all":
        return None
    if not isinstance(key, str):
        return tuple(range(key // 2, key))
    parents, first = tc.SHAPES[key], BRANCH[key]
    assert parents[first] != first - 1, (key, "the branch's first link follows its parent: not a branch off a fork or the base")
    below = tuple(i for i in range(len(parents)) if first in tc.path_to(parents, i))  # the sub-tree that hangs on `first`
    assert below == BRANCH_LINKS[key] and 0 < len(below) < len(parents), (key, below)
    return below


def name_of(quantity, which):
    return quantity if which == "all" else quantity + "_set"


def reference_of(robot, mount, q, qs, links):
    """float64 references of momentum and energy2 on one link set with their magnitudes (name + "_mag") and, under "yardstick",
    the error each shows against np.longdouble in the metric."""
    return cc.references({name: (functools.partial(getattr(momentum_ref, name), mount=mount, links=links), (robot, q, qs))
                          for name in QUANTITIES})


@functools.lru_cache(maxsize=None)
def reference(key):
    """Both link sets' references of a case under the table's names."""
    robot, q, qs, _ = case(key)
    out = {"yardstick": {}}
    for which in SETS:
        ref = reference_of(robot, MOUNT, q, qs, link_set(key, which))
        for name in QUANTITIES:
            full = name_of(name, which)
            out[full], out[full + "_mag"], out["yardstick"][full] = ref[name], ref[name + "_mag"], ref["yardstick"][name]
    return out


def bound(key, name):
    return BOUND_FACTOR * reference(key)["yardstick"][name]


def accuracy_table():
    """{case: {quantity: {"yardstick", "bound"}}}: what profiles/momentum_accuracy.json records."""
    return cc.table({str(k): reference(k)["yardstick"] for k in CASES})

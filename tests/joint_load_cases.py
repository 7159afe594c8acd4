"""What the joint-load tests share: inputs that exist already -- the chains of tests/chain_cases.py (one per dof of DOFS, 205
points) and the trees of tests/tree_cases.py (69 points) --, for each case a seeded set of sections with random frames, the
float64 references computed once, and the accuracy bound.

The sections of a case always hold joint 0, the last link, every fork, one child i != j + 1 of every fork, and two sections on
one joint (the last link's, with different frames), in a seeded random order.  A set holds at most 8 sections
(TPR_JOINT_MAX_SECTIONS); comb32 needs 11 (4 forks, 4 such children), so its sections are served in two sets (section_sets(key) = the index
lists of the calls); every other case is one set.  Outputs of the calls, concatenated in that order, are [..., S, 6] over all S
sections of the case.

The bound is that of tests/chain_cases.py, by its method and with its factor: |got - ref| / (the reference evaluated with every
product and sum in absolute value), against BOUND_FACTOR (16) x the error the float64 reference itself shows against np.longdouble
on these very inputs, per case and per quantity ("w0", "wa", "wb" of the fused entry, "wrench" = the single entry, whose
reference is wb's).  profiles/joint_load_accuracy.json holds the yardsticks, bounds, the fractions of the bounds the link-local
restatement (tests/joint_load_ref.py) uses on the CPU and the fractions the kernels used on the GPU.
"""
import functools

import numpy as np

from tests import base_wrench_cases as bc, chain_cases as cc, chain_ref, joint_load_ref, tree_cases as tc
from tests.chain_ref import parents_of

BOUND_FACTOR, metric = cc.BOUND_FACTOR, cc.metric
DOFS, NAMES = cc.DOFS, tc.NAMES
CASES = bc.CASES
QUANTITIES = bc.QUANTITIES
MAX_SECTIONS = 8
case, still, evaluations = bc.case, bc.still, bc.evaluations
# The chosen recipe: A = the plain link-local recursion with (f, n) kept, allowed while the restatement stays
# within this share of every bound.
RECIPE, RECIPE_A_SHARE = "A", 0.5


def required_links(parents):
    """Joint 0, the last link, every fork, one child i != j + 1 of every fork; then the last link again."""
    d = len(parents)
    forks = tc.forks_of(parents)
    kids = [max(i for i in range(d) if parents[i] == j and i != j + 1) for j in forks]
    links = []
    for i in [0, d - 1] + forks + kids:
        if i not in links:
            links.append(i)
    return links + [d - 1]


@functools.lru_cache(maxsize=None)
def _sections(key):
    robot = case(key)[0]
    links = required_links(parents_of(robot))
    rng = np.random.default_rng(7000 + CASES.index(key))
    links = [links[i] for i in rng.permutation(len(links))]
    S = len(links)
    sec = {"link": np.array(links, dtype=np.int64), "rot": np.stack([chain_ref.random_rotation(rng) for _ in range(S)]),
           "origin": rng.uniform(-0.3, 0.3, (S, 3))}
    for v in sec.values():
        v.flags.writeable = False
    sets = tuple(tuple(range(at, min(at + MAX_SECTIONS, S))) for at in range(0, S, MAX_SECTIONS))
    return sec, sets


def sections(key):
    """Every section of a case as one dict (link [S], rot [S, 3, 3], origin [S, 3]); S may exceed 8: see section_sets."""
    return _sections(key)[0]


def section_sets(key):
    """The index lists of the calls that serve a case's sections, each at most 8 long, in order."""
    return _sections(key)[1]


def by_sets(key, call):
    """call(sections dict of one set) -> [..., s, 6] or a tuple of such, for every set of the case, concatenated along S."""
    outs = [call(joint_load_ref.subset(sections(key), idx)) for idx in section_sets(key)]
    if isinstance(outs[0], tuple):
        return tuple(np.concatenate([np.asarray(o[k]) for o in outs], -2) for k in range(len(outs[0])))
    return np.concatenate([np.asarray(o) for o in outs], -2)


def reference_of(robot, sec, q, qs, qss):
    """float64 references of w0, wa, wb, wrench [B, N+1, S, 6] with their magnitudes (name + "_mag") and, under "yardstick", the
    error each shows against np.longdouble in the metric."""
    fn, ev = functools.partial(joint_load_ref.joint_wrenches, sections=sec), evaluations(q, qs, qss)
    return cc.alias(cc.references({name: (fn, (robot,) + ev[name]) for name in ("w0", "wa", "wb")}), "wrench", "wb")


@functools.lru_cache(maxsize=None)
def reference(key):
    return reference_of(case(key)[0], sections(key), *case(key)[1:])


def bound(key, name):
    return BOUND_FACTOR * reference(key)["yardstick"][name]


@functools.lru_cache(maxsize=None)
def restatement_fractions(key):
    """{quantity: the link-local restatement's error in the metric over the bound}; where the bound is zero (no gravity: w0 is an
    exact zero) the metric itself, which must then be zero."""
    robot, q, qs, qss = case(key)
    ref, out = reference(key), {}
    for name, args in evaluations(q, qs, qss).items():
        got = joint_load_ref.local_joint_wrenches(robot, *args, sections=sections(key))
        err, b = metric(got, ref[name], ref[name + "_mag"]), bound(key, name)
        out[name] = err / b if b > 0 else err
    return out


def worst_restatement(gravity):
    """The largest restatement fraction over the cases with (True) or without (False) gravity."""
    return max(max(restatement_fractions(k).values()) for k in CASES if bool(np.asarray(case(k)[0]["gravity"]).any()) == bool(gravity))


def accuracy_table():
    """{case: {quantity: {"yardstick", "bound", "restatement"}}}: what profiles/joint_load_accuracy.json records."""
    table = cc.table({str(k): reference(k)["yardstick"] for k in CASES})
    for k in CASES:
        for n, entry in table[str(k)].items():
            entry["restatement"] = restatement_fractions(k)[n]
    return table

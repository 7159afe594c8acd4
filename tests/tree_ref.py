"""The kinematic tree of include/toppra_hip.h (tpr_tree_*) for the tests: its reference is tests/chain_ref.py's recursive
Newton-Euler inverse dynamics in WORLD coordinates, which walks a parent table (the kernels work in link-local frames and keep
banks at the forks: nothing but the model is shared); the chain is the tree -1, 0, 1, ...  ``dtype`` and ``absolute`` as there.

A tree is a chain dict (tests/chain_ref.py; ``tool`` is not read and may be missing) with parent [d]: the link joint i attaches
link i to, -1 = the base; -1 <= parent[i] < i.
"""
import numpy as np

from tests.chain_ref import random_chain, rnea  # noqa: F401  (rnea(tree, q, qd, qdd, dtype, absolute): tau [..., d])


def random_tree(parents, seed, gravity=True, massless=None, prismatic_every=3):
    """chain_ref.random_chain's links (mixed joint types, tilted axes, rotated frames, full inertias, one massless link) on the
    given parent table."""
    tree = random_chain(len(parents), seed, gravity=gravity, massless=massless, prismatic_every=prismatic_every)
    tree["parent"] = np.array(parents, dtype=np.int32)
    return tree


def kinematic_tree(tree):
    """The toppra_amd.chain.KinematicTree of a tree dict."""
    from toppra_amd.chain import KinematicTree
    return KinematicTree(tree["parent"], tree["joint_type"], tree["axis"], tree["rot"], tree["trans"], tree["mass"], tree["com"],
                         tree["inertia"], gravity=tree["gravity"])

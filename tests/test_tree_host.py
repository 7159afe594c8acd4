"""The kinematic tree on the CPU: what KinematicTree validates and counts, the serial chain to a link, a payload on any link,
and the numpy reference (tests/tree_ref.py) against the chain's on chain-shaped trees."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import chain_cases as cc, chain_ref, tree_cases as tc, tree_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _links(tree):
    return [tree[k] for k in ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia")]


def test_validation_and_repr():
    from toppra_amd import KinematicTree, chain
    assert KinematicTree is chain.KinematicTree
    tree = tc.case("nested")[0]
    kt = KinematicTree(tc.SHAPES["nested"], *_links(tree), gravity=tree["gravity"])
    assert repr(kt) == "KinematicTree(9 dof, 2 forks, 4 leaves: RPRRPRRPR)"
    assert kt.dof == 9 and kt.parents.dtype == np.int32 and kt.parents.tolist() == tc.SHAPES["nested"]
    assert not hasattr(kt, "tool")
    for name, key in (("axes", "axis"), ("rotations", "rot"), ("translations", "trans"), ("masses", "mass"), ("coms", "com"),
                      ("inertias", "inertia"), ("gravity", "gravity")):
        assert np.array_equal(getattr(kt, name), tree[key]), name
        with pytest.raises(ValueError):
            getattr(kt, name)[...] = 0.0
    with pytest.raises(ValueError):
        kt.parents[0] = 0
    assert np.array_equal(KinematicTree(tc.SHAPES["nested"], *_links(tree)).gravity, [0.0, 0.0, -9.81])
    good = list(tc.SHAPES["nested"])
    for i, p in ((0, 0), (4, 4), (3, 7), (2, -2), (8, 8)):
        bad = list(good)
        bad[i] = p
        with pytest.raises(ValueError, match="the parent of link %d is %d, outside -1 .. %d" % (i, p, i - 1)):
            KinematicTree(bad, *_links(tree))
    for bad in (None, [[-1, 0]], [-1.0, 0.0, 0.0], "abc"):
        with pytest.raises(ValueError, match="parents"):
            KinematicTree(bad, *_links(tree))
    with pytest.raises(ValueError, match="parents has 8 entries, joint_types 9"):
        KinematicTree(good[:8], *_links(tree))
    with pytest.raises(ValueError, match="a tree has 1..32 joints, got 33"):
        KinematicTree([-1] * 33, *_links(tree))
    # the per-link arguments are validated as SerialChain validates them
    links = _links(tree)
    with pytest.raises(ValueError, match="axes must be unit vectors"):
        KinematicTree(good, links[0], 2.0 * links[1], *links[2:])
    with pytest.raises(ValueError, match="masses must be >= 0"):
        KinematicTree(good, *(links[:4] + [-links[4]] + links[5:]))
    with pytest.raises(ValueError, match="inertia holds a value that is not finite"):
        KinematicTree(good, *(links[:6] + [np.full((9, 6), np.inf)]))
    with pytest.raises(ValueError, match="joint_types must hold"):
        KinematicTree(good, ["ball"] * 9, *links[1:])


@pytest.mark.parametrize("name", tc.NAMES)
def test_fork_counting(name):
    kt = tree_ref.kinematic_tree(tc.case(name)[0])
    assert kt.forks == tc.forks_of(tc.SHAPES[name]) and len(kt.forks) == tc.FORKS[name]
    assert all(p >= 0 for p in kt.forks)  # the base is never a fork


def test_more_than_four_forks_are_refused_with_the_count():
    from toppra_amd import KinematicTree, _capi
    assert _capi.TREE_MAX_FORKS == 4
    tree = tree_ref.random_tree([-1, 0, 0, 1, 1, 2, 2, 3, 3], seed=1)
    assert len(tree_ref.kinematic_tree(tree).forks) == 4
    tree["parent"][8] = 5
    with pytest.raises(NotImplementedError, match=r"the tree has 5 forks \(links \[0, 1, 2, 3, 5\]\), the kernels keep banks for 4"):
        tree_ref.kinematic_tree(tree)
    # a forest of many roots has no fork at all
    assert KinematicTree([-1] * 9, *_links(tree)).forks == []


def test_from_chain_and_the_chain_shaped_table():
    from toppra_amd import KinematicTree
    chain = cc.case(9)[0]
    sc = chain_ref.serial_chain(chain)
    for kt in (KinematicTree.from_chain(sc), KinematicTree(np.arange(9) - 1, *_links(chain), gravity=chain["gravity"])):
        assert kt.parents.tolist() == list(range(-1, 8)) and kt.forks == [] and kt.joint_types == sc.joint_types
        for name in ("axes", "rotations", "translations", "masses", "coms", "inertias", "gravity"):
            assert np.array_equal(getattr(kt, name), getattr(sc, name)), name


@pytest.mark.parametrize("name", ["vee", "nested", "torso", "comb32"])
def test_chain_to(name):
    tree = tc.case(name)[0]
    kt = tree_ref.kinematic_tree(tree)
    for link in range(kt.dof):
        sc, joints = kt.chain_to(link, tool=(0.1, 0.2, 0.3))
        assert joints.tolist() == tc.path_to(tc.SHAPES[name], link) and joints[-1] == link
        assert sc.dof == len(joints) and np.array_equal(sc.tool, [0.1, 0.2, 0.3]) and np.array_equal(sc.gravity, kt.gravity)
        assert sc.joint_types == [kt.joint_types[i] for i in joints]
        for attr in ("axes", "rotations", "translations", "masses", "coms", "inertias"):
            assert np.array_equal(getattr(sc, attr), getattr(kt, attr)[joints]), attr
    assert np.array_equal(kt.chain_to(0)[0].tool, np.zeros(3))
    for bad in (-1, kt.dof):
        with pytest.raises(ValueError, match="outside the tree's links"):
            kt.chain_to(bad)


def test_with_payload_on_a_chain_shaped_tree_is_the_chain_s():
    from toppra_amd import KinematicTree, Payload
    sc = chain_ref.serial_chain(cc.case(7)[0])
    A = np.random.default_rng(3).uniform(-0.1, 0.1, (3, 3))
    for obj in (Payload(1.7, com=(0.05, -0.02, 0.11), inertia=A @ A.T + 0.01 * np.eye(3)), Payload(0.0, inertia=[0.01, 0.02, 0.03, 0, 0, 0])):
        loaded, want = KinematicTree.from_chain(sc).with_payload(obj, 6), sc.with_payload(obj)
        for name in ("axes", "rotations", "translations", "masses", "coms", "inertias", "gravity"):
            assert np.array_equal(getattr(loaded, name), getattr(want, name)), name
        assert loaded.parents.tolist() == list(range(-1, 6))
    with pytest.raises(ValueError, match="outside the tree's links"):
        KinematicTree.from_chain(sc).with_payload(obj, 7)


def test_with_payload_loads_the_joints_as_an_appended_link_does():
    """torso, one hand loaded: tree_ref torques of the merged tree equal those of a tree with the payload appended as a massive
    link on a zero-length joint that is held still, within 16 x the error the float64 appended tree shows against np.longdouble
    (the metric of tests/chain_cases.py; the bound of the chain's with_payload test)."""
    from toppra_amd import Payload
    tree, q, qs, qss = tc.case("torso")
    A = np.random.default_rng(4).uniform(-0.1, 0.1, (3, 3))
    obj = Payload(2.5, com=(0.03, -0.04, 0.12), inertia=A @ A.T + 0.01 * np.eye(3))
    hand = 14
    kt = tree_ref.kinematic_tree(tree).with_payload(obj, hand)
    merged = dict(tree, mass=kt.masses, com=kt.coms, inertia=kt.inertias)
    assert merged["mass"][hand] == tree["mass"][hand] + 2.5 and np.array_equal(np.delete(merged["mass"], hand), np.delete(tree["mass"], hand))
    more = {"parent": np.append(tree["parent"], hand), "joint_type": np.append(tree["joint_type"], 0),
            "axis": np.vstack([tree["axis"], [0.0, 0.0, 1.0]]), "rot": np.concatenate([tree["rot"], np.eye(3)[None]]),
            "trans": np.vstack([tree["trans"], np.zeros(3)]), "mass": np.append(tree["mass"], obj.mass),
            "com": np.vstack([tree["com"], obj.com]), "inertia": np.vstack([tree["inertia"], obj.inertia]), "gravity": tree["gravity"]}
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (1,))], -1)  # noqa: E731
    got = tree_ref.rnea(merged, q, qs, qss)
    want, mag, ld = (tree_ref.rnea(more, pad(q), pad(qs), pad(qss), **kw)[..., :15] for kw in ({}, {"absolute": True}, {"dtype": np.longdouble}))
    yardstick = cc._own_error(want, ld, mag)
    err = tc.metric(got, want, mag)
    print("merged vs appended link %.3g, bound %.3g" % (err, tc.BOUND_FACTOR * yardstick))
    assert 0 < yardstick and err <= tc.BOUND_FACTOR * yardstick
    assert np.abs(got - tree_ref.rnea(tree, q, qs, qss))[..., [0, 8, 14]].min() > 1e-3  # the load is felt from the hand to the torso
    assert np.array_equal(got[..., 1:8], tree_ref.rnea(tree, q, qs, qss)[..., 1:8])  # and not in the other arm


@pytest.mark.parametrize("d", [1, 2, 7, 18])
def test_the_reference_on_a_chain_shaped_tree_is_the_chain_s(d):
    chain, q, qs, qss = cc.case(d) if d in cc.DOFS else (chain_ref.random_chain(d, seed=5),) + tuple(np.random.default_rng(6).standard_normal((3, 2, 4, d)))
    tree = dict(chain, parent=np.arange(d) - 1)
    for kw in ({}, {"absolute": True}, {"dtype": np.longdouble}):
        assert np.array_equal(tree_ref.rnea(tree, q, qs, qss, **kw), chain_ref.rnea(chain, q, qs, qss, **kw)), kw


def test_the_reference_sums_a_fork_s_branches():
    """vee with both children alike and mirrored inputs: by symmetry of the model (not of the code) joint 0 carries both branches --
    the torque of a branch alone, twice, less the trunk link's own share."""
    tree, q, qs, qss = (np.array(v) if isinstance(v, np.ndarray) else v for v in tc.case("vee"))
    tree = {k: np.array(v) for k, v in tree.items()}
    for k in ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia"):
        tree[k][2] = tree[k][1]
    for a in (q, qs, qss):
        a[..., 2] = a[..., 1]
    both = tree_ref.rnea(tree, q, qs, qss)
    one = tree_ref.rnea(dict(tree, mass=tree["mass"] * [1, 1, 0], inertia=tree["inertia"] * [[1], [1], [0]]), q, qs, qss)
    trunk = tree_ref.rnea(dict(tree, mass=tree["mass"] * [1, 0, 0], inertia=tree["inertia"] * [[1], [0], [0]]), q, qs, qss)
    assert np.array_equal(both[..., 1], both[..., 2]) and np.array_equal(both[..., 1], one[..., 1])
    scale = np.abs(one[..., 0]) + np.abs(trunk[..., 0])
    assert np.all(np.abs(both[..., 0] - (2.0 * one[..., 0] - trunk[..., 0])) <= 64 * np.finfo(float).eps * scale)


def test_import_works_without_the_reference():
    """toppra_amd and a KinematicTree need neither the reference package nor the CPU restatement beside the tests."""
    code = ("import sys\n"
            "class Block(object):\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name.split('.')[0] in ('toppra', 'oracle'):\n"
            "            raise ImportError(name + ' is blocked')\n"
            "sys.meta_path.insert(0, Block())\n"
            "import toppra_amd as ta\n"
            "t = ta.KinematicTree([-1, 0, 0], 'rpr', [[0, 0, 1]] * 3, [[[1, 0, 0], [0, 1, 0], [0, 0, 1]]] * 3, [[0, 0, 0.1]] * 3, [1, 1, 1],\n"
            "                     [[0, 0, 0]] * 3, [[0.1, 0.1, 0.1, 0, 0, 0]] * 3)\n"
            "assert t.forks == [0] and 'toppra' not in sys.modules and 'oracle' not in sys.modules\n"
            "print('ok', t)\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, TOPPRA_HIP_NO_TORCH="1"))
    assert out.returncode == 0 and out.stdout.startswith("ok KinematicTree(3 dof, 1 forks, 2 leaves: RPR)"), out.stderr

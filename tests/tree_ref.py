"""Plain numpy reference for the kinematic tree of include/toppra_hip.h (tpr_tree_*): recursive Newton-Euler inverse dynamics
written from the textbook recursion in WORLD coordinates (the kernels work in link-local frames and keep banks at the forks:
nothing but the model is shared).  ``dtype`` and ``absolute`` as in tests/chain_ref.py, whose small vector helpers and
nothing-cancels arithmetic are used; on a chain-shaped tree every operation is chain_ref.rnea's, in its order.

A tree is a chain dict (tests/chain_ref.py; ``tool`` is not read and may be missing) with parent [d]: the link joint i attaches
link i to, -1 = the base; -1 <= parent[i] < i.
"""
import numpy as np

from tests.chain_ref import _Mag, _add, _cross, _dot, _mm, _mtv, _mv, _rodrigues, _scale, random_chain


def rnea(tree, q, qd, qdd, dtype=np.float64, absolute=False):
    """tau(q, qd, qdd), arrays [..., d]."""
    wrap = (lambda x: _Mag(x)) if absolute else (lambda x: x)
    qa, qda, qdda = (np.asarray(a, dtype=dtype) for a in (q, qd, qdd))
    lead = qa.shape[:-1]
    par = {k: np.asarray(tree[k], dtype=dtype) for k in ("axis", "rot", "trans", "mass", "com", "inertia", "gravity")}
    parent = [int(p) for p in tree["parent"]]
    d = len(parent)
    one, zero = wrap(np.ones(lead, dtype=dtype)), wrap(np.zeros(lead, dtype=dtype))
    base = {"R": [[one if r == c else zero for c in range(3)] for r in range(3)], "p": [zero] * 3, "w": [zero] * 3,
            "wd": [zero] * 3, "a": [zero - wrap(par["gravity"][k]) * one for k in range(3)]}
    links = []
    for i in range(d):
        assert -1 <= parent[i] < i, (i, parent[i])
        up = base if parent[i] < 0 else links[parent[i]]
        R, w, wd, a = up["R"], up["w"], up["wd"], up["a"]
        qi, qdi, qddi = wrap(qa[..., i]), wrap(qda[..., i]), wrap(qdda[..., i])
        rot = [[wrap(par["rot"][i, r, c]) * one for c in range(3)] for r in range(3)]
        k = [wrap(par["axis"][i, j]) * one for j in range(3)]
        Rj = _mm(R, rot)
        z = _mv(Rj, k)
        r = _mv(R, [wrap(par["trans"][i, j]) * one for j in range(3)])
        prismatic = int(tree["joint_type"][i]) == 1
        if prismatic:
            Rl = Rj
            r = _add(r, _scale(z, qi))
        else:
            Rl = _mm(Rj, _rodrigues(k, wrap(np.sin(qa[..., i])), wrap(np.cos(qa[..., i]))))
        a_new = _add(_add(a, _cross(wd, r)), _cross(w, _cross(w, r)))
        if prismatic:
            w_new, wd_new = w, wd
            a_new = _add(_add(a_new, _scale(z, qddi)), _scale(_cross(w, z), 2 * qdi))
        else:
            w_new = _add(w, _scale(z, qdi))
            wd_new = _add(_add(wd, _scale(z, qddi)), _scale(_cross(w, z), qdi))
        L = {"R": Rl, "p": _add(up["p"], r), "z": z, "w": w_new, "wd": wd_new, "a": a_new, "prismatic": prismatic}
        com = _mv(Rl, [wrap(par["com"][i, j]) * one for j in range(3)])
        ac = _add(_add(L["a"], _cross(L["wd"], com)), _cross(L["w"], _cross(L["w"], com)))
        I = par["inertia"][i]
        Il = [[wrap(I[0]), wrap(I[3]), wrap(I[4])], [wrap(I[3]), wrap(I[1]), wrap(I[5])], [wrap(I[4]), wrap(I[5]), wrap(I[2])]]
        inertia = lambda x, Rl=Rl, Il=Il: _mv(Rl, _mv(Il, _mtv(Rl, x)))  # noqa: E731
        L["F"] = _scale(ac, wrap(par["mass"][i]))
        L["N"] = _add(inertia(L["wd"]), _cross(L["w"], inertia(L["w"])))
        L["c"] = com
        links.append(L)
    # what the children hand down: (force, moment about this link's origin), summed in descending child number
    handed = [None] * d
    tau = [None] * d
    for i in range(d - 1, -1, -1):
        L = links[i]
        f, n = handed[i] if handed[i] is not None else ([zero] * 3, [zero] * 3)
        f = _add(L["F"], f)
        n = _add(_add(L["N"], _cross(L["c"], L["F"])), n)
        tau[i] = _dot(L["z"], f) if L["prismatic"] else _dot(L["z"], n)
        p = parent[i]
        if p >= 0:
            lever = [L["p"][k] - links[p]["p"][k] for k in range(3)]
            give = (f, _add(n, _cross(lever, f)))
            handed[p] = give if handed[p] is None else (_add(handed[p][0], give[0]), _add(handed[p][1], give[1]))
    return np.stack([t.v if absolute else t for t in tau], -1)


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

"""Plain numpy reference for the joint wrenches of include/toppra_hip.h (tpr_tree_joint_wrench_*): the full 6-D wrench the parent
side exerts ON link i through joint i, reported in a section frame fixed to link i.  joint_wrenches is written the textbook way:
tests/chain_ref.py's way up and way down in WORLD coordinates, every link's (f, n) kept, and only at the end turned into the
link's frame and from there into the section's.  ``dtype`` and ``absolute`` as in tests/tree_ref.py.

Beside it, local_joint_wrenches: a float64 RESTATEMENT of the order the kernels use -- the link-local recursion of
toppra_amd/csrc/tpr_chain_rnea.hip.inc on tpr_tree.hip.inc's walk (the children i != j + 1 of a fork summed in descending number,
the carry on the left), with (f, n) kept: the same operations in the same order, with numpy's sine and cosine.  It exists to
measure, on the CPU, what that order costs against the accuracy bound (tests/joint_load_cases.py, restatement_fractions).

A robot is a tree dict (tests/tree_ref.py) or a chain dict (tests/chain_ref.py; no "parent": the tree -1, 0, 1, ...).  Sections
are a dict: link [S] (resolved, 0 .. d-1), rot [S, 3, 3] (columns = the section frame's axes in link coordinates), origin [S, 3]
(in link coordinates).
"""
import numpy as np

from tests.chain_ref import _add, _cross, _mm, _mtv, _mv, _rodrigues, _scale, backward, forward, parents_of


def default_sections(links):
    links = np.asarray(links, dtype=np.int64).reshape(-1)
    return {"link": links, "rot": np.broadcast_to(np.eye(3), (len(links), 3, 3)).copy(), "origin": np.zeros((len(links), 3))}


def subset(sections, index):
    index = np.asarray(index, dtype=np.int64)
    return {k: np.asarray(sections[k])[index] for k in ("link", "rot", "origin")}


def link_wrenches(robot, q, qd, qdd, dtype=np.float64, absolute=False):
    """(per link i: (f, n, R), ar) -- the wrench ON link i through joint i in WORLD axes, the moment about link i's origin, and the
    link frame's rotation, lists of 3 (3 x 3) arrays over the leading shape; and the evaluation's arithmetic."""
    links, ar = forward(robot, q, qd, qdd, dtype, absolute, dynamics=True)
    return [(f, n, L["R"]) for L, (f, n) in zip(links, backward(links, ar))], ar


def joint_wrenches(robot, q, qd, qdd, sections, dtype=np.float64, absolute=False):
    """w(q, qd, qdd) [..., S, 6]: per section [force; moment about its origin] in its axes; arrays [..., d]."""
    per_link, ar = link_wrenches(robot, q, qd, qdd, dtype=dtype, absolute=absolute)
    rows = []
    for k, i in enumerate(np.asarray(sections["link"]).tolist()):
        f, n, R = per_link[i]
        f, n = _mtv(R, f), _mtv(R, n)  # in link axes; then [Rk' f; Rk' (n - ok x f)]
        Rk = ar.mat(np.asarray(sections["rot"])[k])
        shift = _cross(ar.vec(np.asarray(sections["origin"])[k]), f)
        rows.append(ar.stack(_mtv(Rk, f) + _mtv(Rk, [n[j] - shift[j] for j in range(3)])))
    return np.stack(rows, -2)


def local_link_wrenches(robot, q, qd, qdd):
    """The restatement: per link (f, n) in LINK axes, the moment about the link's origin, float64, the kernels' order."""
    qa, qda, qdda = (np.asarray(a, dtype=np.float64) for a in (q, qd, qdd))
    lead = qa.shape[:-1]
    par = {k: np.asarray(robot[k], dtype=np.float64) for k in ("axis", "rot", "trans", "mass", "com", "inertia", "gravity")}
    parent = parents_of(robot)
    d = len(parent)
    one, zero = np.ones(lead), np.zeros(lead)
    vec = lambda x: [x[j] * one for j in range(3)]  # noqa: E731
    base = (vec(np.zeros(3)), vec(np.zeros(3)), [zero - par["gravity"][k] * one for k in range(3)])
    kin, joints, FN = [], [], []
    for i in range(d):
        w, wd, a = base if parent[i] < 0 else kin[parent[i]]
        prismatic = int(robot["joint_type"][i]) == 1
        k, com = vec(par["axis"][i]), vec(par["com"][i])
        rot = [[par["rot"][i, r, c] * one for c in range(3)] for r in range(3)]
        qi = qa[..., i]
        s, c, slide = (zero, one, qi) if prismatic else (np.sin(qi), np.cos(qi), zero)
        E = _mm(rot, _rodrigues(k, s, c))
        r = _add(vec(par["trans"][i]), _mv(rot, _scale(k, slide)))
        zr, zp = (vec(np.zeros(3)), k) if prismatic else (k, vec(np.zeros(3)))
        ar = _add(_add(a, _cross(wd, r)), _cross(w, _cross(w, r)))
        wl = _mtv(E, w)
        a_i = _add(_add(_mtv(E, ar), _scale(zp, qdda[..., i])), _scale(_cross(wl, zp), 2.0 * qda[..., i]))
        w_i = _add(wl, _scale(zr, qda[..., i]))
        wd_i = _add(_add(_mtv(E, wd), _scale(zr, qdda[..., i])), _scale(_cross(wl, zr), qda[..., i]))
        kin.append((w_i, wd_i, a_i))
        joints.append((E, r))
        ac = _add(_add(a_i, _cross(wd_i, com)), _cross(w_i, _cross(w_i, com)))
        I = par["inertia"][i]
        Il = [[I[0], I[3], I[4]], [I[3], I[1], I[5]], [I[4], I[5], I[2]]]
        FN.append((_scale(ac, par["mass"][i]), _add(_mv(Il, wd_i), _cross(w_i, _mv(Il, w_i))), com))
    bank = [None] * d   # a fork's children i != j + 1, summed in descending number
    carry = None        # link i + 1's wrench when it is link i's child
    out = [None] * d
    for i in range(d - 1, -1, -1):
        C = carry
        if bank[i] is not None:
            C = bank[i] if C is None else (_add(C[0], bank[i][0]), _add(C[1], bank[i][1]))
        if C is None:
            C = (vec(np.zeros(3)), vec(np.zeros(3)))
        F, Nm, com = FN[i]
        f = _add(F, C[0])
        n = _add(_add(Nm, _cross(com, F)), C[1])
        out[i] = (f, n)
        E, r = joints[i]
        cf = _mv(E, f)
        give = (cf, _add(_mv(E, n), _cross(r, cf)))
        carry = None
        p = parent[i]
        if p == i - 1:
            carry = give if p >= 0 else None
        elif p >= 0:
            bank[p] = give if bank[p] is None else (_add(bank[p][0], give[0]), _add(bank[p][1], give[1]))
    return out


def local_joint_wrenches(robot, q, qd, qdd, sections):
    """The restatement in section frames, [..., S, 6]: out = [Rk' f; Rk' (n + f x ok)]."""
    per_link = local_link_wrenches(robot, q, qd, qdd)
    one = np.ones(np.asarray(q).shape[:-1])
    rows = []
    for k, i in enumerate(np.asarray(sections["link"]).tolist()):
        f, n = per_link[i]
        Rk = [[np.asarray(sections["rot"], dtype=np.float64)[k, r, c] * one for c in range(3)] for r in range(3)]
        ok = [np.asarray(sections["origin"], dtype=np.float64)[k, j] * one for j in range(3)]
        rows.append(np.stack(_mtv(Rk, f) + _mtv(Rk, _add(n, _cross(f, ok))), -1))
    return np.stack(rows, -2)


def joint_sections_of(sections):
    """The toppra_amd.chain.JointSections of a sections dict."""
    from toppra_amd.chain import JointSections
    return JointSections(np.asarray(sections["link"]).tolist(), origins=sections["origin"], rotations=sections["rot"])

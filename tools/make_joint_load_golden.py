#!/usr/bin/env python
"""Generate the joint-load fixtures tests/golden/joint_load_*.npz by running the REAL reference (hungpham2511/toppra): its
SecondOrderConstraint with inv_dyn = the numpy joint wrenches of tests/joint_load_ref.py, flattened section-major; and
profiles/joint_load_accuracy.json.  The recipe, and how the two tolerances are made, is tools/rigid_golden.py's.

    python tools/make_joint_load_golden.py        # needs the reference; builds oracle/_ref on demand

Stored beside the recipe's arrays: the robot, the sections (section_*), F, g, w0, wa, wb [B, N+1, S, 6], scheme, and the limits
(tilting, axial, radial, sides; or force, moment).  Two fixtures, sized within the 122 rows of a stage:
  joint_load_torso_d15_N30: a torso joint that carries two 7-dof arms, JointSections.on_axes at the first joint of each arm (the
      shoulder bearings, their centres 4 cm along the axes), BatchJointLoadConstraint.bearing's rows with sides = 6 -- 14 rows per
      section --, Interpolation: 2 + 60 + 56 = 118 rows per stage.  The limits are one per section for the whole batch: the
      largest static norm along the paths plus a share of the largest dynamic part along the reference's own solutions WITHOUT
      the constraint, over cos(pi / sides) -- standing still satisfies the polygon with room.
  joint_load_d4_N30_colloc: tools/rigid_golden.py's SCARA, sections at joint 1 (the elbow bearing) and at the prismatic joint (a
      linear guide's carriage), force / moment boxes chosen per trajectory as base_wrench_d4_N30_colloc chooses its box,
      Collocation.
"""
import numpy as np

import rigid_golden as rg
from tests import joint_load_cases, joint_load_ref, tree_ref

SIDES = 6


def torso_with_shoulder_bearings():
    """The torso under gravity; the sections are the bearings of the arms' first joints (links 1 and 8), z along the joint axes,
    their centres 4 cm along them."""
    from toppra_amd.chain import JointSections
    tree = rg.torso([0.0, 0.0, -9.81])
    sections = JointSections.on_axes(tree_ref.kinematic_tree(tree), [1, 8], 0.04)
    return tree, {"link": np.asarray(sections.joints, dtype=np.int64), "rot": np.array(sections.rotations), "origin": np.array(sections.origins)}


def scara_with_a_linear_guide():
    return rg.as_tree(rg.scara()), {"link": np.array([1, 2], dtype=np.int64), "rot": np.tile(np.eye(3), (2, 1, 1)),
                                    "origin": np.array([[0.0, 0.0, 0.05], [0.0, 0.0, -0.05]])}


def fixture(name, B, N, seed, scheme, bearing):
    from toppra_amd.constraint import BatchJointLoadConstraint, _box_limits
    rng = np.random.default_rng(seed)
    robot, sec = torso_with_shoulder_bearings() if bearing else scara_with_a_linear_guide()
    d, S = len(robot["parent"]), len(sec["link"])
    inv_dyn = lambda q, qd, qdd: joint_load_ref.joint_wrenches(robot, q, qd, qdd, sec).reshape(np.shape(q)[:-1] + (6 * S,))  # noqa: E731
    p = rg.draw_paths(rng, B, d, N, 0.5 if bearing else rg.SCARA_WAY)
    terms = rg.gridpoint_terms(inv_dyn, p)
    free = rg.free_solutions(p)
    static = terms["w0"].reshape(B, N + 1, S, 6)
    moving = [rg.along(terms, free, b, static=True).reshape(N, S, 6) for b in range(B)]
    if bearing:
        norm = lambda x, at: np.sqrt(x[..., at] ** 2 + x[..., at + 1] ** 2)  # noqa: E731
        share, lims = 0.35, {}
        for key, at in (("tilting", 3), ("radial", 0)):
            rest = norm(static, at).max((0, 1))  # [S]
            peak = np.max([norm(m, at).max(0) for m in moving], 0)
            lims[key] = (rest + share * np.maximum(peak - rest, 0.0)) / np.cos(np.pi / SIDES)
        rest = np.abs(static[..., 2]).max((0, 1))
        peak = np.max([np.abs(m[..., 2]).max(0) for m in moving], 0)
        lims["axial"] = rest + share * np.maximum(peak - rest, 0.0)
        F, g1 = BatchJointLoadConstraint.bearing_rows(S, lims["tilting"], lims["axial"], lims["radial"], SIDES)
        g = np.broadcast_to(g1, (B, F.shape[0])).copy()
        extra = dict(lims, sides=np.array(SIDES))
    else:
        rest = np.abs(static).max(1)  # [B, S, 6]
        dynamic = np.stack([np.abs(m - static[b, :-1]).max(0) for b, m in enumerate(moving)])
        hi = rest + 0.5 * dynamic
        force, moment = np.stack([-hi[..., :3], hi[..., :3]], -1), np.stack([-hi[..., 3:], hi[..., 3:]], -1)  # [B, S, 3, 2]
        F, g, _ = _box_limits(S, 6, (("force", force, 0), ("moment", moment, 3)), "S", None, None)
        extra = {"force": force, "moment": moment}
    constraint = rg.reference().constraint
    DT = constraint.DiscretizationType(scheme)
    return rg.second_order_fixture(
        name, p, free, lambda b: constraint.SecondOrderConstraint(inv_dyn, lambda q_: F, lambda q_: g[b], dof=d, discretization_scheme=DT),
        F, g, scheme, terms, ("w0", "wa", "wb"), joint_load_cases.reference_of(robot, sec, p.q, p.qs, p.qss), False, robot,
        rg.ROBOT_KEYS, {"section_" + k: np.asarray(sec[k]) for k in ("link", "rot", "origin")}, extra=extra, shape=(B, N + 1, S, 6))


if __name__ == "__main__":
    fixtures = {"joint_load_torso_d15_N30": fixture("joint_load_torso_d15_N30", 4, 30, 718, 1, True),
                "joint_load_d4_N30_colloc": fixture("joint_load_d4_N30_colloc", 4, 30, 712, 0, False)}
    rg.write_profile("joint_load", "float64 tests/joint_load_ref.py", joint_load_cases.accuracy_table(), fixtures,
                     "; restatement = the share of the bound the float64 link-local restatement (the kernels' order) uses on the CPU",
                     recipe={"chosen": joint_load_cases.RECIPE,
                             "worst_restatement_fraction_with_gravity": joint_load_cases.worst_restatement(True),
                             "worst_restatement_fraction_without_gravity": joint_load_cases.worst_restatement(False)})

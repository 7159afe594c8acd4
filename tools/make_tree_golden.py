#!/usr/bin/env python
"""Generate the tree fixtures tests/golden/tree_torque_*.npz by running the REAL reference (hungpham2511/toppra): its
JointTorqueConstraint and TOPPRA(solver_wrapper="seidel") with inv_dyn taken from tests/tree_ref.py (the numpy recursion over a
kinematic tree), and profiles/tree_dynamics_accuracy.json.  The recipe, and how the two tolerances are made, is
tools/rigid_golden.py's.

    python tools/make_tree_golden.py        # needs the reference; builds oracle/_ref on demand

Stored beside the recipe's arrays: the tree with its parent table, taulim ([d, 2] shared, or [B, d, 2]), fric, w0, wa, wb,
torque_scheme, accel_scheme.
  tree_torque_vee_d3_N30_colloc: tests/tree_cases.py's vee, torque limits per trajectory under Collocation.
  tree_torque_torso_d15_N30: the torso; the torque limits under Interpolation and the acceleration limits under Collocation:
      4 d + 2 d = 90 rows per stage at 15 dof and the x and x_next pairs, 94 as the reference's dense rows count them (92 as
      BatchTOPPRA counts, which takes the x pair as a box): under the 122 the dense-row kernels hold.
"""
import numpy as np

import rigid_golden as rg
from tests import tree_cases, tree_ref


def fixture(name, B, shape, N, seed, torque_scheme, accel_scheme, per_traj_limits):
    rng = np.random.default_rng(seed)
    tree = tree_ref.random_tree(tree_cases.SHAPES[shape], seed=seed + 1, gravity=True, prismatic_every=4)
    inv_dyn = lambda q, qd, qdd: tree_ref.rnea(tree, q, qd, qdd)  # noqa: E731
    p = rg.draw_paths(rng, B, len(tree["parent"]), N)
    constraint = rg.reference().constraint
    DT = constraint.DiscretizationType(torque_scheme)
    return rg.torque_fixture(name, rng, p, tree, rg.TREE_KEYS, inv_dyn, tree_cases.reference_of(tree, p.q, p.qs, p.qss),
                             lambda lim, fric: constraint.JointTorqueConstraint(inv_dyn, lim, fric, discretization_scheme=DT),
                             torque_scheme, accel_scheme, per_traj_limits, {"accel_scheme": np.array(accel_scheme)})


if __name__ == "__main__":
    fixtures = {"tree_torque_vee_d3_N30_colloc": fixture("tree_torque_vee_d3_N30_colloc", 4, "vee", 30, 321, 0, 1, True),
                "tree_torque_torso_d15_N30": fixture("tree_torque_torso_d15_N30", 2, "torso", 30, 322, 1, 0, False)}
    rg.write_profile("tree_dynamics", "float64 tree_ref", tree_cases.accuracy_table(), fixtures)

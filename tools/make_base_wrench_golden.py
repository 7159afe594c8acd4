#!/usr/bin/env python
"""Generate the base-reaction fixtures tests/golden/base_wrench_*.npz by running the REAL reference (hungpham2511/toppra): its
SecondOrderConstraint with inv_dyn = the numpy base wrench of tests/base_wrench_ref.py; and profiles/base_wrench_accuracy.json.
The recipe, and how the two tolerances are made, is tools/rigid_golden.py's.

    python tools/make_base_wrench_golden.py        # needs the reference; builds oracle/_ref on demand

Stored beside the recipe's arrays: the robot, the mount (mount_*), F, g, w0, wa, wb, scheme (and mu, half_extents).
  base_wrench_torso_d15_N30: a torso joint that carries two 7-dof arms, on a cart (a platform under the base, the mount frame on
      the floor), BatchBaseWrenchConstraint.surface_contact's 16 rows -- the cart must not tip, slide or spin --, Interpolation:
      2 + 60 + 32 = 94 rows per stage.
  base_wrench_d4_N30_colloc: tools/rigid_golden.py's SCARA on a pedestal, the mount frame at the pedestal's foot, a force /
      moment box (the flange's data sheet), Collocation.  The box is chosen per trajectory: the largest static |w0| along the
      path plus half of the largest dynamic part |w - w0| along the reference's own solution WITHOUT the constraint -- standing
      still satisfies it with room, and it is active.
"""
import numpy as np

import rigid_golden as rg
from tests import base_wrench_cases, base_wrench_ref

MOUNT_KEYS = ("rot", "origin", "mass", "com")
I3, Z3 = np.eye(3), np.zeros((3, 3))
F_BOX = np.block([[I3, Z3], [-I3, Z3], [Z3, I3], [Z3, -I3]])


def torso_on_a_cart():
    """The torso under gravity, its base 0.6 m above the floor on a 40 kg cart whose centre of mass lies low; the mount frame is
    the floor under the base (normal +z)."""
    return rg.torso([0.0, 0.0, -9.81]), {"rot": np.eye(3), "origin": np.array([0.0, 0.0, -0.6]), "mass": 40.0,
                                         "com": np.array([0.02, -0.01, -0.45])}


def scara_on_a_pedestal():
    """(the pedestal's flange is not quite level)"""
    return rg.as_tree(rg.scara()), {"rot": rg.tilted(0.1), "origin": np.array([0.05, 0.0, -0.8]), "mass": 0.0, "com": np.zeros(3)}


def fixture(name, B, N, seed, scheme, contact):
    rng = np.random.default_rng(seed)
    robot, mount = torso_on_a_cart() if contact else scara_on_a_pedestal()
    d = len(robot["parent"])
    inv_dyn = lambda q, qd, qdd: base_wrench_ref.base_wrench(robot, q, qd, qdd, mount)  # noqa: E731
    p = rg.draw_paths(rng, B, d, N, 0.5 if contact else rg.SCARA_WAY)
    terms = rg.gridpoint_terms(inv_dyn, p)
    free = rg.free_solutions(p)
    if contact:
        F, g, extra = rg.surface_contact(B, 0.5, (0.30, 0.25))
    else:
        F, extra = F_BOX, {}
        hi = np.abs(terms["w0"]).max(1) + 0.5 * np.stack([np.abs(rg.along(terms, free, b)).max(0) for b in range(B)])  # [B, 6]
        g = np.concatenate((hi[:, :3], hi[:, :3], hi[:, 3:], hi[:, 3:]), -1)  # [upper; -lower] per part, the force first
    constraint = rg.reference().constraint
    DT = constraint.DiscretizationType(scheme)
    return rg.second_order_fixture(
        name, p, free, lambda b: constraint.SecondOrderConstraint(inv_dyn, lambda q_: F, lambda q_: g[b], dof=d, discretization_scheme=DT),
        F, g, scheme, terms, ("w0", "wa", "wb"), base_wrench_cases.reference_of(robot, mount, p.q, p.qs, p.qss), False, robot,
        rg.ROBOT_KEYS, {"mount_" + k: np.asarray(mount[k], dtype=np.float64) for k in MOUNT_KEYS}, extra=extra)


if __name__ == "__main__":
    fixtures = {"base_wrench_torso_d15_N30": fixture("base_wrench_torso_d15_N30", 4, 30, 618, 1, True),
                "base_wrench_d4_N30_colloc": fixture("base_wrench_d4_N30_colloc", 4, 30, 612, 0, False)}
    rg.write_profile("base_wrench", "float64 tests/base_wrench_ref.py", base_wrench_cases.accuracy_table(), fixtures)

#!/usr/bin/env python
"""Generate the chain fixtures tests/golden/chain_torque_*.npz by running the REAL reference (hungpham2511/toppra): its
JointTorqueConstraint and TOPPRA(solver_wrapper="seidel") with inv_dyn taken from tests/chain_ref.py (the numpy recursion), and
profiles/chain_dynamics_accuracy.json.  The recipe, and how the two tolerances are made, is tools/rigid_golden.py's.

    python tools/make_chain_golden.py        # needs the reference; builds oracle/_ref on demand

Stored beside the recipe's arrays: the chain, taulim ([d, 2] shared, or [B, d, 2]), fric, w0, wa, wb, torque_scheme.
  chain_torque_d6_N40: 6 dof, Collocation, one set of torque limits.
  chain_torque_d3_N30_interp: 3 dof, Interpolation, limits per trajectory.
The accuracy bound is relative to the all-absolute magnitude, which stands orders above the values for a 6-dof chain
(tests/chain_cases.py), so noise of its size is about 1e-12 relative to w0 and moves sd of about 0.4 by up to 5e-9 near the
switching points: sd_tol = 2e-8 for the 6-dof fixture, 5e-14 for the 3-dof one.
"""
import numpy as np

import rigid_golden as rg
from tests import chain_cases, chain_ref


def fixture(name, B, d, N, seed, torque_scheme, per_traj_limits):
    rng = np.random.default_rng(seed)
    chain = chain_ref.random_chain(d, seed=seed + 1, gravity=True, prismatic_every=4)
    inv_dyn = lambda q, qd, qdd: chain_ref.rnea(chain, q, qd, qdd)  # noqa: E731
    p = rg.draw_paths(rng, B, d, N)
    constraint = rg.reference().constraint
    DT = constraint.DiscretizationType(torque_scheme)
    return rg.torque_fixture(name, rng, p, chain, rg.CHAIN_KEYS, inv_dyn, chain_cases.reference_of(chain, p.q, p.qs, p.qss),
                             lambda lim, fric: constraint.JointTorqueConstraint(inv_dyn, lim, fric, discretization_scheme=DT),
                             torque_scheme, 1, per_traj_limits)


if __name__ == "__main__":
    fixtures = {"chain_torque_d6_N40": fixture("chain_torque_d6_N40", 4, 6, 40, 311, 0, False),
                "chain_torque_d3_N30_interp": fixture("chain_torque_d3_N30_interp", 4, 3, 30, 312, 1, True)}
    rg.write_profile("chain_dynamics", "float64 chain_ref", chain_cases.accuracy_table(), fixtures)

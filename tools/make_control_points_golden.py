#!/usr/bin/env python
"""Generate the control-point fixtures tests/golden/control_points_*.npz by running the REAL reference (hungpham2511/toppra):
its SecondOrderConstraint with inv_dyn = the numpy accelerations of the control points stacked [3 P] (tests/control_points_cases.py:
the tool acceleration of tests/tool_accel_ref.py on the chain cut after each point's link), F = the signed identity on every
point's three components and g the limits; and profiles/control_points_accuracy.json.  The recipe, and how the two tolerances
are made, is tools/rigid_golden.py's.

    python tools/make_control_points_golden.py        # needs the reference; builds oracle/_ref on demand

Stored beside the recipe's arrays: the chain, links, offsets, linear, F, g, wa, wb [B, N+1, 3 P], scheme.  w0 is an exact zero
and is not disturbed.
  control_points_d6_N40: 6 dof, three points (two on one link), Interpolation, limits per trajectory [B, P, 3, 2].
  control_points_d4_N30_colloc: 4 dof, four points, Collocation, one set of limits [P, 3, 2] for the batch.
The limits are a fraction of each point's largest acceleration along the reference's own solution WITHOUT the constraint -- so
the constraint is active -- lower and upper limits of different size and positive on both sides, so standing still satisfies
them and every trajectory stays feasible.
"""
import numpy as np

import rigid_golden as rg
from tests import chain_ref, control_points_cases as cp


def fixture(name, B, d, N, seed, scheme, links, per_traj):
    rng = np.random.default_rng(seed)
    chain = chain_ref.random_chain(d, seed=seed + 1, gravity=True, prismatic_every=4)
    links = np.array(links, dtype=np.int64)
    P = len(links)
    offsets = rng.uniform(-0.25, 0.25, (P, 3))
    inv_dyn = lambda q, qd, qdd: cp.point_accelerations(chain, links, offsets, q, qd, qdd).reshape(q.shape[:-1] + (3 * P,))  # noqa: E731
    p = rg.draw_paths(rng, B, d, N)
    terms = rg.gridpoint_terms(inv_dyn, p)
    assert not terms["w0"].any(), "acc(q, 0, 0) is an exact zero"
    free = rg.free_solutions(p)
    peak = np.array([np.abs(rg.along(terms, free, b)).reshape(-1, P, 3).max((0, 2)) for b in range(B)])  # [B, P]
    if per_traj:
        hi = 0.5 * peak[:, :, None] * (1.0 + 0.2 * rng.random((B, P, 3)))
    else:
        hi = 0.5 * peak.min(0)[:, None] * (1.0 + 0.2 * rng.random((P, 3)))
    linear = np.stack([-hi * (1.0 + 0.2 * rng.random(hi.shape)), hi], -1)
    F = rg.signed_identity(range(0, 3 * P, 3), 3 * P)
    g = np.concatenate((linear[..., 1], -linear[..., 0]), -1).reshape(hi.shape[:-2] + (6 * P,))  # [B, 6 P] or [6 P]
    constraint = rg.reference().constraint
    DT = constraint.DiscretizationType(scheme)
    return rg.second_order_fixture(
        name, p, free, lambda b: constraint.SecondOrderConstraint(inv_dyn, lambda q_: F, lambda q_: g[b] if per_traj else g, dof=d,
                                                                  discretization_scheme=DT),
        F, g, scheme, terms, ("wa", "wb"), cp.reference_of(chain, links, offsets, p.q, p.qs, p.qss), True, chain, rg.CHAIN_KEYS,
        {"links": links, "offsets": offsets}, {"linear": linear})


if __name__ == "__main__":
    fixtures = {"control_points_d6_N40": fixture("control_points_d6_N40", 4, 6, 40, 511, 1, [2, -1, 2], True),
                "control_points_d4_N30_colloc": fixture("control_points_d4_N30_colloc", 4, 4, 30, 512, 0, [-1, 0, 1, 1], False)}
    rg.write_profile("control_points", "the float64 numpy recursion on the chain cut after each point's link "
                     "(tests/control_points_cases.py)", cp.accuracy_table(), fixtures)

#!/usr/bin/env python
"""Generate the tool-acceleration fixtures tests/golden/tool_accel_*.npz by running the REAL reference (hungpham2511/toppra):
its SecondOrderConstraint with inv_dyn = the numpy tool acceleration of tests/tool_accel_ref.py, F = the signed identity on the
limited parts and g the limits -- the problem of the reference's examples-old/cartesian_accel.py; and
profiles/tool_accel_accuracy.json.  The recipe, and how the two tolerances are made, is tools/rigid_golden.py's.

    python tools/make_tool_accel_golden.py        # needs the reference; builds oracle/_ref on demand

Stored beside the recipe's arrays: the chain, linear (and angular), F, g, wa, wb, scheme.  w0 is an exact zero and is not
disturbed.
  tool_accel_d6_N40: 6 dof, Interpolation, linear limits.
  tool_accel_d3_N30_colloc: 3 dof, Collocation, linear and angular limits.
The limits are a fraction of the largest tool acceleration along the reference's own solution WITHOUT the constraint, per
trajectory (the angular ones: one set for the batch) -- so the constraint is active -- lower and upper limits of different size
and positive on both sides, so standing still satisfies them and every trajectory stays feasible.
"""
import numpy as np

import rigid_golden as rg
from tests import chain_ref, tool_accel_cases, tool_accel_ref


def fixture(name, B, d, N, seed, scheme, with_angular):
    rng = np.random.default_rng(seed)
    chain = chain_ref.random_chain(d, seed=seed + 1, gravity=True, prismatic_every=4)
    inv_dyn = lambda q, qd, qdd: tool_accel_ref.tool_acceleration(chain, q, qd, qdd)  # noqa: E731
    p = rg.draw_paths(rng, B, d, N)
    terms = rg.gridpoint_terms(inv_dyn, p)
    assert not terms["w0"].any(), "acc(q, 0, 0) is an exact zero"
    free = rg.free_solutions(p)
    peak = np.array([[np.abs(a[:, :3]).max(), np.abs(a[:, 3:]).max()] for a in (rg.along(terms, free, b) for b in range(B))])
    # linear: per trajectory [B, 3, 2]; angular: one [3, 2] for the batch
    hi = 0.5 * peak[:, 0, None] * (1.0 + 0.2 * rng.random((B, 3)))
    linear = np.stack([-hi * (1.0 + 0.2 * rng.random((B, 3))), hi], -1)
    g = np.concatenate((linear[..., 1], -linear[..., 0]), -1)  # [B, 6]
    extra = {}
    if with_angular:
        ahi = 0.6 * peak[:, 1].min() * (1.0 + 0.2 * rng.random(3))
        angular = extra["angular"] = np.stack([-ahi * (1.0 + 0.2 * rng.random(3)), ahi], -1)
        g = np.concatenate((g, np.broadcast_to(np.concatenate((angular[:, 1], -angular[:, 0])), (B, 6))), -1)
    F = rg.signed_identity([0, 3] if with_angular else [0], 6)
    constraint = rg.reference().constraint
    DT = constraint.DiscretizationType(scheme)
    return rg.second_order_fixture(
        name, p, free, lambda b: constraint.SecondOrderConstraint(inv_dyn, lambda q_: F, lambda q_: g[b], dof=d, discretization_scheme=DT),
        F, g, scheme, terms, ("wa", "wb"), tool_accel_cases.reference_of(chain, p.q, p.qs, p.qss), True, chain, rg.CHAIN_KEYS,
        own={"linear": linear}, extra=extra)


if __name__ == "__main__":
    fixtures = {"tool_accel_d6_N40": fixture("tool_accel_d6_N40", 4, 6, 40, 411, 1, False),
                "tool_accel_d3_N30_colloc": fixture("tool_accel_d3_N30_colloc", 4, 3, 30, 412, 0, True)}
    rg.write_profile("tool_accel", "float64 tests/tool_accel_ref.py", tool_accel_cases.accuracy_table(), fixtures)

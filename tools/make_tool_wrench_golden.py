#!/usr/bin/env python
"""Generate the tool-wrench fixtures tests/golden/tool_wrench_*.npz by running the REAL reference (hungpham2511/toppra): its
SecondOrderConstraint with inv_dyn = the numpy wrench of tests/tool_wrench_ref.py; and profiles/tool_wrench_accuracy.json.  The
recipe, and how the two tolerances are made, is tools/rigid_golden.py's.

    python tools/make_tool_wrench_golden.py        # needs the reference; builds oracle/_ref on demand

Stored beside the recipe's arrays: the chain, the payload (payload_*), F, g, w0, wa, wb, scheme (and mu, half_extents).
  tool_wrench_d6_N40: a random chain, a dense F (five rows that mix force and moment), Interpolation.  g is chosen per
      trajectory: the largest static value F w0 along the path plus half of the largest dynamic part F (w - w0) along the
      reference's own solution WITHOUT the constraint -- standing still satisfies it with room, and it is active.
  tool_wrench_d4_N30_colloc: a SCARA-like arm (vertical revolute axes, a vertical prismatic joint: the tray stays level) that
      carries a box on a tray, BatchToolWrenchConstraint.surface_contact's 16 rows, Collocation.
"""
import numpy as np

import rigid_golden as rg
from tests import chain_ref, tool_wrench_cases, tool_wrench_ref

PAYLOAD_KEYS = ("mass", "com", "inertia", "rot", "origin")


def box_on_tray(tool):
    """A 0.8 kg box, 10 x 6 x 8 cm, standing on the tray at the tool point: the contact frame is the tray's (normal +z)."""
    m, sx, sy, sz = 0.8, 0.10, 0.06, 0.08
    return {"mass": m, "com": np.asarray(tool) + np.array([0.0, 0.0, sz / 2]),
            "inertia": np.array([m * (sy ** 2 + sz ** 2) / 12, m * (sx ** 2 + sz ** 2) / 12, m * (sx ** 2 + sy ** 2) / 12, 0.0, 0.0, 0.0]),
            "rot": np.eye(3), "origin": np.asarray(tool, dtype=np.float64)}


def fixture(name, B, d, N, seed, scheme, contact):
    rng = np.random.default_rng(seed)
    if contact:
        chain = rg.scara()
        payload = box_on_tray(chain["tool"])
    else:
        chain = chain_ref.random_chain(d, seed=seed + 1, gravity=True, prismatic_every=4)
        payload = dict(tool_wrench_cases.PAYLOAD)
    inv_dyn = lambda q, qd, qdd: tool_wrench_ref.tool_wrench(chain, payload, q, qd, qdd)  # noqa: E731
    p = rg.draw_paths(rng, B, d, N, rg.SCARA_WAY if contact else 1.0)
    terms = rg.gridpoint_terms(inv_dyn, p)
    free = rg.free_solutions(p)
    if contact:
        F, g, extra = rg.surface_contact(B, 0.1, (0.05, 0.03))
    else:
        F, extra = rng.uniform(-1.0, 1.0, (5, 6)), {}
        static = np.einsum("mk,bnk->bnm", F, terms["w0"]).max(1)  # [B, m]
        dynamic = np.stack([np.abs(np.einsum("mk,nk->nm", F, rg.along(terms, free, b))).max(0) for b in range(B)])
        g = static + 0.5 * dynamic
    constraint = rg.reference().constraint
    DT = constraint.DiscretizationType(scheme)
    return rg.second_order_fixture(
        name, p, free, lambda b: constraint.SecondOrderConstraint(inv_dyn, lambda q_: F, lambda q_: g[b], dof=d, discretization_scheme=DT),
        F, g, scheme, terms, ("w0", "wa", "wb"), tool_wrench_cases.reference_of(chain, payload, p.q, p.qs, p.qss), False, chain,
        rg.CHAIN_KEYS, {"payload_" + k: np.asarray(payload[k], dtype=np.float64) for k in PAYLOAD_KEYS}, extra=extra)


if __name__ == "__main__":
    fixtures = {"tool_wrench_d6_N40": fixture("tool_wrench_d6_N40", 4, 6, 40, 511, 1, False),
                "tool_wrench_d4_N30_colloc": fixture("tool_wrench_d4_N30_colloc", 4, 4, 30, 512, 0, True)}
    rg.write_profile("tool_wrench", "float64 tests/tool_wrench_ref.py", tool_wrench_cases.accuracy_table(), fixtures)

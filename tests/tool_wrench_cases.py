"""What the tool-wrench tests share: the inputs of tests/chain_cases.py (one random chain per dof of DOFS, B = 5 trajectories
of N + 1 = 41 gridpoints -- 205 points: no multiple of 64, more than one block --, one of them standing still, gravity on in
every other case), ONE fixed random payload (a tilted contact frame, its origin away from the tool point, a full inertia), the
float64 references computed once, and the accuracy bound.

The bound is that of tests/chain_cases.py, by its method and with its factor: the metric is |got - ref| / (the reference
evaluated with every product and sum in absolute value), the yardstick is the error the float64 reference itself shows against
the same recursion in np.longdouble on these very inputs, per case and per quantity, and the bound is BOUND_FACTOR (16) times
that.  The quantities: "w0" = wrench(q, 0, 0), "wa" = wrench(q, 0, q'), "wb" = wrench(q, q', q'') of the fused entry, and
"wrench" = the single entry on (q, q', q''), whose reference is wb's.
"""
import functools

import numpy as np

from tests import chain_cases as cc, chain_ref, tool_wrench_ref

DOFS, B, N, BOUND_FACTOR = cc.DOFS, cc.B, cc.N, cc.BOUND_FACTOR


def _payload():
    rng = np.random.default_rng(4242)
    A = rng.uniform(-0.2, 0.2, (3, 3))
    full = A @ A.T + 0.02 * np.eye(3)
    p = {"mass": 1.7, "com": rng.uniform(-0.15, 0.15, 3),
         "inertia": np.array([full[0, 0], full[1, 1], full[2, 2], full[0, 1], full[0, 2], full[1, 2]]),
         "rot": chain_ref.random_rotation(rng), "origin": rng.uniform(-0.1, 0.1, 3)}
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return p


PAYLOAD = _payload()


def evaluations(q, qs, qss):
    """The arguments of w0, wa, wb and the single evaluation."""
    zero = np.zeros_like(q)
    return {"w0": (q, zero, zero), "wa": (q, zero, qs), "wb": (q, qs, qss), "wrench": (q, qs, qss)}


def reference_of(chain, payload, q, qs, qss):
    """float64 references of w0, wa, wb, wrench with their magnitudes (name + "_mag") and, under "yardstick", the error each
    shows against np.longdouble in the metric."""
    ev = evaluations(q, qs, qss)
    return cc.alias(cc.references({name: (tool_wrench_ref.tool_wrench, (chain, payload) + ev[name]) for name in ("w0", "wa", "wb")}),
                    "wrench", "wb")


@functools.lru_cache(maxsize=None)
def reference(d):
    return reference_of(cc.case(d)[0], PAYLOAD, *cc.case(d)[1:])


def bound(d, name):
    return BOUND_FACTOR * reference(d)["yardstick"][name]


def accuracy_table():
    """{dof: {quantity: {"yardstick", "bound"}}}: what profiles/tool_wrench_accuracy.json records."""
    return cc.table({str(d): reference(d)["yardstick"] for d in DOFS})

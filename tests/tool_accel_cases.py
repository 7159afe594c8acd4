"""What the tool-acceleration tests share: the inputs of tests/chain_cases.py (one random chain per dof of DOFS, B = 5
trajectories of N + 1 = 41 gridpoints, one of them standing still, gravity on in every other case -- it must make no
difference here), the float64 references computed once, and the accuracy bound.

The bound is that of tests/chain_cases.py, by its method and with its factor: the metric is |got - ref| / (the reference
evaluated with every product and sum in absolute value), the yardstick is the error the float64 reference itself shows against
the same recursion in np.longdouble on these very inputs, per case and per quantity, and the bound is BOUND_FACTOR (16) times
that.  The quantities: "wa" = acc(q, 0, q'), "wb" = acc(q, q', q'') of the fused entry, and "acc" = the single entry on
(q, q', q''), whose reference is wb's.
"""
import functools

import numpy as np

from tests import chain_cases as cc, tool_accel_ref

DOFS, B, N, BOUND_FACTOR = cc.DOFS, cc.B, cc.N, cc.BOUND_FACTOR


def evaluations(q, qs, qss):
    """The arguments of wa, wb and the single evaluation."""
    zero = np.zeros_like(q)
    return {"wa": (q, zero, qs), "wb": (q, qs, qss), "acc": (q, qs, qss)}


def reference_of(chain, q, qs, qss):
    """float64 references of wa, wb, acc with their magnitudes (name + "_mag") and, under "yardstick", the error each shows
    against np.longdouble in the metric."""
    ev = evaluations(q, qs, qss)
    return cc.alias(cc.references({name: (tool_accel_ref.tool_acceleration, (chain,) + ev[name]) for name in ("wa", "wb")}), "acc", "wb")


@functools.lru_cache(maxsize=None)
def reference(d):
    return reference_of(*cc.case(d))


def bound(d, name):
    return BOUND_FACTOR * reference(d)["yardstick"][name]


def accuracy_table():
    """{dof: {quantity: {"yardstick", "bound"}}}: what profiles/tool_accel_accuracy.json records."""
    return cc.table({str(d): reference(d)["yardstick"] for d in DOFS})

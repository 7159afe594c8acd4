"""The inputs the chain tests share, their references (computed once) and the accuracy bound.

Cases: one random chain per dof of DOFS -- both sides of the register / LDS split of the kernels (8 | 9), the fused / one-
after-the-other split of the 9..32-dof kernel (17 | 32) and TPR_MAX_DOF -- with mixed revolute / prismatic joints, tilted
axes, rotated joint frames, one massless link, gravity on and off, and B = 5 trajectories of N + 1 = 41 gridpoints (205 points:
no multiple of 64, more than one block), one of them standing still (q' = 0).

The accuracy bound.  The device's sine and cosine are not the host's, so bits cannot match.  The metric is
|got - ref| / (|ref| evaluated with every product and sum in absolute value); its yardstick is the error the float64
reference itself shows against the same recursion in np.longdouble, on these very inputs, taken per case and per quantity
(the magnitude of a quantity grows with the chain's depth and differs by tens of orders between w0 and the tool speed at 32
dof: one pooled figure would leave the deep cases unchecked); the bound is 16 x that (a different but fixed summation order,
and 1 - 2 ulp device trigonometry carried along up to 32 links).  Measured on the MI355X, the kernels use at most 10.5 of
the 16 (tool speed at 32 dof); profiles/chain_dynamics_accuracy.json holds the yardsticks and bounds.

What the figures mean, and what they do not.  The all-absolute magnitude of the world-frame reference grows roughly
geometrically with the chain's depth (every rotation multiplies it by up to sqrt 3), so at 32 dof it stands some 25 orders
above a torque and 50 above a tool speed, and a yardstick of 1e-40 or 1e-66 is NOT a relative accuracy of the value: relative
to the values the errors are of the usual rounding size.  The check reads "the kernel's error, weighted by that magnitude, is
at most 16 x the float64 reference's own worst weighted error on the same inputs" -- both sides carry the same weight, which
is why it is taken per case and per quantity: pooled into one figure (the issue's single yardstick read literally), the
shallow cases' 1e-16 would leave every deep case with a bound 1e24 times its own errors.
"""
import functools

import numpy as np

from tests import chain_ref

DOFS = (1, 2, 3, 7, 8, 9, 17, 32)
B, N = 5, 40
BOUND_FACTOR = 16.0
# a weight with cross terms between the linear and the angular part: symmetric, positive definite
_rng = np.random.default_rng(7)
_A = _rng.uniform(-1.0, 1.0, (6, 6))
S_FULL = _A @ _A.T + 0.5 * np.eye(6)


@functools.lru_cache(maxsize=None)
def case(d):
    """(chain dict, q, qs, qss [B, N+1, d]) of the dof-d case."""
    chain = chain_ref.random_chain(d, seed=100 + d, gravity=(DOFS.index(d) % 2 == 0), massless=d // 2 if d > 1 else None)
    rng = np.random.default_rng(200 + d)
    q = rng.uniform(-3.0, 3.0, (B, N + 1, d))
    qs = rng.standard_normal((B, N + 1, d))
    qss = 2.0 * rng.standard_normal((B, N + 1, d))
    qs[2] = 0.0  # a trajectory standing still in joint space
    for a in (q, qs, qss):
        a.flags.writeable = False
    return chain, q, qs, qss


def evaluations(q, qs, qss):
    """The arguments of w0, wa, wb."""
    zero = np.zeros_like(q)
    return {"w0": (q, zero, zero), "wa": (q, zero, qs), "wb": (q, qs, qss)}


def _own_error(val, ld, mag):
    live = mag > 0
    return float(np.max(np.abs(val - ld)[live] / mag[live])) if live.any() else 0.0


def references(quantities):
    """The scaffold every cases module of the family builds its references with.  ``quantities`` is {name: (fn, args)}, fn taking
    ``dtype=`` and ``absolute=``; returns {name: fn(*args) in float64, name + "_mag": its all-absolute magnitude, "yardstick":
    {name: the error the float64 value shows against np.longdouble, in the metric}}, the arrays read-only."""
    ref = {"yardstick": {}}
    for name, (fn, args) in quantities.items():
        ref[name], ref[name + "_mag"] = fn(*args), fn(*args, absolute=True)
        ref["yardstick"][name] = _own_error(ref[name], fn(*args, dtype=np.longdouble), ref[name + "_mag"])
        ref[name].flags.writeable = ref[name + "_mag"].flags.writeable = False
    return ref


def alias(ref, name, of):
    """Quantity ``name`` is quantity ``of`` under another entry's name: the same arrays, the same yardstick."""
    ref[name], ref[name + "_mag"], ref["yardstick"][name] = ref[of], ref[of + "_mag"], ref["yardstick"][of]
    return ref


def table(yardsticks):
    """{case: {quantity: {"yardstick", "bound"}}} of {case: a reference's "yardstick"}: what an accuracy profile records."""
    return {case: {k: {"yardstick": v, "bound": BOUND_FACTOR * v} for k, v in ys.items()} for case, ys in yardsticks.items()}


def reference_of(chain, q, qs, qss):
    """float64 references of w0, wa, wb, vsv (S = None) and vsv_S (S_FULL) with their magnitudes (name + "_mag"), and under
    "yardstick" the error each of them shows against the same recursion in np.longdouble, in the metric."""
    quantities = {name: (chain_ref.rnea, (chain,) + args) for name, args in evaluations(q, qs, qss).items()}
    quantities.update({name: (chain_ref.tool_vsv, (chain, q, qs, S)) for name, S in (("vsv", None), ("vsv_S", S_FULL))})
    return references(quantities)


@functools.lru_cache(maxsize=None)
def reference(d):
    return reference_of(*case(d))


def bound(d, name):
    """The accuracy bound of quantity ``name`` in the dof-d case: BOUND_FACTOR times the float64 reference's own error there."""
    return BOUND_FACTOR * reference(d)["yardstick"][name]


def accuracy_table():
    """{dof: {quantity: {"yardstick", "bound"}}}: what profiles/chain_dynamics_accuracy.json records."""
    return table({str(d): reference(d)["yardstick"] for d in DOFS})


def metric(got, ref, mag):
    """The largest |got - ref| / mag; where the magnitude is zero (every term vanishes) the values must agree exactly."""
    got, ref, mag = np.asarray(got), np.asarray(ref), np.asarray(mag)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    dead = mag == 0
    assert np.array_equal(got[dead], ref[dead]), "values differ where every term of the reference is zero"
    return float(np.max(np.abs(got - ref)[~dead] / mag[~dead])) if (~dead).any() else 0.0

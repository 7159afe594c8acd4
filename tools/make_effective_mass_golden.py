#!/usr/bin/env python
"""Generate the contact-energy fixtures tests/golden/contact_energy_*.npz by running the REAL reference (hungpham2511/toppra): a
host LinearConstraint that returns (None, None, None, None, None, None, xbound) -- the bound on x = sd^2 made from the numpy
squared speeds and mobilities of tests/effective_mass_ref.py; and the "fixtures" entry of profiles/effective_mass_accuracy.json.
The recipe, and how the two tolerances are made, is tools/rigid_golden.py's; the constraint has no rows, so the reference
wrapper's own low / high are stored, and the disturbed quantities are speed2 and mobility, the bound made again from them.

    python tools/make_effective_mass_golden.py        # needs the reference; builds oracle/_ref on demand

This family's metric is the RELATIVE error (tests/effective_mass_cases.py): the stored values are the np.longdouble restatement
rounded to float64, a quantity's "magnitude" is its own absolute value, and the yardstick is the larger of the float64
restatement's and the float64 dense route's distance to the longdouble restatement on the fixture's own inputs.

Stored beside the recipe's arrays: active, the robot, point_links, point_offsets, energy [B, P] (J), body_mass [P] (kg, inf = a
clamped body part), limit [B, P, 2] = (2 E_max, 1 / m_body), speed2, mobility (with their magnitudes), xbound.
  contact_energy_d6_N40: a 6-dof chain; the tool end, a middle link twice and link 0.
  contact_energy_torso_d15_N30: a torso joint that carries two 7-dof arms; both hands, both elbows and the torso.
The limits are chosen in physical units: a fraction of each point's peak contact energy along the reference's own solution WITHOUT
the constraint, lowered until the new bound is the active upper bound on x -- the controllable set's upper end K[i, 1] equals it,
below what the velocity limits leave -- at at least a quarter of the stages of every trajectory.  That is asserted.
"""
import json
import os

import numpy as np

import rigid_golden as rg
from oracle import oracle as orc
from tests import chain_cases as cc, chain_ref, effective_mass_cases as ec, effective_mass_ref as er, second_order_ref as sor
from tests.stage_boxes_ref import bound_only

NAMES = ("speed2", "mobility")


def chain6():
    robot = rg.as_tree(chain_ref.random_chain(6, seed=731, gravity=True, massless=None, prismatic_every=4))
    return robot, [5, 3, 0, 3], np.array([[0.05, 0.0, 0.12], [0.0, 0.08, 0.1], [0.1, 0.0, 0.0], [-0.06, 0.02, 0.2]]), np.array([4.0, 40.0, np.inf, 0.6])


def torso_arms():
    offsets = np.array([[0.0, 0.0, 0.1], [0.02, 0.0, 0.1], [0.0, 0.05, 0.0], [0.0, -0.05, 0.0], [0.15, 0.0, 0.3]])
    return rg.torso(), [7, 14, 4, 11, 0], offsets, np.array([0.6, 0.6, 3.0, 3.0, np.inf])


def reference_of(robot, links, offsets, q, qs):
    """The fixture's reference in the shape rigid_golden's steps take: {name: the longdouble walk rounded to float64, name + "_mag":
    its absolute value, "yardstick": {name: ...}}."""
    exact = er.walk(robot, links, offsets, q, qs, dtype=np.longdouble)
    plain, dense = er.walk(robot, links, offsets, q, qs), er.dense(robot, links, offsets, q, qs)
    ref = {"yardstick": {}}
    for k, name in enumerate(NAMES):
        ref[name] = exact[k].astype(np.float64)
        ref[name + "_mag"] = np.abs(ref[name])
        ref["yardstick"][name] = max(ec.relative_error(plain[k], exact[k]), ec.relative_error(dense[k], exact[k]))
    return ref


def fixture(name, B, N, seed, make):
    rng = np.random.default_rng(seed)
    robot, links, offsets, body = make()
    d, P = len(robot["parent"]), len(links)
    p = rg.draw_paths(rng, B, d, N, 0.5 if d > 8 else 1.0)
    ref = reference_of(robot, links, offsets, p.q, p.qs)
    s2, g = ref["speed2"], ref["mobility"]
    inv = 1.0 / body
    free = rg.free_solutions(p)  # each point's peak contact energy along the solution without the constraint, in J
    peak = np.array([np.max(0.5 * s2[b] / (inv + g[b] / s2[b]) * (sd * sd)[:, None], 0) for b, (_, sd) in enumerate(free)])  # [B, P]
    vel_high = sor.velocity_box(p.qs, p.vlim)[1][..., 1]
    fraction = 0.9
    while True:
        energy = fraction * peak * (1.0 + 0.1 * np.arange(B) / B)[:, None]  # (per trajectory: no two alike)
        lim = np.stack([2.0 * energy, np.broadcast_to(inv, (B, P))], -1)
        xb = er.xbound(s2, g, lim)
        rec, _ = rg.solve_reference(name, p, lambda b: bound_only(rg.reference().constraint, None, xb[b]), rows=False)
        active = [int(np.sum((rec["K"][b, :, 1] == xb[b, :, 1]) & (xb[b, :, 1] < vel_high[b]))) for b in range(B)]
        print("%s: fraction %.3f of the peak -> the bound is active at %s of %d stages" % (name, fraction, active, N + 1))
        if min(active) >= (N + 1 + 3) // 4:
            break
        fraction *= 0.85
        assert fraction > 0.02, "%s: the bound never becomes active at a quarter of the stages" % name
    assert all(4 * a >= N + 1 for a in active)
    rg.assert_active(name, rec["sd"], free)
    rec["active"] = np.array(active, dtype=np.int32)

    # the restatement: the box made from (disturbed) speed2 and mobility over the rows of the joint limits alone
    rows = sor.dense_problem(p.coef, p.breaks, p.grid, p.vlim, p.alim, True, [])

    def capped(terms):
        cap = er.xbound(terms["speed2"], terms["mobility"], lim)[..., 1]
        high = rows["high"].copy()
        high[..., 1] = np.where(high[..., 1] < cap, high[..., 1], cap)  # (dbl_min with the running value first, as the fold spells it)
        return high
    terms = {k: ref[k] for k in NAMES}
    assert np.array_equal(capped(terms), rec["high"]) and np.array_equal(rows["low"], rec["low"]), "the restated boxes differ"
    attached = {"point_links": np.array(links, dtype=np.int32), "point_offsets": offsets, "energy": energy, "body_mass": body}
    return rg.finish(name, p, rec, lambda t: orc.solve_dense_batch(rows["a"], rows["b"], rows["c"], rows["low"], capped(t), rows["deltas"]),
                     terms, NAMES, ref, True, robot, rg.ROBOT_KEYS, attached,
                     dict(limit=lim, speed2=s2, mobility=g, speed2_mag=ref["speed2_mag"], mobility_mag=ref["mobility_mag"], xbound=xb),
                     fraction_of_peak=fraction)


def write_profile(fixtures):
    """profiles/effective_mass_accuracy.json: the cases' table and the fixtures' entries; the `measured` entry of a GPU run is kept."""
    path = os.path.join(rg.ROOT, "profiles", "effective_mass_accuracy.json")
    doc = {"metric": "relative error |got - ref| / |ref| of speed2 and mobility against the np.longdouble restatement of the kernel's walk "
                     "(tests/effective_mass_ref.py: walk) on the same inputs; yardstick = the larger of the float64 restatement's and the "
                     "float64 dense route's (mass matrix and solve) distance to it; bound = %g x yardstick" % cc.BOUND_FACTOR,
           "cases": ec.accuracy_table(), "fixtures": fixtures}
    if os.path.exists(path):
        with open(path) as fh:
            measured = json.load(fh).get("measured")
        if measured is not None:
            doc["measured"] = measured
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    write_profile({"contact_energy_d6_N40": fixture("contact_energy_d6_N40", 4, 40, 831, chain6),
                   "contact_energy_torso_d15_N30": fixture("contact_energy_torso_d15_N30", 4, 30, 832, torso_arms)})

#!/usr/bin/env python
"""Generate the momentum fixtures tests/golden/momentum_*.npz by running the REAL reference (hungpham2511/toppra): a host
LinearConstraint that returns (None, None, None, None, None, None, xbound) -- the bound on x = sd^2 made from the numpy momentum
and kinetic energy of tests/momentum_ref.py; and profiles/momentum_accuracy.json.  The recipe, and how the two tolerances are
made, is tools/rigid_golden.py's; the constraint has no rows, so the reference wrapper's own low / high are stored, and the
disturbed quantities are momentum and energy2, the bound made again from them.

    python tools/make_momentum_golden.py        # needs the reference; builds oracle/_ref on demand

Stored beside the recipe's arrays: active, the robot, the mount (mount_*), limit_<kind>, links, limit, momentum, energy2 (with
their all-absolute magnitudes), xbound.
  momentum_d6_N40: a 6-dof chain, every link, a linear-momentum and an energy limit, per trajectory, about the base frame.
  momentum_torso_d15_N30: a torso joint that carries two 7-dof arms; the second arm's links alone, an angular- and a
      linear-momentum limit about a tilted mount frame away from the base.
The limits are chosen in physical units: a fraction of each quantity's peak along the reference's own solution WITHOUT the
constraint, lowered until the new bound is the active upper bound on x -- the controllable set's upper end K[i, 1] equals it,
below what the velocity limits leave -- at at least a quarter of the stages of every trajectory.  That is asserted.
"""
import numpy as np

import rigid_golden as rg
from oracle import oracle as orc
from tests import chain_ref, momentum_cases as mc, momentum_ref as mr, second_order_ref as sor
from tests.stage_boxes_ref import bound_only

NAMES = ("momentum", "energy2")
KINDS = ("linear", "angular", "energy")


def chain6():
    return rg.as_tree(chain_ref.random_chain(6, seed=711, gravity=True, prismatic_every=4)), dict(mr.NO_MOUNT), None, ("linear", "energy")


def torso_arm():
    return rg.torso(), {"rot": rg.tilted(0.15), "origin": np.array([0.1, -0.05, -0.4])}, tuple(range(8, 15)), ("angular", "linear")


def squared(limits, B):
    """[B, 3] = (p_max^2, L_max^2, 2 E_max) of physical limits {kind: [B]}: what the kernel divides; +inf where none is given."""
    lim = np.full((B, 3), np.inf)
    for kind, value in limits.items():
        k = KINDS.index(kind)
        lim[:, k] = 2.0 * value if kind == "energy" else value * value
    return lim


def fixture(name, B, N, seed, make):
    rng = np.random.default_rng(seed)
    robot, mount, links, kinds = make()
    d = len(robot["parent"])
    p = rg.draw_paths(rng, B, d, N, 0.5 if d > 8 else 1.0)
    ref = mc.reference_of(robot, mount, p.q, p.qs, links)
    h, e2 = ref["momentum"], ref["energy2"]
    free = rg.free_solutions(p)  # each quantity's peak along the solution without the constraint, in physical units
    peak = {"linear": np.array([np.max(np.sqrt((h[b, :, :3] ** 2).sum(-1)) * sd) for b, (_, sd) in enumerate(free)]),
            "angular": np.array([np.max(np.sqrt((h[b, :, 3:] ** 2).sum(-1)) * sd) for b, (_, sd) in enumerate(free)]),
            "energy": np.array([np.max(0.5 * e2[b] * sd * sd) for b, (_, sd) in enumerate(free)])}
    vel_high = sor.velocity_box(p.qs, p.vlim)[1][..., 1]
    fraction = 0.9
    while True:
        limits = {kind: fraction * peak[kind] * (1.0 + 0.1 * np.arange(B) / B) for kind in kinds}  # (per trajectory: no two alike)
        lim = squared(limits, B)
        xb = mr.xbound(h, e2, lim)
        rec, _ = rg.solve_reference(name, p, lambda b: bound_only(rg.reference().constraint, None, xb[b]), rows=False)
        active = [int(np.sum((rec["K"][b, :, 1] == xb[b, :, 1]) & (xb[b, :, 1] < vel_high[b]))) for b in range(B)]
        print("%s: fraction %.3f of the peak -> the bound is active at %s of %d stages" % (name, fraction, active, N + 1))
        if min(active) >= (N + 1 + 3) // 4:
            break
        fraction *= 0.85
        assert fraction > 0.05, "%s: the bound never becomes active at a quarter of the stages" % name
    assert all(4 * a >= N + 1 for a in active)
    rg.assert_active(name, rec["sd"], free)
    rec["active"] = np.array(active, dtype=np.int32)

    # the restatement: the box made from (disturbed) momentum and energy2 over the rows of the joint limits alone
    rows = sor.dense_problem(p.coef, p.breaks, p.grid, p.vlim, p.alim, True, [])

    def capped(terms):
        cap = mr.xbound(terms["momentum"], terms["energy2"], lim)[..., 1]
        high = rows["high"].copy()
        high[..., 1] = np.where(high[..., 1] < cap, high[..., 1], cap)  # (dbl_min with the running value first, as the fold spells it)
        return high
    terms = {k: ref[k] for k in NAMES}
    assert np.array_equal(capped(terms), rec["high"]) and np.array_equal(rows["low"], rec["low"]), "the restated boxes differ"
    attached = {"mount_" + k: np.asarray(mount[k], dtype=np.float64) for k in ("rot", "origin")}
    attached.update({"limit_" + kind: limits[kind] for kind in kinds}, links=np.array(mr.link_set(robot, links), dtype=np.int32))
    return rg.finish(name, p, rec, lambda t: orc.solve_dense_batch(rows["a"], rows["b"], rows["c"], rows["low"], capped(t), rows["deltas"]),
                     terms, NAMES, ref, True, robot, rg.ROBOT_KEYS, attached,
                     dict(limit=lim, momentum=h, energy2=e2, momentum_mag=ref["momentum_mag"], energy2_mag=ref["energy2_mag"], xbound=xb),
                     fraction_of_peak=fraction)


if __name__ == "__main__":
    fixtures = {"momentum_d6_N40": fixture("momentum_d6_N40", 4, 40, 811, chain6),
                "momentum_torso_d15_N30": fixture("momentum_torso_d15_N30", 4, 30, 812, torso_arm)}
    rg.write_profile("momentum", "float64 tests/momentum_ref.py", mc.accuracy_table(), fixtures)

"""Retime paths of a 7-dof collaborative arm that works next to an operator, under a cap on the energy a contact can transfer
(ISO/TS 15066, power and force limiting) -- once as a cap on the arm's TOTAL kinetic energy, which is what bounds the transferred
energy for every contact point and direction at once, and once as the cap at the two points that can actually meet the operator:
the elbow and the tool point, through the arm's effective (reflected) mass there.  Both use the same E_max; the per-point limit
is never slower, because the total energy is the upper envelope of what any one point can transfer (Cauchy-Schwarz), and on an
arm with more than two joints it is much faster.

    1 / m_R = u' J M(q)^-1 J' u          the arm's mobility at the point along the contact direction u (here: the point's velocity)
    E = 1/2 mu v^2,  mu = (1 / m_body + 1 / m_R)^-1

The energy is in J and the body masses in kg (the class doubles and inverts on the host); no table of body regions is shipped:
``from_force`` turns a region's force limit and stiffness into its energy, E = F^2 / (2 k).

    python examples/contact_limits.py [--batch 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import toppra_amd as ta  # noqa: E402


def arm():
    """The arm of examples/cobot_limits.py, without the workpiece: 12 kg of links, a heavy forearm, thin-rod inertias."""
    axes = np.array([[0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1]], dtype=float)
    offsets = np.array([[0, 0, 0.35], [0, 0, 0], [0, 0, 0], [0.045, 0, 0.55], [-0.045, 0, 0.3], [0, 0, 0], [0, 0, 0.06]])
    masses = np.array([3.0, 2.5, 2.0, 2.5, 1.0, 0.6, 0.4])
    coms = np.array([[0, 0, -0.1], [0, 0, 0.2], [0, 0, 0.4], [0, 0, 0.15], [0, 0, 0.2], [0, 0, 0.02], [0, 0, 0.03]])
    inertias = np.stack([np.array([0.02, 0.02, 0.004, 0, 0, 0]) * m for m in masses])
    return ta.SerialChain(["revolute"] * 7, axes, np.stack([np.eye(3)] * 7), offsets, masses, coms, inertias, tool=(0, 0, 0.12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    B = ap.parse_args().batch
    np.random.seed(9)
    chain, d, N = arm(), 7, 100
    points = ta.ControlPoints([3, -1], [[0.0, 0.0, 0.0], chain.tool])  # the elbow, the tool point
    waypoints = np.random.randn(B, 5, d) * 0.6
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    vlim = np.tile([-2.0, 2.0], (B, d, 1))
    alim = np.tile([-8.0, 8.0], (B, d, 1))
    e_max = 0.5  # J, at both points; the body part is clamped (1 / m_body = 0): the case the total energy is compared with

    total = ta.BatchMomentumConstraint(chain, energy=e_max)
    per_point = ta.BatchContactEnergyConstraint(chain, points, e_max)
    make = lambda cons: ta.algorithm.BatchTOPPRA.from_waypoints(knots, waypoints, grid, vlim, alim, **({"constraints": cons} if cons else {}))  # noqa: E731
    runs = {"total kinetic energy": make([total]), "energy at the two points": make([per_point]), "joint limits alone": make([])}
    pe = ta.batch.path_eval_batch(runs["joint limits alone"].coef, runs["joint limits alone"].breaks, grid)
    dur = {}
    for label, bt in runs.items():
        out = bt.compute_parameterization()
        assert np.all(out["status"] == 0), label
        qd = pe["qs"] * out["sd"][..., None]
        at_points = chain.contact_energy(pe["q"], qd, points)
        whole = chain.kinetic_energy(pe["q"], qd)
        dur[label] = bt.compute_trajectory().duration
        print("%-25s mean duration %.3f s; largest energy at the elbow %.3f J, at the tool %.3f J, of the whole arm %.3f J (cap %.1f J)"
              % (label, dur[label].mean(), at_points[..., 0].max(), at_points[..., 1].max(), whole.max(), e_max))
        if label != "joint limits alone":
            assert at_points.max() <= e_max * (1 + 1e-9)  # the total-energy limit holds the points too: their upper envelope
        if label == "total kinetic energy":
            assert whole.max() <= e_max * (1 + 1e-9)
    # the effective mass the operator meets, and how much of the total energy a point can transfer
    m_eff = chain.effective_mass(pe["q"], pe["qs"], points)
    share = chain.contact_energy(pe["q"], pe["qs"], points) / chain.kinetic_energy(pe["q"], pe["qs"])[..., None]
    print("effective mass along the path: elbow %.2f .. %.2f kg, tool %.2f .. %.2f kg (the links weigh %.1f kg)"
          % (np.nanmin(m_eff[..., 0]), np.nanmax(m_eff[..., 0]), np.nanmin(m_eff[..., 1]), np.nanmax(m_eff[..., 1]), chain.masses.sum()))
    print("a point carries %.0f .. %.0f %% of the arm's kinetic energy" % (100 * np.nanmin(share), 100 * np.nanmax(share)))
    assert np.nanmax(share) <= 1.0 + 1e-9
    a, b = dur["energy at the two points"], dur["total kinetic energy"]
    print("the per-point limit is faster on %d of %d paths, by %.1f %% on average" % (int((a < b).sum()), B, 100.0 * (1.0 - (a / b).mean())))
    assert np.all(a <= b * (1 + 1e-9)) and (a < b).any()
    # a body region by its force limit and stiffness (the user's numbers): 140 N on 75 N / mm, a free 40 kg trunk
    region = ta.BatchContactEnergyConstraint.from_force(chain, points, force=140.0, stiffness=75e3, body_mass=40.0)
    out = make([region]).compute_parameterization()
    qd = pe["qs"] * out["sd"][..., None]
    print("a 140 N / 75 N/mm region (%.3f J) against a 40 kg body part: largest contact energy %.3f J"
          % (float(region.energy), chain.contact_energy(pe["q"], qd, points, 40.0).max()))
    assert np.all(out["status"] == 0) and chain.contact_energy(pe["q"], qd, points, 40.0).max() <= float(region.energy) * (1 + 1e-9)


if __name__ == "__main__":
    main()

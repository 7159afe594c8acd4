#!/usr/bin/env python
"""Generate tests/golden/path_*.npz: the REAL reference (hungpham2511/toppra, seidel solver) on geometric paths that are not
cubic splines -- SimplePath, PolynomialPath, UnivariateSplineInterpolator and a hand-written trigonometric path.

    python tools/make_golden_paths.py        # build container only: needs the reference, builds oracle/_ref on demand

Each fixture stores the gridpoints, the samples q, qs, qss exactly as the reference's path object returned them, the limits, the
discretisation, and the reference's results: controllable sets K_set for one (sdmin, sdmax), feasible sets X, reachable sets L,
the parameterization (sd, u, K, status) for (0, 0) and for one nonzero boundary pair, a TOPPRAsd result, and both parametrizers'
duration and q / qd / qdd at 32 times.  Every result comes from a fresh reference object, like a fresh library call.  The tests
feed the STORED samples to the kernels, so another scipy on the test machine cannot leak into a comparison with stored bits.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

from oracle import ref_loader  # noqa: E402
from tests import sampled_ref  # noqa: E402

ta = ref_loader.load()
if ta is None:
    raise SystemExit("reference not available")
import toppra.algorithm as algo  # noqa: E402
import toppra.constraint as constraint  # noqa: E402
import toppra.parametrizer as tparam  # noqa: E402
from toppra.algorithm.algorithm import ParameterizationReturnCode as RC  # noqa: E402

STATUS = {RC.Ok: 0, RC.FailUncontrollable: 1, RC.ErrUnknown: 2}


def fixture(name, spec, grid, vlim, alim, interpolation, sets=(0.0, 1.0), pair=(0.5, 0.25), bad_pair=None):
    path = sampled_ref.make_path(spec, ta)
    grid = np.asarray(grid, dtype=np.float64)
    N = len(grid) - 1
    scheme = 1 if interpolation else 0

    def inst(cls=algo.TOPPRA):
        cons = [constraint.JointVelocityConstraint(vlim), constraint.JointAccelerationConstraint(alim, discretization_scheme=scheme)]
        return cls(cons, path, gridpoints=grid, solver_wrapper="seidel")

    rec = dict(spec)
    shape = (N + 1, path.dof)
    rec.update(grid=grid, vlim=np.asarray(vlim, dtype=np.float64), alim=np.asarray(alim, dtype=np.float64),
               interpolation=np.array(interpolation), q=np.asarray(path(grid), dtype=np.float64).reshape(shape),
               qs=np.asarray(path(grid, 1), dtype=np.float64).reshape(shape),
               qss=np.asarray(path(grid, 2), dtype=np.float64).reshape(shape), sets=np.array(sets), pair=np.array(pair))
    rec["K_set"] = inst().compute_controllable_sets(*sets)
    rec["X"] = inst().compute_feasible_sets()
    rec["L"] = inst().compute_reachable_sets(*sets)
    pairs = [("zero", (0.0, 0.0)), ("pair", pair)] + ([("bad", bad_pair)] if bad_pair else [])
    traj_sd = None
    for tag, (s0, s1) in pairs:
        obj = inst()
        sdd, sd, _, K = obj.compute_parameterization(s0, s1, return_data=True)
        st = STATUS[obj.problem_data.return_code]
        if sd is None:
            sd, sdd = np.full(N + 1, np.nan), np.full(N, np.nan)
        elif traj_sd is None and st == 0:
            traj_sd = sd
        rec.update({tag + "_sd": sd, tag + "_u": sdd, tag + "_K": K, tag + "_status": np.array(st)})
    if bad_pair:
        rec["bad_pair"] = np.array(bad_pair)
    if traj_sd is not None:
        # TOPPRAsd: half again as long as the time-optimal duration, from the same boundary velocities as the first Ok solve
        s0, s1 = (0.0, 0.0) if rec["zero_status"] == 0 else pair
        t_opt = tparam.ParametrizeConstAccel(path, grid, traj_sd).duration
        obj = inst(algo.TOPPRAsd)
        obj.set_desired_duration(1.5 * t_opt)
        sdd, sd, _, K = obj.compute_parameterization(s0, s1, return_data=True)
        rec.update(sd_desired=np.array(1.5 * t_opt), sd_pair=np.array([s0, s1]), sd_sd=sd, sd_u=sdd, sd_K=K,
                   sd_status=np.array(STATUS[obj.problem_data.return_code]))
        rec["traj_sd"] = traj_sd
        for tag, cls in (("spline", tparam.ParametrizeSpline), ("accel", tparam.ParametrizeConstAccel)):
            traj = cls(path, grid, traj_sd)
            ts = np.linspace(0, traj.duration, 32)
            rec.update({tag + "_duration": np.array(traj.duration), tag + "_ts": ts, tag + "_q": traj(ts),
                        tag + "_qd": traj(ts, 1), tag + "_qdd": traj(ts, 2)})
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **rec)
    print("%-40s N %3d d %2d  status zero / pair / sd: %s / %s / %s%s" % (
        name, N, path.dof, rec["zero_status"], rec["pair_status"], rec.get("sd_status"),
        "  bad: %s" % rec["bad_status"] if bad_pair else ""))


def limits(rng, d, v=(1.0, 2.0), a=(2.0, 3.0)):
    vmax, amax = v[0] + v[1] * rng.random(d), a[0] + a[1] * rng.random(d)
    return np.stack([-vmax, vmax], -1), np.stack([-amax, amax], -1)


def main():
    rng = np.random.default_rng(20241018)
    # SimplePath, 3 dof, N 40: without and with yd (the second on a non-uniform grid, with an uncontrollable start)
    x = np.array([0.0, 0.3, 0.55, 0.8, 1.0])
    y = rng.standard_normal((5, 3))
    vl, al = limits(rng, 3)
    fixture("path_simple_d3_N40", {"kind": "simple", "path_x": x, "path_y": y}, np.linspace(0, 1, 41), vl, al, True)
    yd = rng.standard_normal((5, 3))
    g = np.sort(np.concatenate(([0.0, 1.0], rng.random(39))))
    fixture("path_simple_yd_d3_N40", {"kind": "simple", "path_x": x, "path_y": y, "path_yd": yd}, g, vl, al, True,
            bad_pair=(50.0, 0.0))
    # PolynomialPath of degree 5, 2 dof, N 60
    vl, al = limits(rng, 2)
    fixture("path_poly5_d2_N60", {"kind": "poly", "path_coeff": rng.standard_normal((2, 6))}, np.linspace(0, 1, 61), vl, al, True)
    # UnivariateSplineInterpolator, 4 dof, N 40
    xs = np.linspace(0, 1, 12)
    vl, al = limits(rng, 4)
    fixture("path_uspl_d4_N40", {"kind": "uspl", "path_x": xs, "path_y": np.cumsum(0.3 * rng.standard_normal((12, 4)), axis=0)},
            np.linspace(0, xs[-1], 41), vl, al, True)
    # the trigonometric path: one shape per lane-group width and the row limits of both discretisations
    for d in (9, 17, 30):
        vl, al = limits(rng, d, (2.0, 2.0), (4.0, 4.0))
        for interp in (True, False):
            fixture("path_trig_d%d_N30_%s" % (d, "interp" if interp else "colloc"),
                    {"kind": "trig", "trig_dof": np.array(d), "trig_seed": np.array(100 + d), "trig_slope": np.array(0.0)},
                    np.linspace(0, 1, 31), vl, al, interp)
    vl, al = limits(rng, 32, (2.0, 2.0), (4.0, 4.0))
    fixture("path_trig_d32_N30_colloc", {"kind": "trig", "trig_dof": np.array(32), "trig_seed": np.array(132), "trig_slope": np.array(0.0)},
            np.linspace(0, 1, 31), vl, al, False)
    # a velocity range that excludes 0: every joint moves forward (slope 8 > amp w), so sd has a positive lower bound
    vl, al = limits(rng, 3, (8.0, 4.0), (30.0, 10.0))
    vl[:, 0] = 0.5 + rng.random(3)
    fixture("path_trig_d3_N30_vpos", {"kind": "trig", "trig_dof": np.array(3), "trig_seed": np.array(7), "trig_slope": np.array(8.0)},
            np.linspace(0, 1, 31), vl, al, True, sets=(0.5, 0.75), pair=(0.5, 0.5))


if __name__ == "__main__":
    main()

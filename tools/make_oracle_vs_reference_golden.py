#!/usr/bin/env python
"""Generate tests/golden/oracle_vs_reference_*.npz by running the REAL reference (hungpham2511/toppra, seidel solver) on
the problems that tests/test_oracle_vs_reference.py generates.  The reference cannot travel with the repository, so
its outputs on those problems are committed as fixtures; this script is their provenance.

    python tools/make_oracle_vs_reference_golden.py    # needs the reference sources; builds oracle/_ref on demand

Keys are '<case>__<trial>__<name>' (tests/test_oracle_vs_reference.py::reference_outputs).  A trajectory the reference
declares FailUncontrollable (it returns None) is stored with failed = 1 and no sd / sdd.

Fixtures: parameterization, irregular, lp2d, velocity_bound, reachable, host_glue, general, and extreme (limits at the edge of
the number range: tests/test_oracle_vs_reference.py::extreme_limit_problems; one stacked array per name and case, trial
'all', failed trajectories NaN-filled, and the reference's own velocity bound at every gridpoint beside K, X, sd, sdd).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import test_oracle_vs_reference as T  # noqa: E402

reference = ref_loader.load()
if reference is None:
    raise SystemExit("reference not available")
import toppra.algorithm as algo  # noqa: E402
import toppra.constraint as constraint  # noqa: E402


def put(out, case, trial, **arrays):
    for name, v in arrays.items():
        out["%s__%s__%s" % (case, trial, name)] = np.asarray(v)


def profile(rec, sdd, sdv):
    rec["failed"] = int(sdv is None)
    if sdv is not None:
        rec["sd"], rec["sdd"] = sdv, sdd
    return rec


def parameterization():
    out = {}
    for d, N, scheme, sd in T.PARAMETERIZATION_CASES:
        for t, (knots, grid, way, vl, al) in enumerate(T.parameterization_problems(d, N)):
            path = reference.SplineInterpolator(knots, way)
            cons = [constraint.JointVelocityConstraint(vl),
                    constraint.JointAccelerationConstraint(al, discretization_scheme=scheme)]
            inst = algo.TOPPRA(cons, path, gridpoints=grid, solver_wrapper="seidel")
            sdd, sdv, _, K = inst.compute_parameterization(sd[0], sd[1], return_data=True)
            X = algo.TOPPRA(cons, path, gridpoints=grid, solver_wrapper="seidel").compute_feasible_sets()
            rec = profile({"c": path.cspl.c, "x": path.cspl.x, "K": K, "X": X,
                           "stages": inst.solver_wrapper.get_no_stages()}, sdd, sdv)
            put(out, T.case_id(d, N, scheme, *sd), t, **rec)
    return out


def irregular():
    out = {}
    for d, N, nway, seed in T.IRREGULAR_CASES:
        for t, (knots, grid, way, vl, al, sd0, sd1) in enumerate(T.irregular_problems(d, N, nway, seed)):
            path = reference.SplineInterpolator(knots, way)
            cons = [constraint.JointVelocityConstraint(vl), constraint.JointAccelerationConstraint(al)]
            inst = algo.TOPPRA(cons, path, gridpoints=grid, solver_wrapper="seidel")
            sdd, sdv, _, K = inst.compute_parameterization(sd0, sd1, return_data=True)
            put(out, T.case_id(d, N, nway, seed), t, **profile({"c": path.cspl.c, "x": path.cspl.x, "K": K}, sdd, sdv))
    return out


def lp2d():
    import toppra.solverwrapper.cy_seidel_solverwrapper as seidel
    out = {}
    for t, (v, a, b, c, low, high, ac) in enumerate(T.lp2d_problems()):
        result, optval, optvar, active_c = seidel.solve_lp2d(v, a, b, c, low, high, ac.astype(int))
        put(out, "all", t, result=int(result), optval=optval, optvar=list(optvar), active_c=list(active_c))
    return out


def velocity_bound():
    from toppra._CythonUtils import _create_velocity_constraint
    qs, vlim = T.velocity_bound_problem()
    _, _, cc = _create_velocity_constraint(qs, vlim)
    out = {}
    put(out, "all", 0, xbound=np.stack([cc[:, 1], -cc[:, 0]], 1))
    return out


def reachable():
    out = {}
    for d, N, scheme, sds in T.REACHABLE_CASES:
        for t, (knots, grid, way, vl, al) in enumerate(T.reachable_problems(d, N)):
            path = reference.SplineInterpolator(knots, way)
            cons = [constraint.JointVelocityConstraint(vl),
                    constraint.JointAccelerationConstraint(al, discretization_scheme=scheme)]
            inst = algo.TOPPRA(cons, path, gridpoints=grid, solver_wrapper="seidel")
            L = inst.compute_reachable_sets(*sds)
            put(out, T.case_id(d, N, scheme, *sds), t, c=path.cspl.c, x=path.cspl.x, L=L, X=inst.problem_data.X)
    return out


def host_glue():
    import toppra.interpolator as ri
    import toppra.parametrizer as rp
    out = {}
    for t, way, kw, rng in T.host_glue_problems():
        path = reference.SplineInterpolator(np.linspace(0, 1, len(way)), way)
        grid = np.array(ri.propose_gridpoints(path, **kw))
        sd = T.host_glue_sd(rng, len(grid), t)
        p = rp.ParametrizeSpline(path, grid, sd)
        # (the coefficient tables as a digest of their bytes: 4 MB of doubles otherwise)
        put(out, "all", t, grid=grid, x=p.cspl.x, c_shape=np.shape(p.cspl.c), c_sha256=T.array_digest(p.cspl.c))
    return out


def general():
    from toppra_amd.solverwrapper import dense_rows
    out = {}
    for scheme in T.GENERAL_CASES:
        for trial, d, way, inv_dyn, taulim, fric, vfun in T.general_problems(scheme):
            path = reference.SplineInterpolator(T.GENERAL_KNOTS, way)
            cons = T.general_constraint_lists(constraint, scheme, inv_dyn, taulim, fric, vfun)
            rows = dense_rows(cons, path, T.GENERAL_GRID)
            sd0, sd1 = (0.0, 0.0) if trial % 2 else (0.1, 0.05)
            inst = algo.TOPPRA(cons, path, gridpoints=T.GENERAL_GRID, solver_wrapper="seidel")
            sdd, sdv, _, K = inst.compute_parameterization(sd0, sd1, return_data=True)
            X = algo.TOPPRA(cons, path, gridpoints=T.GENERAL_GRID, solver_wrapper="seidel").compute_feasible_sets()
            rec = profile({"K": K, "X": X}, sdd, sdv)
            rec.update({"rows_" + k: rows[k] for k in ("a", "b", "c", "low", "high", "deltas")})
            put(out, T.case_id(scheme), trial, **rec)
    return out


def extreme():
    from toppra._CythonUtils import _create_velocity_constraint
    out = {}
    for d, N, seed in T.EXTREME_CASES:
        recs = []
        for kind, knots, grid, way, vl, al, sd0, sd1 in T.extreme_limit_problems(d, N, seed):
            path = reference.SplineInterpolator(knots, way)
            cons = [constraint.JointVelocityConstraint(vl), constraint.JointAccelerationConstraint(al)]
            inst = algo.TOPPRA(cons, path, gridpoints=grid, solver_wrapper="seidel")
            sdd, sdv, _, K = inst.compute_parameterization(sd0, sd1, return_data=True)
            X = algo.TOPPRA(cons, path, gridpoints=grid, solver_wrapper="seidel").compute_feasible_sets()
            _, _, cc = _create_velocity_constraint(path(grid, 1).reshape(N + 1, d), vl)
            failed = sdv is None
            recs.append({"c": path.cspl.c, "x": path.cspl.x, "K": K, "X": X, "failed": int(failed),
                         "sd": np.full(N + 1, np.nan) if failed else sdv, "sdd": np.full(N, np.nan) if failed else sdd,
                         "xbound": np.stack([cc[:, 1], -cc[:, 0]], 1)})
        put(out, T.case_id(d, N, seed), "all", **{k: np.stack([np.asarray(r[k]) for r in recs]) for k in recs[0]})
    return out


if __name__ == "__main__":
    only = sys.argv[1:]
    for name, fn in (("parameterization", parameterization), ("irregular", irregular), ("lp2d", lp2d),
                     ("velocity_bound", velocity_bound), ("reachable", reachable), ("host_glue", host_glue), ("general", general),
                     ("extreme", extreme)):
        if only and name not in only:
            continue
        arrays = fn()
        np.savez_compressed(T.golden_path(name), **arrays)
        print("%s: %d arrays, %d bytes" % (T.golden_path(name), len(arrays), os.path.getsize(T.golden_path(name))))

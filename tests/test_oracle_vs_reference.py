"""Pinning of the CPU oracle against the REAL reference on fresh seeds, bit-exact.  The problems are generated here
(the functions below; those with limits at the edge of the number range, which the GPU tests run as well, in
tests/solver_support.py); the reference's outputs on exactly these problems are stored in
tests/golden/oracle_vs_reference_*.npz by tools/make_oracle_vs_reference_golden.py, which runs the reference on
them -- so the pin holds wherever the suite runs, the reference itself being absent there."""
import functools
import hashlib

import numpy as np
import pytest

from tests.helpers import assert_same, torque_model
from tests.solver_support import (EXTREME_CASES, EXTREME_KINDS, FLT_MAX, FLT_MIN_NORMAL, case_id, extreme_limit_batch,  # noqa: F401
                                  extreme_limit_problems, golden_path, oracle_flags, ordinary_problem as _problem, reference_outputs)
# (noqa: tools/make_oracle_vs_reference_golden.py and tools/host_cert_hunt.py read the generators and the fixture's path here)

PARAMETERIZATION_CASES = [(7, 200, 1, (0, 0)), (6, 500, 1, (0, 0)), (3, 60, 0, (0.1, 0.05)), (2, 40, 1, (3.0, 0.0)), (5, 77, 1, (0, 0.2))]
IRREGULAR_CASES = [(6, 90, 9, 1), (7, 120, 6, 2), (9, 50, 7, 3), (14, 40, 5, 4), (3, 150, 4, 5)]
REACHABLE_CASES = [(7, 100, 1, (0.0, 0.0)), (5, 60, 1, (0.0, 0.3)), (3, 40, 0, (0.1, 0.4)), (6, 80, 1, (0.5, 0.5))]
GENERAL_CASES = [0, 1]


# ---- the problems (shared with tools/make_oracle_vs_reference_golden.py) ----

def parameterization_problems(d, N):
    """12 x (knots, grid, waypoints, vlim, alim)."""
    rng = np.random.default_rng(d * 1000 + N)
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    for _ in range(12):
        yield (knots, grid) + _problem(rng, d)


def irregular_problems(d, N, nway, seed):
    """Asymmetric limits incl. positive lower velocity limits, joints that stand still, non-uniform knots and grids,
    non-zero boundary velocities: 10 x (knots, grid, waypoints, vlim, alim, sd_start, sd_end)."""
    rng = np.random.default_rng(9000 + seed)
    knots = np.concatenate([[0.0], np.sort(rng.random(nway - 2)) * 0.9 + 0.05, [1.0]])
    grid = 0.6 * np.concatenate([[0.0], np.sort(rng.random(N - 1)), [1.0]]) + 0.4 * np.linspace(0, 1, N + 1)
    for _ in range(10):
        way = rng.standard_normal((nway, d))
        still = rng.random(d) < 0.15
        way = np.where(still[None, :], way[:1, :], way)
        vhi = 5 + 25 * rng.random(d); vlo = -(5 + 25 * rng.random(d))
        vlo = np.where(rng.random(d) < 0.05, 0.05 * rng.random(d), vlo)
        ahi = 5 + 10 * rng.random(d); alo = -(5 + 10 * rng.random(d))
        vl, al = np.stack([vlo, vhi], 1), np.stack([alo, ahi], 1)
        sd0 = 0.3 * rng.random() if rng.random() < 0.5 else 0.0
        sd1 = 0.3 * rng.random() if rng.random() < 0.5 else 0.0
        yield knots, grid, way, vl, al, sd0, sd1


def lp2d_problems():
    """300 x (v, a, b, c, low, high, active_c)."""
    for seed in range(300):
        rng = np.random.default_rng(seed + 5000)
        n = int(rng.integers(1, 60))
        v = rng.standard_normal(3)
        a, b = rng.standard_normal((2, n))
        c = -rng.random(n) if seed % 2 == 0 else rng.standard_normal(n)
        low, high = np.array([-0.5, -0.9]), np.array([0.5, 0.9])
        ac = rng.integers(-1, n + 1, size=2)
        yield v, a, b, c, low, high, ac


def velocity_bound_problem():
    """(path velocities qs [500, 7], vlim [7, 2]): zero rows, and a positive lower limit (the sdmin branch)."""
    rng = np.random.default_rng(3)
    qs = rng.standard_normal((500, 7))
    qs[::17] = 0.0
    vmax = 10 + 20 * rng.random(7)
    vlim = np.stack([-vmax, 0.5 * vmax + rng.random(7)], 1)
    vlim[3] = [0.5, 2.0]
    return qs, vlim


def reachable_problems(d, N):
    """8 x (knots, grid, waypoints, vlim, alim) on a non-uniform grid (deltas[i-1] != deltas[i])."""
    rng = np.random.default_rng(77 * d + N)
    knots = np.linspace(0, 1, 5)
    grid = np.concatenate([[0.0], np.sort(rng.random(N - 1)), [1.0]])
    grid = 0.5 * grid + 0.5 * np.linspace(0, 1, N + 1)
    for _ in range(8):
        yield (knots, grid) + _problem(rng, d)


def host_glue_problems():
    """20 x (t, waypoints, propose_gridpoints keywords, rng); host_glue_sd(rng, ...) draws the trial's sd from the same
    stream once the grid's length is known."""
    rng = np.random.default_rng(0)
    for t in range(20):
        d, m = int(rng.integers(1, 8)), int(rng.integers(3, 9))
        way = rng.standard_normal((m, d)) * float(rng.choice([0.1, 1, 5]))
        kw = dict(max_err_threshold=float(rng.choice([1e-4, 1e-3, 1e-5])), max_seg_length=float(rng.choice([0.05, 0.02, 0.2])),
                  min_nb_points=int(rng.choice([100, 30, 250])))
        yield t, way, kw, rng


def array_digest(a):
    """SHA-256 of an array's float64 bytes (C order): bit-for-bit equality of tables too large to store."""
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def host_glue_sd(rng, n, t):
    sd = np.abs(rng.standard_normal(n))
    sd[0] = sd[-1] = 0
    if t % 3 == 0:
        sd[5:8] = 0  # a standing stretch (the 5 s rule)
    return sd


def general_problems(scheme):
    """6 x (d, waypoints, inverse dynamics, torque limits, friction, varying velocity limits) on 40 stages."""
    rng = np.random.default_rng(40 + scheme)
    for trial in range(6):
        d = int(rng.integers(2, 7))
        way = rng.standard_normal((5, d))
        inv_dyn = torque_model(1 + rng.random(d), 0.5 * rng.standard_normal(d), 0.3 * rng.standard_normal(d))
        taulim = np.stack([-6 - 6 * rng.random(d), 6 + 6 * rng.random(d)], axis=1)
        fric = 0.1 * rng.random(d)
        base = np.stack([-10 - 5 * rng.random(d), 10 + 5 * rng.random(d)], axis=1)
        vfun = lambda s, base=base: base * (1 + 0.4 * np.sin(5 * s))  # noqa: E731
        yield trial, d, way, inv_dyn, taulim, fric, vfun


GENERAL_KNOTS, GENERAL_GRID = np.linspace(0, 1, 5), np.linspace(0, 1, 41)


def general_constraint_lists(mod, scheme, inv_dyn, taulim, fric, vfun):
    DT = mod.DiscretizationType(scheme)
    return [mod.JointVelocityConstraintVarying(vfun), mod.JointTorqueConstraint(inv_dyn, taulim, fric, discretization_scheme=DT),
            mod.SecondOrderConstraint.joint_torque_constraint(inv_dyn, 1.3 * taulim, fric, discretization_scheme=DT)]


# ---- the oracle against the reference's outputs (tests/solver_support.py::reference_outputs) ----

@pytest.mark.parametrize("d,N,scheme,sd", PARAMETERIZATION_CASES)
def test_parameterization_matches_reference(oracle, d, N, scheme, sd):
    flags = oracle_flags(oracle, True, bool(scheme))
    for t, (knots, grid, way, vl, al) in enumerate(parameterization_problems(d, N)):
        ref = reference_outputs("parameterization", case_id(d, N, scheme, *sd), t)
        # the reference's own spline tables (path.cspl.c / .x) are the oracle's input
        w = oracle.Wrapper(ref["c"], ref["x"], grid, vl, al, flags=flags)
        st, osdd, osd, oxs, oK = w.compute_parameterization(*sd)
        assert_same(oK, ref["K"], "K")
        if ref["failed"]:
            assert st == 1
        else:
            assert_same(osd, ref["sd"], "sd")
            assert_same(osdd, ref["sdd"], "sdd")
        # wrapper internals: the feasible sets (dense rows and the variable box) and the stage count
        w2 = oracle.Wrapper(ref["c"], ref["x"], grid, vl, al, flags=flags)
        assert_same(w2.compute_feasible_sets(), ref["X"], "X")
        assert int(ref["stages"]) == N


@pytest.mark.parametrize("d,N,nway,seed", IRREGULAR_CASES)
def test_irregular_problems_match_reference(oracle, d, N, nway, seed):
    """Asymmetric limits incl. positive lower velocity limits, joints that stand still, non-uniform knots
    and grids, non-zero boundary velocities, up to 14 dof: the oracle against the reference."""
    seen = set()
    for t, (knots, grid, way, vl, al, sd0, sd1) in enumerate(irregular_problems(d, N, nway, seed)):
        ref = reference_outputs("irregular", case_id(d, N, nway, seed), t)
        w = oracle.Wrapper(ref["c"], ref["x"], grid, vl, al)
        st, osdd, osd, oxs, oK = w.compute_parameterization(sd0, sd1)
        assert_same(oK, ref["K"], "K")
        seen.add(st)
        if ref["failed"]:
            assert st == 1
        else:
            assert_same(osd, ref["sd"], "sd")
            assert_same(osdd, ref["sdd"], "sdd")
    assert 0 in seen


@functools.lru_cache(maxsize=None)
def extreme_fixture_census():
    """What the REFERENCE's stored outputs hold, over the whole fixture: (non-zero fp32 subnormal upper bounds of `vsub`, its
    exact zeros, quotients |vlim / q'| beyond FLT_MAX of `vhuge`, gridpoints of `vneg` with a positive lower bound)."""
    from scipy.interpolate import PPoly
    sub = zero = beyond = pos_lower = 0
    for d, N, seed in EXTREME_CASES:
        ref = reference_outputs("extreme", case_id(d, N, seed), "all")
        for t, (kind, knots, grid, way, vl, al, sd0, sd1) in enumerate(extreme_limit_problems(d, N, seed)):
            lo, hi = ref["xbound"][t][:, 0], ref["xbound"][t][:, 1]
            if kind == "vsub":
                sub += int(np.sum((hi > 0) & (hi < FLT_MIN_NORMAL)))
                zero += int(np.sum(hi == 0))
            elif kind == "vhuge":
                qs = PPoly(ref["c"][t], ref["x"][t]).derivative()(grid)  # the reference's path(grid, 1): scipy on its own table
                with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
                    beyond += int(np.sum(np.abs(vl[None, :, :] / qs[:, :, None]) > FLT_MAX))
            elif kind == "vneg":
                pos_lower += int(np.sum(lo > 0))
    return sub, zero, beyond, pos_lower


@pytest.mark.parametrize("d,N,seed", EXTREME_CASES)
def test_extreme_limits_match_reference(oracle, d, N, seed):
    """Infinite, huge, subnormal-squared, one-sided and inverted limits, standing joints, shifted path parameters: the
    oracle against the reference bit for bit -- K, the feasible sets, sd, sdd, failures, and the fp32 velocity bound against
    the reference's own _create_velocity_constraint at every gridpoint.  The conditions at the end are on the REFERENCE's
    stored outputs: every kind but `inverted` and `vneg` is solved at least once in every case, `inverted` never, and the
    fixture does hold subnormal and underflowed bounds, quotients beyond FLT_MAX and positive lower bounds."""
    ref = reference_outputs("extreme", case_id(d, N, seed), "all")
    solved = {}
    for t, (kind, knots, grid, way, vl, al, sd0, sd1) in enumerate(extreme_limit_problems(d, N, seed)):
        c, x, what = ref["c"][t], ref["x"][t], " (%s, trial %d)" % (kind, t)
        assert not any(np.isnan(v).any() for v in (c, x, grid, vl, al))
        st, osdd, osd, oxs, oK = oracle.Wrapper(c, x, grid, vl, al).compute_parameterization(sd0, sd1)
        assert_same(oK, ref["K"][t], "K" + what)
        if ref["failed"][t]:
            assert st == 1, what
        else:
            assert st == 0, what
            assert_same(osd, ref["sd"][t], "sd" + what)
            assert_same(osdd, ref["sdd"][t], "sdd" + what)
        assert_same(oracle.Wrapper(c, x, grid, vl, al).compute_feasible_sets(), ref["X"][t], "X" + what)
        xb = np.array([oracle.velocity_xbound(oracle.path_eval(c, x, float(s))[0], vl) for s in grid])
        assert_same(xb, ref["xbound"][t], "xbound" + what)
        solved.setdefault(kind, []).append(not ref["failed"][t])
    assert set(solved) == set(EXTREME_KINDS)
    for kind, ok in solved.items():
        if kind == "inverted":
            assert not any(ok), kind
        elif kind != "vneg":
            assert any(ok), kind
    sub, zero, beyond, pos_lower = extreme_fixture_census()
    assert sub > 0 and zero > 0 and beyond > 0 and pos_lower > 0, (sub, zero, beyond, pos_lower)


def test_lp2d_matches_reference(oracle):
    for t, (v, a, b, c, low, high, ac) in enumerate(lp2d_problems()):
        want = reference_outputs("lp2d", "all", t)
        got = oracle.lp2d(v, a, b, c, low, high, ac)
        assert got[0] == want["result"]
        if want["result"]:
            assert got[1] == want["optval"] and list(got[2]) == list(want["optvar"]) and list(got[3]) == list(want["active_c"])


def test_velocity_bound_is_fp32(oracle):
    """The fp32 rounding of the velocity bound (SURVEY.md trap 1) is reproduced exactly."""
    qs, vlim = velocity_bound_problem()
    want = reference_outputs("velocity_bound", "all", 0)["xbound"]
    got = np.array([oracle.velocity_xbound(q, vlim) for q in qs])
    assert_same(got, want, "xbound")
    # and it is NOT what fp64 arithmetic would give
    assert np.any(got[:, 1] != np.array([np.min(np.where(q > 0, vlim[:, 1] / q, vlim[:, 0] / q)) ** 2
                                         for q in np.where(qs == 0, 1e-30, qs)]))


@pytest.mark.parametrize("d,N,scheme,sds", REACHABLE_CASES)
def test_reachable_sets_match_reference(oracle, d, N, scheme, sds):
    """compute_reachable_sets (reachability_algorithm.py:378-431) incl. its deltas[i-1] objective and the
    warm-start state carried over from the feasible-set pass it runs first."""
    flags = oracle_flags(oracle, True, bool(scheme))
    for t, (knots, grid, way, vl, al) in enumerate(reachable_problems(d, N)):
        ref = reference_outputs("reachable", case_id(d, N, scheme, *sds), t)
        w = oracle.Wrapper(ref["c"], ref["x"], grid, vl, al, flags=flags)
        oL, oX = w.compute_reachable_sets(*sds)
        assert_same(oL, ref["L"], "L")
        assert_same(oX, ref["X"], "X")


def test_host_glue_matches_reference():
    """propose_gridpoints and ParametrizeSpline (vectorised host code here, loops in the reference) give the
    reference's grids, knot times and spline coefficients value for value."""
    import toppra_amd as ta
    from toppra_amd.interpolator import propose_gridpoints
    for t, way, kw, rng in host_glue_problems():
        ref = reference_outputs("host_glue", "all", t)
        p1 = ta.SplineInterpolator(np.linspace(0, 1, len(way)), way)
        g1 = propose_gridpoints(p1, **kw)
        assert np.array_equal(np.array(g1), ref["grid"])
        sd = host_glue_sd(rng, len(g1), t)
        a = ta.ParametrizeSpline(p1, g1, sd)
        assert np.array_equal(a.cspl.x, ref["x"])
        assert np.shape(a.cspl.c) == tuple(ref["c_shape"]) and array_digest(a.cspl.c) == str(ref["c_sha256"])


@pytest.mark.parametrize("scheme", GENERAL_CASES)
def test_general_constraint_lists_match_reference(oracle, scheme):
    """Constraint lists beyond velocity + acceleration: the reference's TOPPRA (seidel) on [varying velocity limits,
    JointTorqueConstraint, SecondOrderConstraint] against (1) toppra_amd's mirror classes (host numpy through the same
    callbacks) -- same parameters --, (2) toppra_amd.solverwrapper.dense_rows -- the wrapper's row assembly, which the
    reference's rows stored here came from --, (3) the oracle's DenseWrapper on those rows: K, sd, u, feasible sets bit
    for bit."""
    import toppra_amd as ta
    from toppra_amd.solverwrapper import dense_rows
    for trial, d, way, inv_dyn, taulim, fric, vfun in general_problems(scheme):
        ref = reference_outputs("general", case_id(scheme), trial)
        mpath = ta.SplineInterpolator(GENERAL_KNOTS, way)
        mrows = dense_rows(general_constraint_lists(ta.constraint, scheme, inv_dyn, taulim, fric, vfun), mpath, GENERAL_GRID)
        for k in ("a", "b", "c", "low", "high", "deltas"):
            assert_same(mrows[k], ref["rows_" + k], "rows %s (mirror classes vs the reference's)" % k)
        sd0, sd1 = (0.0, 0.0) if trial % 2 else (0.1, 0.05)
        w = oracle.DenseWrapper(mrows["a"], mrows["b"], mrows["c"], mrows["low"], mrows["high"], mrows["deltas"])
        st, osdd, osd, oxs, oK = w.compute_parameterization(sd0, sd1)
        assert_same(oK, ref["K"], "K")
        if ref["failed"]:
            assert st == 1
        else:
            assert st == 0
            assert_same(osd, ref["sd"], "sd")
            assert_same(osdd, ref["sdd"], "u")
        w2 = oracle.DenseWrapper(mrows["a"], mrows["b"], mrows["c"], mrows["low"], mrows["high"], mrows["deltas"])
        assert_same(w2.compute_feasible_sets(), ref["X"], "X")

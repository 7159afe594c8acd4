"""Any geometric path, host side: the path classes against the scipy / numpy objects they wrap, the tpr_sampled_problem
binding against the header, refusals that need no GPU, and the numpy restatement of the sampled rows (tests/sampled_ref.py)
pinned against the reference's stored results on every tests/golden/path_*.npz fixture, through the CPU checker."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.interpolate import BPoly, UnivariateSpline

from tests import sampled_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sampled_ref.fixtures()


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- the three path classes ----------------------------------------------------------------------------------------
ARGS = (0.37, np.float64(0.0), np.linspace(0, 1, 7), np.array([0.2]))


def test_exports():
    import toppra_amd as ta
    for name in ("SimplePath", "PolynomialPath", "UnivariateSplineInterpolator", "SplineInterpolator"):
        assert name in ta.__all__ and hasattr(ta, name)
    assert ta.SimplePath is ta.simplepath.SimplePath
    assert ta.PolynomialPath is ta.interpolator.PolynomialPath


@pytest.mark.parametrize("with_yd", [False, True])
def test_simple_path(with_yd):
    import toppra_amd as ta
    rng = np.random.default_rng(1)
    x, y = np.array([0.0, 0.2, 0.7, 1.0]), rng.standard_normal((4, 3))
    yd = rng.standard_normal((4, 3)) if with_yd else None
    path = ta.SimplePath(x, y, yd)
    fill = yd
    if fill is None:
        fill = np.zeros_like(y)
        for i in range(1, 3):
            fill[i] = (y[i + 1] - y[i - 1]) / (x[i + 1] - x[i - 1])
    polys = [BPoly.from_derivatives(x, np.vstack((y[:, j], fill[:, j])).T) for j in range(3)]
    for order in (0, 1, 2):
        for s in ARGS:
            _same(path(s, order), np.array([p.derivative(order)(s) for p in polys]).T)
    assert path.dof == 3
    _same(path.path_interval, np.array([0.0, 1.0]))
    _same(path.waypoints, y)
    one = ta.SimplePath(x, y[:, 0])  # a 1-d y is one joint
    assert one.dof == 1 and one(np.linspace(0, 1, 5)).shape == (5, 1)


def test_polynomial_path():
    import toppra_amd as ta
    coeff = np.random.default_rng(2).standard_normal((2, 6))
    path = ta.PolynomialPath(coeff, 0.0, 2.0)
    polys = [np.polynomial.Polynomial(coeff[i]) for i in range(2)]
    for order in (0, 1, 2):
        for s in ARGS:
            _same(path(s, order), np.array([p(np.array(s)) for p in polys]).T)
        polys = [p.deriv() for p in polys]
    assert path.dof == 2 and path.duration == 2.0
    _same(path.path_interval, np.array([0.0, 2.0]))
    with pytest.raises(ValueError):
        path(0.5, 3)
    with pytest.raises(NotImplementedError):
        path.waypoints  # (the reference defines none for this class: the base class's answer)
    one = ta.PolynomialPath([1.0, 2.0, 3.0])
    assert one.dof == 1
    _same(one(np.array([0.0, 0.5])), np.polynomial.Polynomial([1.0, 2.0, 3.0])(np.array([0.0, 0.5])))
    _same(one(np.array([0.0, 0.5]), 1), np.polynomial.Polynomial([1.0, 2.0, 3.0]).deriv()(np.array([0.0, 0.5])))
    row = ta.PolynomialPath([[1.0, 2.0, 3.0]])  # a 2-d coeff of one row is a single joint too: flat samples
    assert row.dof == 1
    for order in (0, 1, 2):
        _same(row(np.array([0.0, 0.5]), order), one(np.array([0.0, 0.5]), order))


def test_univariate_spline_interpolator():
    import toppra_amd as ta
    rng = np.random.default_rng(3)
    x, y = np.linspace(0, 1, 10), rng.standard_normal((10, 4))
    path = ta.UnivariateSplineInterpolator(x, y)
    spl = [UnivariateSpline(x, y[:, i]) for i in range(4)]
    for order in (0, 1, 2):
        for s in ARGS:
            _same(path(s, order), np.array([f(s) for f in spl]).T)
        spl = [f.derivative() for f in spl]
    _same(path.eval(0.3), path(0.3))
    _same(path.evald(0.3), path(0.3, 1))
    _same(path.evaldd(0.3), path(0.3, 2))
    assert path.dof == 4 and list(path.path_interval) == [0.0, 1.0]
    with pytest.raises(AssertionError):
        ta.UnivariateSplineInterpolator(x + 0.5, y)
    with pytest.raises(AssertionError):
        ta.UnivariateSplineInterpolator(x, y[:-1])
    assert all(isinstance(f, UnivariateSpline) for f in path.uspl) and len(path.uspl) == 4 and len(path.uspld) == 4 and len(path.uspldd) == 4


@pytest.mark.reference
@pytest.mark.parametrize("name", [n for n in FIXTURES if "trig" not in n])
def test_path_classes_equal_the_reference(reference, name):
    """The package's classes return the reference's samples (same machine, same scipy)."""
    import toppra_amd as ta
    f = sampled_ref.load(name)
    mine, theirs = sampled_ref.make_path(f, ta), sampled_ref.make_path(f, reference)
    for order in (0, 1, 2):
        _same(mine(f["grid"], order), theirs(f["grid"], order))
        _same(mine(0.4, order), theirs(0.4, order))
    assert mine.dof == theirs.dof
    _same(mine.path_interval, theirs.path_interval)


# ---- the binding --------------------------------------------------------------------------------------------------
def test_sampled_struct_matches_header():
    from toppra_amd import _capi
    S = _capi.tpr_sampled_problem
    assert ctypes.sizeof(S) == 4 * 4 + 9 * 8
    assert S.grid.offset == 16 and S.q.offset == 24 and S.active.offset == 16 + 8 * 8
    hdr = open(os.path.join(ROOT, "include", "toppra_hip.h")).read()
    body = hdr[hdr.index("typedef struct tpr_sampled_problem {"):hdr.index("} tpr_sampled_problem;")]
    order = [body.index(name) for name in ("B, d, N, flags;", "*grid;", "*q, *qs, *qss;", "*vlim, *alim;", "*sd_start, *sd_end;",
                                           "*active;")]
    assert order == sorted(order)
    assert [n for n, _ in S._fields_] == ["B", "d", "N", "flags", "grid", "q", "qs", "qss", "vlim", "alim", "sd_start", "sd_end",
                                          "active"]


def test_sampled_symbols_exported():
    from toppra_amd import _capi, build
    build.build()
    lib = _capi.load()
    for name in ("tpr_sampled_problem_bytes", "tpr_sampled_rows_batch", "tpr_solve_sampled_batch",
                 "tpr_controllable_sets_sampled_batch", "tpr_feasible_sets_sampled_batch", "tpr_reachable_sets_sampled_batch",
                 "tpr_solve_desired_duration_sampled_batch", "tpr_param_spline_samples_batch"):
        assert hasattr(lib, name) and name in _capi.EXPORTS, name
    assert lib.tpr_sampled_problem_bytes() == ctypes.sizeof(_capi.tpr_sampled_problem)


def test_integration_stub_declares_the_sampled_struct():
    from toppra_amd import _capi
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = re.search(r"class tpr_sampled_problem\(C\.Structure\):\s*_fields_ = \[(.*?)\]\s*(#[^\n]*)?\n\n", text, re.S)
    assert block
    fields = re.findall(r'\("(\w+)",\s*C\.(\w+)\)', block.group(1))
    assert [(n, getattr(ctypes, t)) for n, t in fields] == list(_capi.tpr_sampled_problem._fields_)


# ---- refusals from shapes alone, before any launch (no GPU here) ------------------------------------------------------
def _samples(B, N, d, seed=0):
    rng = np.random.default_rng(seed)
    lim = np.stack([-np.ones((B, d)), np.ones((B, d))], -1)
    return np.linspace(0, 1, N + 1), rng.standard_normal((B, N + 1, d)), rng.standard_normal((B, N + 1, d)), \
        rng.standard_normal((B, N + 1, d)), 3 * lim, 5 * lim


def test_refusals_need_no_gpu():
    from toppra_amd import batch
    from toppra_amd.algorithm import BatchTOPPRA
    grid, q, qs, qss, vlim, alim = _samples(2, 5, 31)
    with pytest.raises(NotImplementedError, match="31 dof"):
        batch.solve_sampled_batch(grid, qs, qss, vlim, alim, interpolation=True)
    with pytest.raises(NotImplementedError, match="31 dof"):
        BatchTOPPRA.from_path_samples(grid, q, qs, qss, vlim, alim)
    BatchTOPPRA.from_path_samples(grid, q, qs, qss, vlim, alim, interpolation=False)  # 2 + 2 * 31 rows: fine
    grid, q, qs, qss, vlim, alim = _samples(2, 5, 3)
    for bad in (dict(qss=qss[:, :-1]), dict(qss=qss[:, :, :2]), dict(q=q[:1]), dict(grid=grid[:-1]), dict(vlim=vlim[:, :2]),
                dict(alim=alim[:1]), dict(qs=qs[0])):
        kw = dict(gridpoints=grid, q=q, qs=qs, qss=qss, vlim=vlim, alim=alim)
        kw.update({("gridpoints" if k == "grid" else k): v for k, v in bad.items()})
        with pytest.raises(ValueError):
            BatchTOPPRA.from_path_samples(**kw)
    with pytest.raises(ValueError, match="increasing"):
        batch.feasible_sets_sampled_batch(grid[::-1], qs, qss, vlim, alim)
    with pytest.raises(ValueError, match="sd must have shape"):
        batch.param_spline_samples_batch(grid, q, qs, np.ones((2, 5)))
    inst = BatchTOPPRA.from_path_samples(grid, q, qs, qss, vlim, alim)
    with pytest.raises(NotImplementedError, match="between the gridpoints"):
        inst.compute_trajectory(parametrizer="ParametrizeConstAccel")
    with pytest.raises(NotImplementedError):
        inst.compute_trajectory_samples(np.linspace(0, 1, 4))


# ---- the yardstick itself: the restated rows through the CPU checker give the reference's stored bits -------------------
def _rows(f):
    r = sampled_ref.sampled_problem(f["grid"], f["qs"][None], f["qss"][None], f["vlim"][None], f["alim"][None], f["interpolation"])
    return [r[k] for k in ("a", "b", "c", "low", "high", "deltas")]


def test_fixture_set():
    assert len(FIXTURES) == 12
    kinds = {sampled_ref.load(n)["kind"] for n in FIXTURES}
    assert kinds == {"simple", "poly", "uspl", "trig"}
    assert sampled_ref.load("path_simple_yd_d3_N40")["bad_status"] == 1          # sd_start outside K[0]
    assert (sampled_ref.load("path_trig_d3_N30_vpos")["vlim"][:, 0] > 0).all()   # a velocity range that excludes 0
    assert not np.allclose(np.diff(sampled_ref.load("path_simple_yd_d3_N40")["grid"]), 1 / 40)  # a non-uniform grid
    for n in FIXTURES:
        assert os.path.getsize(os.path.join(sampled_ref.GOLDEN, n + ".npz")) <= 455519  # the largest fixture before these


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_rows_reproduce_the_reference(oracle, name):
    f = sampled_ref.load(name)
    rows = _rows(f)
    tags = ["zero", "pair"] + (["bad"] if "bad_pair" in f else [])
    for tag in tags:
        s0, s1 = (0.0, 0.0) if tag == "zero" else f[tag + "_pair" if tag == "bad" else "pair"]
        out = oracle.solve_dense_batch(*rows, np.array([s0]), np.array([s1]), want_X=True)
        assert int(out["status"][0]) == int(f[tag + "_status"]), tag
        _same(out["K"][0], f[tag + "_K"])
        _same(out["X"][0], f["X"])
        _same(out["sd"][0], f[tag + "_sd"])
        _same(out["u"][0], f[tag + "_u"])
    s0, s1 = f["sd_pair"]
    out = oracle.solve_dense_batch_sd(*rows, float(f["sd_desired"]), np.array([s0]), np.array([s1]))
    assert int(out["status"][0]) == int(f["sd_status"])
    _same(out["K"][0], f["sd_K"])
    _same(out["sd"][0], f["sd_sd"])
    _same(out["u"][0], f["sd_u"])

"""Stage boxes of first-order constraints, host side: the binding against the header and the library, refusals that need no GPU,
and the numpy restatement of the fold (tests/stage_boxes_ref.py) pinned against the reference's own low_arr / high_arr and
against the stored results of tests/golden/boxes_*.npz, through the CPU checker."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import sampled_ref, stage_boxes_ref as sbr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sbr.fixtures()
NEW = ("tpr_bound_source_bytes", "tpr_stage_boxes_batch", "tpr_solve_sampled_boxed_batch",
       "tpr_solve_desired_duration_sampled_boxed_batch", "tpr_controllable_sets_sampled_boxed_batch",
       "tpr_feasible_sets_sampled_boxed_batch", "tpr_reachable_sets_sampled_boxed_batch")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(np.signbit(a), np.signbit(b))


# ---- the binding --------------------------------------------------------------------------------------------------
def test_the_seven_symbols_are_exported():
    from toppra_amd import _capi, build
    build.build()
    lib = _capi.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _capi.EXPORTS, name
    import toppra_amd as ta
    for name in ("stage_boxes_batch", "solve_sampled_boxed_batch", "solve_desired_duration_sampled_boxed_batch",
                 "controllable_sets_sampled_boxed_batch", "feasible_sets_sampled_boxed_batch", "reachable_sets_sampled_boxed_batch"):
        assert name in ta.batch.__all__ and hasattr(ta.batch, name)
    assert hasattr(ta.constraint, "BatchJointVelocityConstraintVarying") and hasattr(ta.constraint, "BatchBoundConstraint")


def test_bound_source_struct_matches_header_and_library():
    from toppra_amd import _capi
    S = _capi.tpr_bound_source
    assert ctypes.sizeof(S) == 2 * 4 + 8
    assert _capi.load().tpr_bound_source_bytes() == ctypes.sizeof(S)
    assert [n for n, _ in S._fields_] == ["kind", "flags", "data"] and S.data.offset == 8
    hdr = open(os.path.join(ROOT, "include", "toppra_hip.h")).read()
    body = hdr[hdr.index("typedef struct tpr_bound_source {"):hdr.index("} tpr_bound_source;")]
    assert body.index("int32_t kind, flags;") < body.index("const double *data;")
    for name, val in (("TPR_BOUND_VLIM", _capi.BOUND_VLIM), ("TPR_BOUND_VLIM_GRID", _capi.BOUND_VLIM_GRID), ("TPR_BOUND_X", _capi.BOUND_X),
                      ("TPR_BOUND_U", _capi.BOUND_U), ("TPR_BOUND_SHARED", _capi.BOUND_SHARED),
                      ("TPR_BOUND_MAX_SOURCES", _capi.BOUND_MAX_SOURCES)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, hdr).group(1)) == val, name


def test_integration_stub_declares_the_bound_source():
    from toppra_amd import _capi
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = re.search(r"class tpr_bound_source\(C\.Structure\):\s*_fields_ = \[(.*?)\]\s*(#[^\n]*)?\n\n", text, re.S)
    assert block
    fields = re.findall(r'\("(\w+)",\s*C\.(\w+)\)', block.group(1))
    assert [(n, getattr(ctypes, t)) for n, t in fields] == list(_capi.tpr_bound_source._fields_)


# ---- refusals from shapes alone, before any launch (no GPU here) ------------------------------------------------------
def _samples(B, N, d, seed=0):
    rng = np.random.default_rng(seed)
    lim = np.stack([-np.ones((B, d)), np.ones((B, d))], -1)
    coef = rng.standard_normal((B, 4, 4, d))
    return np.linspace(0, 1, N + 1), rng.standard_normal((B, N + 1, d)), rng.standard_normal((B, N + 1, d)), \
        rng.standard_normal((B, N + 1, d)), 3 * lim, 5 * lim, coef, np.linspace(0, 1, 5)


def test_refusals_need_no_gpu():
    from toppra_amd import batch
    from toppra_amd.algorithm import BatchTOPPRA
    from toppra_amd.constraint import BatchBoundConstraint, BatchJointVelocityConstraintVarying
    B, N, d = 2, 5, 3
    grid, q, qs, qss, vlim, alim, coef, breaks = _samples(B, N, d)
    box = np.stack([np.zeros((B, N + 1)), np.ones((B, N + 1))], -1)
    vgrid = np.broadcast_to(vlim[:, None], (B, N + 1, d, 2)).copy()
    # a 3-D array of limits is ambiguous between [B, d, 2] and [N+1, d, 2]
    with pytest.raises(ValueError, match="ambiguous"):
        BatchJointVelocityConstraintVarying(vlim)
    with pytest.raises(ValueError):
        BatchJointVelocityConstraintVarying(vgrid[..., :1])
    # too many sources: vlim + 8 bounds
    many = [BatchBoundConstraint(xbound=box) for _ in range(8)]
    with pytest.raises(NotImplementedError, match="bound sources"):
        BatchTOPPRA(coef, breaks, grid, vlim, alim, constraints=many)
    with pytest.raises(NotImplementedError, match="bound sources"):
        BatchTOPPRA.from_path_samples(grid, q, qs, qss, vlim, alim, constraints=many)
    BatchTOPPRA(coef, breaks, grid, None, alim, constraints=many)  # 8 fit
    with pytest.raises(NotImplementedError, match="9 bound sources"):
        batch.stage_boxes_batch(qs, [("xbound", box)] * 9)
    # vlim given to a boxed entry
    for fn, args in ((batch.solve_sampled_boxed_batch, ()), (batch.feasible_sets_sampled_boxed_batch, ()),
                     (batch.controllable_sets_sampled_boxed_batch, (0.0, 0.0)), (batch.reachable_sets_sampled_boxed_batch, (0.0, 0.0)),
                     (batch.solve_desired_duration_sampled_boxed_batch, (2.0,))):
        with pytest.raises(NotImplementedError, match="take no vlim"):
            fn(grid, qs, qss, alim, box, box, *args, vlim=vlim)
    # NaN in a numpy bound
    bad = box.copy()
    bad[1, 2, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        batch.stage_boxes_batch(qs, [("xbound", bad)])
    with pytest.raises(ValueError, match="NaN"):
        batch.solve_sampled_boxed_batch(grid, qs, qss, alim, bad, box)
    nanv = vgrid.copy()
    nanv[0, 0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        batch.stage_boxes_batch(qs, [("vlim_grid", nanv)])
    # wrong shapes
    for src in (("xbound", box[:, :-1]), ("ubound", box[:1]), ("xbound", box[..., :1]), ("vlim", vlim[:, :2]), ("vlim_grid", vgrid[:, :, :2]),
                ("vlim_grid", vgrid[:, 1:]), ("speed", box)):
        with pytest.raises(ValueError):
            batch.stage_boxes_batch(qs, [src])
    with pytest.raises(NotImplementedError, match="dof 33"):
        batch.stage_boxes_batch(np.ones((2, N + 1, 33)), [("vlim", np.ones((33, 2)))])
    with pytest.raises(ValueError, match="needs qs"):
        batch.stage_boxes_batch(None, [("xbound", box), ("vlim", vlim)], N=N)
    for low, high in ((box[:, :-1], box), (box, box[:1]), (box[..., 0], box)):
        with pytest.raises(ValueError, match="must have shape"):
            batch.feasible_sets_sampled_boxed_batch(grid, qs, qss, alim, low, high)
    with pytest.raises(ValueError):
        BatchTOPPRA(coef, breaks, grid, vlim, alim, constraints=[BatchBoundConstraint(xbound=box[:, :-1])])
    with pytest.raises(ValueError):
        BatchTOPPRA.from_path_samples(grid, q, qs, qss, vlim, alim, constraints=[BatchJointVelocityConstraintVarying(vgrid[:, :, :2])])
    with pytest.raises(ValueError):
        BatchBoundConstraint()
    # the 122-row limit
    grid, q, qs, qss, vlim, alim, coef, breaks = _samples(2, 5, 31)
    box = np.stack([np.zeros((2, 6)), np.ones((2, 6))], -1)
    with pytest.raises(NotImplementedError, match="31 dof"):
        batch.solve_sampled_boxed_batch(grid, qs, qss, alim, box, box)
    with pytest.raises(NotImplementedError, match="31 dof"):
        BatchTOPPRA(coef, breaks, grid, vlim, alim, constraints=[BatchBoundConstraint(xbound=box)])
    with pytest.raises(NotImplementedError, match="31 dof"):
        BatchTOPPRA.from_path_samples(grid, q, qs, qss, vlim, alim, constraints=[BatchBoundConstraint(xbound=box)])
    BatchTOPPRA(coef, breaks, grid, vlim, alim, interpolation=False, constraints=[BatchBoundConstraint(xbound=box)])  # 2 + 2 * 31


def test_the_callable_is_checked_and_single_path_use_is_refused():
    from toppra_amd.constraint import BatchBoundConstraint, BatchJointVelocityConstraintVarying
    grid = np.linspace(0, 1, 6)
    calls = []

    def good(s):
        calls.append(np.shape(s))
        return np.ones(np.shape(s) + (3, 2))
    src = BatchJointVelocityConstraintVarying(good).bound_sources(grid, 2, 5, 3, np.zeros((2, 6, 3)))
    assert calls == [(6,)] and src[0][0] == "vlim_grid" and src[0][1].shape == (6, 3, 2)
    with pytest.raises(ValueError, match="must return"):
        BatchJointVelocityConstraintVarying(lambda s: np.ones((3, 2))).bound_sources(grid, 2, 5, 3, np.zeros((2, 6, 3)))
    with pytest.raises(NotImplementedError):
        BatchBoundConstraint(xbound=np.zeros((6, 2))).compute_constraint_params(None, grid)


def test_compute_entries_refuse_to_run_without_tpr_init():
    """In a process that never called tpr_init (this one has no GPU to call it on)."""
    import subprocess
    import sys
    code = (
        "import ctypes as C, numpy as np\n"
        "from toppra_amd import _capi\n"
        "L = _capi.load()\n"
        "x = np.zeros((1, 3, 2)); qs = np.ones((1, 3, 1)); g = np.linspace(0, 1, 3); al = np.array([[[-1.0, 1.0]]])\n"
        "src = (_capi.tpr_bound_source * 1)(_capi.tpr_bound_source(kind=3, flags=0, data=x.ctypes.data))\n"
        "rcs = [L.tpr_stage_boxes_batch(1, 2, 1, None, 1, src, 0, x.ctypes.data, x.ctypes.data, None)]\n"
        "assert b'tpr_init' in L.tpr_last_error()\n"
        "p = _capi.tpr_sampled_problem(B=1, d=1, N=2, flags=6, grid=g.ctypes.data, qs=qs.ctypes.data, qss=qs.ctypes.data, alim=al.ctypes.data)\n"
        "r = _capi.tpr_result(K=x.ctypes.data)\n"
        "v = np.zeros(1)\n"
        "rcs.append(L.tpr_solve_sampled_boxed_batch(C.byref(p), x.ctypes.data, x.ctypes.data, C.byref(r), None))\n"
        "rcs.append(L.tpr_solve_desired_duration_sampled_boxed_batch(C.byref(p), x.ctypes.data, x.ctypes.data, v.ctypes.data, 1e-5, C.byref(r), None, None))\n"
        "rcs.append(L.tpr_controllable_sets_sampled_boxed_batch(C.byref(p), x.ctypes.data, x.ctypes.data, v.ctypes.data, v.ctypes.data, x.ctypes.data, None))\n"
        "rcs.append(L.tpr_feasible_sets_sampled_boxed_batch(C.byref(p), x.ctypes.data, x.ctypes.data, x.ctypes.data, None))\n"
        "rcs.append(L.tpr_reachable_sets_sampled_boxed_batch(C.byref(p), x.ctypes.data, x.ctypes.data, v.ctypes.data, v.ctypes.data, x.ctypes.data, None, None))\n"
        "assert b'tpr_init' in L.tpr_last_error()\n"
        "print(rcs)\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env=dict(os.environ, TOPPRA_HIP_NO_TORCH="1"))
    assert out.returncode == 0, out.stderr
    rcs = eval(out.stdout.strip().splitlines()[-1])
    assert len(rcs) == 6 and all(rc != 0 for rc in rcs) and len(set(rcs)) == 1, rcs


# ---- the yardstick itself ------------------------------------------------------------------------------------------
def test_fixture_set_and_its_binding_conditions():
    """Re-asserted from the stored arrays: a kernel that ignores a bound cannot reproduce these results."""
    assert FIXTURES == ["boxes_a_d3_N30", "boxes_b_d9_N30", "boxes_c_d17_N30", "boxes_d_d7_N40"]
    kinds = {n[6]: sbr.load(n)["kinds"] for n in FIXTURES}
    assert kinds == {"a": ["vary", "acc"], "b": ["vel", "vary", "acc", "bound"], "c": ["acc", "bound"], "d": ["vary", "torque"]}
    for n in FIXTURES:
        f = sbr.load(n)
        assert os.path.getsize(os.path.join(sbr.GOLDEN, n + ".npz")) < 100 * 1024
        assert f["qs"].shape[0] == 4 and f["qs"].shape[1] - 1 in (30, 40)
        cond = sbr.binding_conditions(f)
        assert cond["ok"], n
        assert ("vary" in cond) == ("vary" in f["kinds"]) and min(cond.get("vary", [5])) >= 5, (n, cond)
        assert ("vary_box" in cond) == (n == "boxes_b_d9_N30") and min(cond.get("vary_box", [5])) >= 5, (n, cond)
        assert ("xcap" in cond) == ("bound" in f["kinds"]) and min(cond.get("xcap", [5])) >= 5, (n, cond)
        assert min(cond.get("ucap", [3])) >= 3, (n, cond)
        assert (f["bad_status"] == 1).all() and (f["pair_status"] == 0).all() and (f["pair"] > 0).all()
    assert "ucap" in sbr.binding_conditions(sbr.load("boxes_b_d9_N30")) and not sbr.load("boxes_c_d17_N30")["interpolation"]


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_fold_gives_the_stored_reference_boxes(oracle, name):
    f = sbr.load(name)
    low, high = sbr.stage_boxes(oracle, f["qs"], sbr.sources(f), 4, f["qs"].shape[1] - 1)
    _same(low, f["low_ref"])
    _same(high, f["high_ref"])


@pytest.mark.reference
@pytest.mark.parametrize("name", FIXTURES)
def test_restated_fold_equals_the_reference_wrapper(reference, oracle, name):
    """The reference's own seidelWrapper.low_arr / high_arr for the fixture lists.  The arrays are private to the Cython class;
    on a wrapper that holds the first-order constraints only (no rows) the optimum of a stage LP is a corner of the box,
    copied, so two solve_stagewise_optim calls per stage read them back.  vgrid is rebuilt by the reference's own loop."""
    from toppra.solverwrapper.cy_seidel_solverwrapper import seidelWrapper
    f = sbr.load(name)
    nan = float("nan")
    for b in range(4):
        path = reference.SplineInterpolator(f["knots"], f["way"][b])
        cons = [c for c in sbr.reference_list(f, b, reference.constraint) if c.compute_constraint_params(path, f["grid"])[0] is None]
        w = seidelWrapper(cons, path, f["grid"])
        low = np.array([w.solve_stagewise_optim(i, None, np.array([1.0, 1.0]), nan, nan, nan, nan) for i in range(len(f["grid"]))])
        high = np.array([w.solve_stagewise_optim(i, None, np.array([-1.0, -1.0]), nan, nan, nan, nan) for i in range(len(f["grid"]))])
        src = [(k, a[b]) for k, a in sbr.sources(f)]
        if "vary" in f["kinds"]:
            _same(np.array([sbr.vlim_func(f, b)(s) for s in f["grid"]]), f["vgrid"][b])
        mine = sbr.fold(oracle, f["qs"][b], src, len(f["grid"]))
        _same(mine[0], low)
        _same(mine[1], high)


def _rows(f):
    """The dense problem of the fixture's list: rows without a velocity constraint, the boxes from the restated fold."""
    from tests.second_order_ref import batched_torque_model
    blocks = []
    if "torque" in f["kinds"]:
        model = batched_torque_model(f["mass"], f["grav"], f["cori"])
        zero = np.zeros_like(f["q"])
        blocks = [{"w0": model(f["q"], zero, zero), "wa": model(f["q"], zero, f["qs"]), "wb": model(f["q"], f["qs"], f["qss"]),
                   "F": None, "g": np.concatenate((f["taumax"], f["taumax"]), -1), "friction": f["fric"], "interpolation": False}]
    r = sampled_ref.sampled_problem(f["grid"], f["qs"], f["qss"], None, f.get("alim"), f["interpolation"], blocks)
    return r


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_boxes_reproduce_the_reference_results(oracle, name):
    """Rows without vlim + folded boxes through the CPU checker: the reference's stored K, sd, u, status, X and TOPPRAsd."""
    f = sbr.load(name)
    r = _rows(f)
    low, high = sbr.stage_boxes(oracle, f["qs"], sbr.sources(f), 4, f["qs"].shape[1] - 1)
    rows = [r["a"], r["b"], r["c"], low, high, r["deltas"]]
    for tag, pair in (("zero", np.zeros((4, 2))), ("pair", f["pair"]), ("bad", np.broadcast_to(f["bad_pair"], (4, 2)))):
        out = oracle.solve_dense_batch(*rows, pair[:, 0].copy(), pair[:, 1].copy(), want_X=True)
        assert np.array_equal(out["status"], f[tag + "_status"]), tag
        _same(out["K"], f[tag + "_K"])
        _same(out["sd"], f[tag + "_sd"])
        _same(out["u"], f[tag + "_u"])
        _same(out["X"], f["X"])
    out = oracle.solve_dense_batch_sd(*rows, f["sd_desired"])
    assert np.array_equal(out["status"], f["sd_status"])
    _same(out["K"], f["sd_K"]); _same(out["sd"], f["sd_sd"]); _same(out["u"], f["sd_u"])
    for b in range(4):
        w = oracle.DenseWrapper(*[np.ascontiguousarray(v[b]) for v in rows])
        _same(w.compute_controllable_sets(*f["sets"]), f["K_set"][b])
        L, X = oracle.DenseWrapper(*[np.ascontiguousarray(v[b]) for v in rows]).compute_reachable_sets(*f["sets"])
        _same(L, f["L"][b])

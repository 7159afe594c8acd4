"""What the five passes return on each of their four sources (spline table, dense rows, samples, samples with stage boxes) and
what the robust solve returns: the exact keys, arities, shapes, dtypes and kinds, once from numpy and once from tensors on device
0, at B = 3, d = 2, N = 4 (the smallest shape with an interior stage, more than one dof and a non-trivial batch).  Recorded
before the pass bodies were folded onto one path for all four sources: this file is the evidence that the fold moved nothing."""
import itertools

import numpy as np
import pytest

from toppra_amd import batch

pytestmark = pytest.mark.gpu

B, D, N = 3, 2, 4
BOOL = (False, True)
SHAPES = {"sd2": (B, N + 1), "sd": (B, N + 1), "u": (B, N), "K": (B, N + 1, 2), "X": (B, N + 1, 2), "status": (B,), "alpha": (B,)}


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


@pytest.fixture(scope="module", params=["numpy", "tensor"])
def sources(request, gpu):
    """The four sources of one problem, as arrays of one kind: {name: (suffix of the functions, leading arguments)}."""
    data = batch.make_synthetic_batch(B, D, N)
    if request.param == "tensor":
        import torch
        data = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda:0") for k, v in data.items()}
    table = tuple(data[k] for k in ("coef", "breaks", "grid", "vlim", "alim"))
    pe = batch.path_eval_batch(*table[:3])
    rows = batch.constraint_params_batch(*table)
    low, high = batch.stage_boxes_batch(pe["qs"], [("vlim", data["vlim"])])
    deltas = data["grid"][1:] - data["grid"][:-1]
    return {"like": data["coef"],
            "table": ("", table),
            "dense": ("_dense", (rows["a"], rows["b"], rows["c"], rows["low"], rows["high"], deltas)),
            "sampled": ("_sampled", (data["grid"], pe["qs"], pe["qss"], data["vlim"], data["alim"])),
            "boxed": ("_sampled_boxed", (data["grid"], pe["qs"], pe["qss"], data["alim"], low, high))}


def _check_array(x, name, like):
    """``x`` has the shape and dtype of the output ``name`` and the kind of ``like``: numpy, or a tensor on like's device."""
    if isinstance(like, np.ndarray):
        assert isinstance(x, np.ndarray) and x.dtype == (np.int32 if name == "status" else np.float64), name
    else:
        import torch
        assert isinstance(x, torch.Tensor) and x.device == like.device, name
        assert x.dtype == (torch.int32 if name == "status" else torch.float64), name
    assert tuple(x.shape) == SHAPES[name], name


def _check_dict(out, keys, like):
    assert isinstance(out, dict) and set(out) == set(keys)
    for name, arr in out.items():
        _check_array(arr, name, like)
    assert np.array_equal(_host(out["status"]), np.zeros(B, dtype=np.int32))
    assert not any(np.isnan(_host(arr)).any() for arr in out.values())


def _duration(sd, grid):
    """The duration of the profile sd [B, N+1] on the shared grid, as ParametrizeConstAccel integrates it."""
    sd, grid = _host(sd), _host(grid)
    return (2 * np.diff(grid) / (sd[:, 1:] + sd[:, :-1])).sum(axis=1)


@pytest.mark.parametrize("name", ["table", "dense", "sampled", "boxed"])
def test_the_five_passes_of_a_source(sources, name):
    like = sources["like"]
    suffix, lead = sources[name]
    fn = {p: getattr(batch, "%s%s_batch" % (p, suffix)) for p in ("solve", "solve_desired_duration", "controllable_sets",
                                                                  "feasible_sets", "reachable_sets")}
    if name == "table":
        for want_sd, want_K, want_u in itertools.product(BOOL, repeat=3):
            out = fn["solve"](*lead, 0.1, 0.1, want_sd=want_sd, want_K=want_K, want_u=want_u)
            _check_dict(out, ["sd2", "status"] + ["sd"] * want_sd + ["K"] * want_K + ["u"] * want_u, like)
    for want_sd in BOOL:
        out = fn["solve"](*lead, 0.1, 0.1, want_sd=want_sd)
        _check_dict(out, ["sd2", "u", "K", "status"] + ["sd"] * want_sd, like)
    desired = 1.25 * _duration(out["sd"], sources["table"][1][2])
    out = fn["solve_desired_duration"](*lead, desired, 0.1, 0.1)
    _check_dict(out, ["sd2", "sd", "u", "K", "status", "alpha"], like)
    alpha = _host(out["alpha"])
    assert np.all((alpha > 0) & (alpha < 1))
    _check_array(fn["controllable_sets"](*lead, 0.0, 0.2), "K", like)
    _check_array(fn["feasible_sets"](*lead), "X", like)
    _check_array(fn["reachable_sets"](*lead, 0.0, 0.2), "X", like)
    _check_array(fn["reachable_sets"](*lead, 0.0, 0.2, want_X=False), "X", like)
    both = fn["reachable_sets"](*lead, 0.0, 0.2, want_X=True)
    assert isinstance(both, tuple) and len(both) == 2
    for arr in both:
        _check_array(arr, "X", like)
        assert not np.isnan(_host(arr)).any()


def test_the_robust_solve(sources):
    like, (_, lead) = sources["like"], sources["table"]
    for want_X in BOOL:
        out = batch.robust_solve_batch(*lead, [1e-3, 5e-2, 9e-3], 0.1, 0.1, want_X=want_X)
        _check_dict(out, ["sd2", "sd", "u", "K", "status"] + ["X"] * want_X, like)


def test_the_table_source_agrees_with_the_sampled_source(sources):
    """Measured before the fold, on an MI355X at this shape, from numpy and from tensors: max |sd2 of the table source - sd2 of
    the sampled source on path_eval_batch's samples| = 0.0 for the solve and 0.0 for the desired-duration solve
    (profiles/python_layer_refactor.md).  A deviation of zero is asserted as bit equality."""
    (_, table), (_, sampled) = sources["table"], sources["sampled"]
    fast = batch.solve_batch(*table, 0.1, 0.1, want_sd=True)
    pairs = [(fast, batch.solve_sampled_batch(*sampled, 0.1, 0.1))]
    desired = 1.25 * _duration(fast["sd"], table[2])
    pairs.append((batch.solve_desired_duration_batch(*table, desired, 0.1, 0.1),
                  batch.solve_desired_duration_sampled_batch(*sampled, desired, 0.1, 0.1)))
    deviation = [float(np.max(np.abs(_host(a["sd2"]) - _host(b["sd2"])))) for a, b in pairs]
    print("table against sampled, max |sd2 - sd2| (solve, desired duration): %r" % (deviation,))
    for a, b in pairs:
        assert np.array_equal(_host(a["sd2"]), _host(b["sd2"]))


@pytest.mark.parametrize("interpolation", [True, False])
def test_the_table_wrapper_runs_the_batch_entries_and_carries_its_state(gpu, interpolation):
    """The five passes of ``hipSeidelWrapper`` on one object, each against the ``batch`` entry it stands for, bit for bit:
    controllable sets, feasible sets and the solve read and update the object's warm-start state; the reachable sets and the
    desired-duration solve leave it alone; and the desired-duration solve runs under Interpolation whatever the acceleration
    constraint's discretisation is -- what the wrapper did before its passes moved onto the shared base class."""
    import toppra_amd as ta
    from toppra_amd.interpolator import spline_tables
    data = batch.make_synthetic_batch(B, D, N)
    path = ta.SplineInterpolator(data["knots"], data["waypoints"][0])
    vel, acc = ta.constraint.JointVelocityConstraint(data["vlim"][0]), ta.constraint.JointAccelerationConstraint(data["alim"][0])
    acc.set_discretization_type(1 if interpolation else 0)
    wrapper = ta.solverwrapper.hipSeidelWrapper([vel, acc], path, data["grid"])
    coef, breaks = spline_tables(path)
    table = (coef[None], breaks, data["grid"], data["vlim"][:1], data["alim"][:1])
    state = np.zeros((1, 4), dtype=np.int32)   # what a wrapper object's state must be after the same passes
    lo, hi = np.array([0.0]), np.array([0.5 ** 2])

    def same(got, want):
        return np.array_equal(got, want, equal_nan=True)

    K = batch.controllable_sets_batch(*table, lo, hi, interpolation, active=state, squared=True)
    assert same(wrapper.controllable_sets(0.0, 0.5), K[0]) and np.array_equal(wrapper._active, state)
    X = batch.feasible_sets_batch(*table, interpolation, active=state)
    assert same(wrapper.feasible_sets(), X[0]) and np.array_equal(wrapper._active, state)
    out = batch.solve_batch(*table, 0.0, 0.0, interpolation, want_sd=True, active=state)
    res = wrapper.parameterization(0.0, 0.0)
    assert set(res) == {"sd2", "sd", "u", "K", "status"} and res["status"] == 0 and out["status"][0] == 0
    assert all(same(res[k], out[k][0]) for k in ("sd2", "sd", "u", "K")) and np.array_equal(wrapper._active, state)
    assert state.any()
    L, X = batch.reachable_sets_batch(*table, lo, hi, interpolation, want_X=True, squared=True)
    got = wrapper.reachable_sets(0.0, 0.5)
    assert same(got[0], L[0]) and same(got[1], X[0]) and np.array_equal(wrapper._active, state)
    desired = float(1.25 * _duration(out["sd"], data["grid"])[0])
    out = batch.solve_desired_duration_batch(*table, desired, lo, lo, 1e-5, squared=True)
    res = wrapper.parameterization_sd(0.0, 0.0, desired)
    assert set(res) == {"sd2", "sd", "u", "K", "status", "alpha"}
    assert all(same(res[k], out[k][0]) for k in res) and np.array_equal(wrapper._active, state)

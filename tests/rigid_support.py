"""What the GPU tests of the rigid-body family share (tests/test_gpu_chain.py, _tree, _tool_accel, _tool_wrench, _control_points,
_base_wrench, _joint_load): the device, the synthetic problem on the shapes of tests/chain_cases.py, an instance from a spline or
from samples, all five passes, deep bit-equality, the accuracy check against a cases module and the constraint-against-its-
callback comparison.  A plain module: the tests import it, not each other."""
import numpy as np

from tests import chain_cases as cc


def torch_device():
    import torch
    return torch, torch.device("cuda", 0)


def check(cases, key, got, label="d %d"):
    """Every quantity of ``got`` {name: value} within the bound of ``cases`` (a cases module) for the case ``key``."""
    ref = cases.reference(key)
    for name, val in got.items():
        err, bound = cc.metric(val, ref[name], ref[name + "_mag"]), cases.bound(key, name)
        print((label + " %s: error %.3g, bound %.3g (%.2f of it)") % (key, name, err, bound, err / bound if bound else 0.0))
        assert err <= bound, (key, name, err, bound)


def problem(d, B=cc.B, N=cc.N, seed=5):
    from toppra_amd import batch
    data = batch.make_synthetic_batch(B, d, N, seed=seed)
    return data, (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])


def instance(source, data, args, cons):
    """BatchTOPPRA with the constraints ``cons`` on the problem: from its spline, or ("samples") from the path's samples."""
    from toppra_amd import algorithm, batch
    if source == "spline":
        return algorithm.BatchTOPPRA(*args, constraints=cons)
    pe = batch.path_eval_batch(*args[:3])
    return algorithm.BatchTOPPRA.from_path_samples(data["grid"], pe["q"], pe["qs"], pe["qss"], data["vlim"], data["alim"], constraints=cons)


def run_passes(inst):
    out = {"rows": inst.dense_rows() if inst.constraints else inst.stage_boxes()}
    out["compute_parameterization"] = inst.compute_parameterization()
    out["compute_parameterization_sd"] = inst.compute_parameterization_sd(np.full(cc.B, 8.0))
    out["compute_feasible_sets"] = inst.compute_feasible_sets()
    out["compute_controllable_sets"] = inst.compute_controllable_sets(np.zeros(cc.B), np.full(cc.B, 0.3))
    out["compute_reachable_sets"] = inst.compute_reachable_sets(np.zeros(cc.B), np.full(cc.B, 0.3))
    return out


def same(a, b, what):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            same(a[k], b[k], what + "." + k)
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, "%s[%d]" % (what, i))
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), what


def compare(source, data, args, ours, inv_dyn, F, g, DT):
    """The constraint ``ours`` against BatchSecondOrderConstraint(inv_dyn, F, g) -- "theirs", ``inv_dyn`` the callback that gives
    the same quantity: the dense rows and all five passes are equal, and the limits leave every trajectory feasible."""
    from toppra_amd import constraint
    theirs = constraint.BatchSecondOrderConstraint(inv_dyn, F, g, discretization_scheme=DT)
    results = [run_passes(instance(source, data, args, [con])) for con in (ours, theirs)]
    same(results[0], results[1], "constraint vs callback")
    assert np.isfinite(results[0]["rows"][0]).all()
    for k in ("compute_parameterization", "compute_parameterization_sd"):
        assert np.all(results[0][k]["status"] == 0), k  # the limits leave every trajectory feasible
    return results[0]


def fixture_chain(fx):
    return {k: fx[k] for k in ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity", "tool")}

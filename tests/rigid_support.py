"""What the GPU tests of the rigid-body family share (tests/test_gpu_chain.py, _tree, _tool_accel, _tool_wrench, _control_points,
_base_wrench, _joint_load, _momentum): the device, the synthetic problem on the shapes of tests/chain_cases.py, an instance from a
spline or from samples, all five passes and what a list of constraints must leave of them, deep bit-equality, the accuracy check
against a cases module, the constraint-against-its-callback comparison, and the checks of a test against the reference's
fixtures -- the accuracy loop and the solve tail; and what the refusal-order tests of the family's C entries share (tests/test_rigid_refusal_order.py,
tests/test_momentum_refusal_order.py): the return codes, a tpr_chain of host arrays, a parent table and the 64-double buffer.
A plain module: the tests import it, not each other."""
import numpy as np

from tests import chain_cases as cc, chain_ref

BADARG, UNSUPPORTED = -1, -3
BUF = np.zeros(64)  # (every pointer a refusal test hands over: nothing is launched, so nothing reads past it)
_KEEP = []  # (what the structs handed out point into, kept alive)


def c_model(d=3, joint_type=None, dof=None):
    """(the chain, a tpr_chain of host arrays): ``joint_type`` in place of its own codes, ``dof`` in place of its own d."""
    sc = chain_ref.serial_chain(chain_ref.random_chain(d, 5))
    model, keep = sc.c_struct(BUF)
    _KEEP.append((sc, keep))
    if joint_type is not None:
        codes = np.array(joint_type, dtype=np.int32)
        _KEEP.append(codes)
        model.joint_type = codes.ctypes.data
    if dof is not None:
        model.d = dof
    return sc, model


def parent_table(d=3, table=None):
    """An int32 parent table, kept alive: the serial chain's of ``d`` links, or ``table``."""
    table = np.array(np.arange(d) - 1 if table is None else table, dtype=np.int32)
    _KEEP.append(table)
    return table


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


def passes_ran(out):
    """What a test_beside_* asks of run_passes(...) on its list: the rows are finite, both parameterizations leave every trajectory
    feasible, the three set passes hold no NaN."""
    assert all(np.isfinite(out["rows"][k]).all() for k in range(3))
    for k in ("compute_parameterization", "compute_parameterization_sd"):
        assert np.all(out[k]["status"] == 0), k
    for k in ("compute_feasible_sets", "compute_controllable_sets", "compute_reachable_sets"):
        sets = out[k] if isinstance(out[k], (tuple, list)) else (out[k],)
        assert all(not np.isnan(np.asarray(s)).any() for s in sets), k


# ---- the reference's fixtures (tests/golden/<family>_*.npz, made by tools/make_<family>_golden.py on tools/rigid_golden.py's recipe) ----

ROBOT_KEYS = ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity")


def fixture_chain(fx):
    return {k: fx[k] for k in ROBOT_KEYS + ("tool",)}


def fixture_tree(fx):
    return {k: fx[k] for k in ROBOT_KEYS + ("parent",)}


def fixture_accuracy(name, fx, got, mags):
    """Every quantity of ``got`` {name: value}, in the order of the fixture's acc_bound, within that bound of the stored one, in
    the metric of tests/chain_cases.py with the magnitudes ``mags`` {name: value}."""
    for i, (k, val) in enumerate(got.items()):
        err, bound = cc.metric(val, fx[k], mags[k]), fx["acc_bound"][i]
        print("ACCURACY fixture %s %s error %.3g bound %.3g fraction %.2f" % (name, k, err, bound, err / bound))
        assert err <= bound, (name, k, err, bound)


def fixture_scheme(fx, key="scheme"):
    """(whether the fixture's constraint is under Interpolation, its DiscretizationType)."""
    from toppra_amd import constraint
    interp = bool(int(fx[key]))
    return interp, constraint.DiscretizationType.Interpolation if interp else constraint.DiscretizationType.Collocation


def fixture_instance(fx, con, interpolation=True):
    from toppra_amd import algorithm
    return algorithm.BatchTOPPRA(fx["coef"], fx["breaks"], fx["grid"], fx["vlim"], fx["alim"], interpolation=interpolation, constraints=[con])


def fixture_sd(name, fx, inst):
    """The return codes are the reference's, all 0; sd within the stored end-to-end tolerance."""
    out = inst.compute_parameterization()
    assert np.array_equal(out["status"], fx["status"]) and np.all(fx["status"] == 0)
    dev = float(np.max(np.abs(out["sd"] - fx["sd"])))
    print("ACCURACY fixture %s sd deviation %.3g tolerance %.3g" % (name, dev, float(fx["sd_tol"])))
    assert dev <= float(fx["sd_tol"]), (name, dev, float(fx["sd_tol"]))


def fixture_solve(name, fx, con, interp):
    """The tail of a dense-row family's fixture test, ``con`` under Interpolation or not: the rows of a stage are the x_next pair,
    the acceleration block and the constraint's (F's rows, or the 2 d of a torque constraint; twice under Interpolation); low /
    high equal the reference's in bits; then fixture_sd.  Returns the dense rows."""
    inst = fixture_instance(fx, con)
    rows = inst.dense_rows()
    d = fx["coef"].shape[3]
    assert rows[0].shape[-1] == 2 + 4 * d + (2 if interp else 1) * (fx["F"].shape[-2] if "F" in fx else 2 * d)
    assert np.array_equal(rows[3], fx["low"]) and np.array_equal(rows[4], fx["high"])
    fixture_sd(name, fx, inst)
    return rows

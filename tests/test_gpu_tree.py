"""The kinematic-tree kernels on the MI355X: chain-shaped trees and forests against the chain entries bit for bit, every
root-to-leaf path isolated by zeroing the links off it (an exact test of both uses of a fork's bank), the fused kernel against
the single one, every shape against the numpy reference (tests/tree_ref.py) within the accuracy bound of tests/tree_cases.py, a
relabelled tree, the input kinds, a KinematicTree inside the torque constraint against the same tree as a callback, the
reference's fixtures, and the refusals.

Measured on the MI355X (B = 3, N = 22; error / bound, the bound being 16 x the float64 reference's own error against
np.longdouble): at most 0.36 over w0 / wa / wb of the eight shapes (y18, wb); the fixtures' terms use at most 0.18 of their
stored bounds, sd deviates by 2.7e-13 (tolerance 9.8e-13, vee) and 1.0e-15 (tolerance 1.8e-8, torso)."""
import ctypes as C

import numpy as np
import pytest

from tests import chain_ref, rigid_support as rs, second_order_ref as sor, tree_cases as tc, tree_ref
from tests.helpers import golden

pytestmark = pytest.mark.gpu
FIXTURES = ("tree_torque_vee_d3_N30_colloc", "tree_torque_torso_d15_N30")
PASSES = ("compute_parameterization", "compute_parameterization_sd", "compute_feasible_sets", "compute_controllable_sets")


def _inputs(d, seed):
    rng = np.random.default_rng(seed)
    q = rng.uniform(-3.0, 3.0, (tc.B, tc.N + 1, d))
    qs = rng.standard_normal((tc.B, tc.N + 1, d))
    qss = 2.0 * rng.standard_normal((tc.B, tc.N + 1, d))
    qs[1] = 0.0
    return q, qs, qss


def _as_tree(chain, parents):
    return tree_ref.kinematic_tree(dict(chain, parent=np.array(parents, dtype=np.int32)))


@pytest.mark.parametrize("d", [1, 3, 8, 9, 17, 18, 32])
def test_a_chain_shaped_tree_gives_the_chain_entries_bits(gpu, d):
    """tau and w0 / wa / wb of parents = -1, 0, 1, ... equal tpr_chain_inverse_dynamics_batch / tpr_chain_torque_terms_batch."""
    from toppra_amd.chain import KinematicTree
    chain = chain_ref.random_chain(d, seed=500 + d, gravity=d % 2 == 1, massless=d // 2 if d > 1 else None)
    sc = chain_ref.serial_chain(chain)
    q, qs, qss = _inputs(d, 600 + d)
    for tree in (_as_tree(chain, np.arange(d) - 1), KinematicTree.from_chain(sc)):
        assert np.array_equal(tree.inverse_dynamics(q, qs, qss), sc.inverse_dynamics(q, qs, qss))
        for got, want in zip(tree.torque_terms(q, qs, qss), sc.torque_terms(q, qs, qss)):
            assert np.array_equal(got, want)
    assert np.isfinite(sc.inverse_dynamics(q, qs, qss)).all()


def test_a_forest_equals_its_chains(gpu):
    """roots: two 9-link chains on the base equal two 9-dof chain-entry calls on the halves."""
    tree, q, qs, qss = tc.case("roots")
    kt = tree_ref.kinematic_tree(tree)
    tau, terms = kt.inverse_dynamics(q, qs, qss), kt.torque_terms(q, qs, qss)
    for half in (slice(0, 9), slice(9, 18)):
        part = {k: (v[half] if k not in ("gravity", "tool") else v) for k, v in tree.items() if k != "parent"}
        sc = chain_ref.serial_chain(part)
        assert np.array_equal(tau[..., half], sc.inverse_dynamics(q[..., half], qs[..., half], qss[..., half]))
        for got, want in zip(terms, sc.torque_terms(q[..., half], qs[..., half], qss[..., half])):
            assert np.array_equal(got[..., half], want)


@pytest.mark.parametrize("name", ["vee", "skip", "nested", "comb32"])
def test_every_path_alone_is_its_serial_chain(gpu, name):
    """With mass and inertia of every link off a root-to-leaf path set to zero, the tree's outputs on the path's joints equal the
    chain entries on chain_to(leaf) (np.array_equal: a zero's sign apart) and the joints off the path give exact zeros: what a
    fork's bank hands to a later child, and what it collects from one, pass through unchanged."""
    tree, q, qs, qss = tc.case(name)
    parents = tc.SHAPES[name]
    for leaf in tc.leaves_of(parents):
        path = tc.path_to(parents, leaf)
        off = np.array([i for i in range(len(parents)) if i not in path], dtype=int)
        alone = dict(tree, mass=tree["mass"].copy(), inertia=tree["inertia"].copy())
        alone["mass"][off] = 0.0
        alone["inertia"][off] = 0.0
        kt = tree_ref.kinematic_tree(alone)
        sc, joints = kt.chain_to(leaf)
        assert joints.tolist() == path
        qp, qsp, qssp = q[..., joints], qs[..., joints], qss[..., joints]
        outs = (kt.inverse_dynamics(q, qs, qss),) + tuple(kt.torque_terms(q, qs, qss))
        wants = (sc.inverse_dynamics(qp, qsp, qssp),) + tuple(sc.torque_terms(qp, qsp, qssp))
        for what, got, want in zip(("tau", "w0", "wa", "wb"), outs, wants):
            assert np.array_equal(got[..., joints], want), (name, leaf, what)
            assert np.all(got[..., off] == 0.0), (name, leaf, what)
        assert np.any(outs[0][..., joints] != 0.0)


@pytest.mark.parametrize("name", tc.NAMES)
def test_fused_equals_single_and_both_meet_the_reference(gpu, name):
    """Each of w0, wa, wb equals tree_inverse_dynamics_batch on the corresponding arguments, and stays within its bound of
    tests/tree_ref.py (where the magnitude is zero the values agree exactly)."""
    tree, q, qs, qss = tc.case(name)
    kt = tree_ref.kinematic_tree(tree)
    fused = dict(zip(("w0", "wa", "wb"), kt.torque_terms(q, qs, qss)))
    for key, args in tc.evaluations(q, qs, qss).items():
        assert np.array_equal(fused[key], kt.inverse_dynamics(*args)), (name, key)
    rs.check(tc, name, fused, label="%s")


def test_relabelling_the_arms(gpu):
    """torso with its two arms listed in the other order, joints and inputs permuted alike: un-permuted, the torques stay within
    twice the bound (either numbering is within the bound of the one reference)."""
    tree, q, qs, qss = tc.case("torso")
    perm = np.array([0] + list(range(8, 15)) + list(range(1, 8)))
    other = {k: (v if k in ("gravity", "tool", "parent") else v[perm]) for k, v in tree.items()}  # (the parent table is the same)
    kt = tree_ref.kinematic_tree(other)
    ref = tc.reference("torso")
    for key, got in zip(("w0", "wa", "wb"), kt.torque_terms(q[..., perm], qs[..., perm], qss[..., perm])):
        back = np.empty_like(got)
        back[..., perm] = got
        err, bound = tc.metric(back, ref[key], ref[key + "_mag"]), 2.0 * tc.bound("torso", key)
        print("relabelled torso %s: error %.3g, bound %.3g" % (key, err, bound))
        assert err <= bound, (key, err, bound)


@pytest.mark.parametrize("name", ["skip", "torso", "y18"])
def test_device_tensors_and_views_give_the_host_call_s_bits(gpu, name):
    import torch
    dev = torch.device("cuda", 0)
    tree, q, qs, qss = tc.case(name)
    d = q.shape[-1]
    kt = tree_ref.kinematic_tree(tree)
    host = kt.torque_terms(q, qs, qss)
    tq, tqs, tqss = (torch.from_numpy(np.array(v)).to(dev) for v in (q, qs, qss))
    for got, want in zip(kt.torque_terms(tq, tqs, tqss), host):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    views = [torch.repeat_interleave(t, 2, dim=1)[:, ::2] for t in (tq, tqs, tqss)]
    assert not views[0].is_contiguous()
    assert np.array_equal(kt.inverse_dynamics(*views).cpu().numpy(), host[2])
    for got, want in zip(kt.torque_terms(*views), host):
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(kt.inverse_dynamics(tq.reshape(-1, d), tqs.reshape(-1, d), tqss.reshape(-1, d)).cpu().numpy(), host[2].reshape(-1, d))
    assert np.array_equal(kt.inverse_dynamics(q[1, 3], qs[1, 3], qss[1, 3]), host[2][1, 3])


def _run_passes(inst):
    out = {"rows": inst.dense_rows()}
    out["compute_parameterization"] = inst.compute_parameterization()
    out["compute_parameterization_sd"] = inst.compute_parameterization_sd(np.full(tc.B, 8.0))
    out["compute_feasible_sets"] = inst.compute_feasible_sets()
    out["compute_controllable_sets"] = inst.compute_controllable_sets(np.zeros(tc.B), np.full(tc.B, 0.3))
    return out


@pytest.mark.parametrize("scheme", ["Collocation", "Interpolation"])
@pytest.mark.parametrize("source", ["spline", "samples"])
@pytest.mark.parametrize("per_traj", [False, True])
def test_a_tree_in_the_torque_constraint_equals_its_callback(gpu, scheme, source, per_traj):
    """BatchJointTorqueConstraint(tree, ...) against the tree's inverse dynamics as a callback, on torso at B = 3, N = 20: the
    same dense rows and the same results of every pass."""
    from toppra_amd import algorithm, batch, constraint
    tree = tc.case("torso")[0]
    kt = tree_ref.kinematic_tree(tree)
    d, B, N = 15, 3, 20
    data = batch.make_synthetic_batch(B, d, N, seed=5)
    args = (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])
    hold = np.abs(tc.reference("torso")["w0"]).max() + 5.0
    rng = np.random.default_rng(9)
    taumax = hold * (1.0 + rng.random((B, d) if per_traj else d))
    taulim, fric = np.stack([-taumax, taumax], -1), 0.05 * rng.random(d)
    DT = getattr(constraint.DiscretizationType, scheme)
    results = []
    for inv_dyn in (kt, lambda q, qd, qdd: kt.inverse_dynamics(q, qd, qdd)):
        cons = [constraint.BatchJointTorqueConstraint(inv_dyn, taulim, fric, discretization_scheme=DT)]
        if source == "spline":
            inst = algorithm.BatchTOPPRA(*args, interpolation=False, constraints=cons)
        else:
            pe = batch.path_eval_batch(*args[:3])
            inst = algorithm.BatchTOPPRA.from_path_samples(data["grid"], pe["q"], pe["qs"], pe["qss"], data["vlim"], data["alim"],
                                                           interpolation=False, constraints=cons)
        results.append(_run_passes(inst))
    rs.same(results[0], results[1], "tree vs callback")
    assert sorted(results[0]) == sorted(PASSES + ("rows",)) and np.isfinite(results[0]["rows"][0]).all()
    if source == "spline":  # the second-order spelling of the same constraint takes a tree as well, and builds the same rows
        so = constraint.BatchSecondOrderConstraint.joint_torque_constraint(kt, taulim, fric, discretization_scheme=DT)
        rs.same(algorithm.BatchTOPPRA(*args, interpolation=False, constraints=[so]).dense_rows(), results[0]["rows"], "second-order spelling")


@pytest.mark.parametrize("name", FIXTURES)
def test_against_the_reference_s_fixtures(gpu, name):
    """w0 / wa / wb within the stored accuracy bound, return codes equal, sd within the stored end-to-end tolerance (both computed
    on the CPU by tools/make_tree_golden.py)."""
    from toppra_amd import constraint
    fx = golden(name)
    tree = rs.fixture_tree(fx)
    kt = tree_ref.kinematic_tree(tree)
    q, qs, qss = sor.path_samples(fx["coef"], fx["breaks"], fx["grid"])
    mags = {k: tree_ref.rnea(tree, *args, absolute=True) for k, args in tc.evaluations(q, qs, qss).items()}
    rs.fixture_accuracy(name, fx, dict(zip(("w0", "wa", "wb"), kt.torque_terms(q, qs, qss))), mags)
    con = constraint.BatchJointTorqueConstraint(kt, fx["taulim"], fx["fric"], discretization_scheme=rs.fixture_scheme(fx, "torque_scheme")[1])
    rs.fixture_sd(name, fx, rs.fixture_instance(fx, con, interpolation=bool(int(fx["accel_scheme"]))))


def _c_call(gpu, kt, parent, q, terms):
    """The C entry on host arrays with `parent` (an int32 array, or None for NULL) in place of the tree's table:
    (rc, message, whether an output was written)."""
    lib = gpu.load()
    model, _, keep = kt.c_struct(q)
    out = [np.full_like(q, np.nan) for _ in range(3)]
    pp = None if parent is None else parent.ctypes.data
    if terms:
        rc = lib.tpr_tree_torque_terms_batch(C.byref(model), pp, q.shape[0], q.shape[1] - 1, gpu.ptr(q), gpu.ptr(q), gpu.ptr(q),
                                             gpu.ptr(out[0]), gpu.ptr(out[1]), gpu.ptr(out[2]), 0, None)
    else:
        rc = lib.tpr_tree_inverse_dynamics_batch(C.byref(model), pp, q.shape[0] * q.shape[1], gpu.ptr(q), gpu.ptr(q), gpu.ptr(q),
                                                 gpu.ptr(out[0]), 0, None)
    return rc, gpu.last_error(), not all(np.isnan(o).all() for o in out)


@pytest.mark.parametrize("terms", [False, True])
def test_the_c_entries_refuse_before_any_launch(gpu, terms):
    tree, q, _, _ = tc.case("nested")
    kt = tree_ref.kinematic_tree(tree)
    q = np.ascontiguousarray(q)
    who = "tpr_tree_torque_terms_batch" if terms else "tpr_tree_inverse_dynamics_batch"
    good = np.array(tc.SHAPES["nested"], dtype=np.int32)
    E_BADARG, E_UNSUPPORTED = -1, -3

    def with_parent(i, p):
        bad = good.copy()
        bad[i] = p
        return bad
    five = np.array([-1, 0, 0, 1, 1, 2, 2, 3, 5], dtype=np.int32)  # forks 0, 1, 2, 3, 5
    for parent, code, text in ((with_parent(4, 4), E_BADARG, "the parent of link 4 is 4, outside -1 .. 3 (links are numbered after their parents)"),
                               (with_parent(3, 7), E_BADARG, "the parent of link 3 is 7, outside -1 .. 2 (links are numbered after their parents)"),
                               (with_parent(2, -2), E_BADARG, "the parent of link 2 is -2, outside -1 .. 1 (links are numbered after their parents)"),
                               (None, E_BADARG, "null parent array"),
                               (five, E_UNSUPPORTED, "the tree has 5 forks, more than TPR_TREE_MAX_FORKS = 4")):
        assert _c_call(gpu, kt, parent, q, terms) == (code, who + ": " + text, False)
    four = np.array([-1, 0, 0, 1, 1, 2, 2, 3, 3], dtype=np.int32)  # forks 0, 1, 2, 3: TPR_TREE_MAX_FORKS of them are taken
    rc, _, wrote = _c_call(gpu, kt, four, q, terms)
    assert rc == 0 and wrote


def test_python_refuses_before_any_launch(gpu):
    from toppra_amd import algorithm, batch, constraint
    from toppra_amd.chain import KinematicTree
    tree, q, qs, qss = tc.case("nested")
    links = [tree[k] for k in ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia")]
    good = list(tc.SHAPES["nested"])
    for i, p, text in ((4, 4, "the parent of link 4 is 4, outside -1 .. 3"), (2, -2, "the parent of link 2 is -2, outside -1 .. 1")):
        bad = list(good)
        bad[i] = p
        with pytest.raises(ValueError, match=text):
            KinematicTree(bad, *links)
    with pytest.raises(ValueError, match="parents must be an integer array"):
        KinematicTree(None, *links)
    with pytest.raises(NotImplementedError, match=r"the tree has 5 forks \(links \[0, 1, 2, 3, 5\]\)"):
        KinematicTree([-1, 0, 0, 1, 1, 2, 2, 3, 5], *links)
    nan_mass = tree["mass"].copy()
    nan_mass[3] = np.nan
    with pytest.raises(ValueError, match="mass holds a value that is not finite"):
        KinematicTree(good, *(links[:4] + [nan_mass] + links[5:]))
    kt = tree_ref.kinematic_tree(tree)
    with pytest.raises(ValueError, match=r"q must have shape \[\.\.\., d\] with d = 9"):
        kt.inverse_dynamics(q[..., :8], qs[..., :8], qss[..., :8])
    # a dof mismatch with the path, told from the sizes alone
    data = batch.make_synthetic_batch(2, 7, 10, seed=1)
    con = constraint.BatchJointTorqueConstraint(kt, np.tile([-50.0, 50.0], (7, 1)), np.zeros(7))
    with pytest.raises(ValueError, match="Wrong dimension: the tree has 9 joints, the path 7 dof"):
        algorithm.BatchTOPPRA(data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"], constraints=[con]).dense_rows()
    # the library's own message reaches Python and tpr_last_error
    model, _, keep = kt.c_struct(q)
    bad = np.array(good, dtype=np.int32)
    bad[5] = 6
    rc = gpu.load().tpr_tree_inverse_dynamics_batch(C.byref(model), bad.ctypes.data, 1, gpu.ptr(q), gpu.ptr(q), gpu.ptr(q), gpu.ptr(np.empty(9)), 0, None)
    with pytest.raises(gpu.ToppraHipError, match="the parent of link 5 is 6"):
        gpu.check(rc)
    assert "the parent of link 5 is 6" in gpu.last_error()

"""The momentum kernel on the MI355X: momentum and energy2 against the numpy reference (tests/momentum_ref.py) within the accuracy
bound of tests/momentum_cases.py on every chain dof and every tree shape, on all links and on a link set, about a tilted mount;
against a second GPU route of its own (the base-reaction kernels on the gravity-free robot, the torque kernels' mass-matrix
product); the bit properties -- outputs independent of what else is asked for, the bound as the minimum of three host divisions,
a link set as the full sum on a robot whose other links weigh nothing, a chain against the tree of its links, the calling
conventions, the +0 of a standstill --; ``BatchMomentumConstraint`` against the same bound made on the host, alone and beside
second-order constraints on the same robot; and the reference's fixtures.

Accuracy: the bound is 16 x the float64 reference's own error against np.longdouble, per case, link set and quantity;
profiles/momentum_accuracy.json holds the yardsticks, the bounds and the measured errors.  Measured on the MI355X the kernel uses
at most 0.43 of a bound over the 16 cases and both link sets (momentum of the 32-dof chain), at most 0.13 of the stored bound on
the reference's fixtures and 0.11 of the allowance of their boxes, and reproduces their sd to 1.7e-16 / 3.9e-16 (tolerances
1.0e-13 / 3.1e-10)."""
import ctypes

import numpy as np
import pytest

from tests import base_wrench_cases as bw, base_wrench_ref as bwr, chain_cases as cc, chain_ref, momentum_cases as mc, momentum_ref as mr
from tests import rigid_support as rs, second_order_ref as sor, tree_cases as tc, tree_ref
from tests.helpers import golden

pytestmark = pytest.mark.gpu
FIXTURES = ("momentum_d6_N40", "momentum_torso_d15_N30")
KINDS = ("linear", "angular", "energy")
EPS = np.finfo(float).eps


def _mount():
    return bwr.mount_of(dict(mc.MOUNT))


def _positive_zeros(*arrays):
    for v in arrays:
        v = np.asarray(v)
        assert not np.signbit(v[v == 0]).any()


@pytest.mark.parametrize("key", mc.CASES)
def test_kernel_against_the_numpy_reference(gpu, key):
    """Every case, both link sets, about the mount; no negative zero; the trajectory that stands still is +0 throughout."""
    from toppra_amd import batch
    robot, q, qs, _ = mc.case(key)
    model, ref = bwr.robot_of(robot), mc.reference(key)
    for which in mc.SETS:
        h, e2 = batch.momentum_batch(model, q, qs, _mount(), mc.link_set(key, which))
        assert h.shape == q.shape[:2] + (6,) and e2.shape == q.shape[:2]
        for quantity, got in (("momentum", h), ("energy2", e2)):
            name = mc.name_of(quantity, which)
            err, bound = mc.metric(got, ref[name], ref[name + "_mag"]), mc.bound(key, name)
            print("ACCURACY case %s %s error %.3g bound %.3g fraction %.2f" % (key, name, err, bound, err / bound if bound else 0.0))
            assert err <= bound, (key, name, err, bound)
        _positive_zeros(h, e2)
        still = mc.still(key)
        assert not h[still].any() and not e2[still].any() and not np.signbit(h[still]).any() and not np.signbit(e2[still]).any()
        assert np.all(e2 >= 0.0)
        if mc.bound(key, mc.name_of("energy2", which)) > 0:
            assert np.all(e2[0] > 0.0) and np.abs(h[0]).max() > 0.0
        # the robots' own methods are this entry: momentum in the mount frame, half of energy2
        assert np.array_equal(model.momentum(q, qs, _mount(), mc.link_set(key, which)), h)
        assert np.array_equal(model.kinetic_energy(q, qs, mc.link_set(key, which)), 0.5 * e2)


@pytest.mark.parametrize("key", (7, 9, "torso", "nested"))
def test_a_second_gpu_route(gpu, key):
    """momentum = the base reaction of the gravity-free robot at (q, 0, qs): at zero velocity the net force and moment are the
    momentum's with qs in place of the velocity.  energy2 = sum_j qs_j (wa - w0)_j of the torque kernels: wa - w0 = M(q) qs.  The
    allowance is the sum of the two families' committed bounds, each on its own all-absolute magnitude, plus the rounding of the
    host's own sum."""
    from toppra_amd import batch
    from toppra_amd.chain import Mount
    robot, q, qs, qss = mc.case(key)
    model, ref = bwr.robot_of(robot), mc.reference(key)
    h, e2 = batch.momentum_batch(model, q, qs, _mount())
    frame = Mount(rotation=mc.MOUNT["rot"], origin=mc.MOUNT["origin"])
    floating = bwr.robot_of(dict(robot, gravity=np.zeros(3)))
    w = batch.base_wrench_batch(floating, q, np.zeros_like(q), qs, frame)
    allow = mc.bound(key, "momentum") * ref["momentum_mag"] + bw.bound(key, "wa") * bw.reference(key)["wa_mag"]
    off = np.abs(h - w)
    print("%s: |momentum - base wrench(q, 0, qs)| at most %.3g of its allowance" % (key, float(np.max(off[allow > 0] / allow[allow > 0]))))
    assert np.all(off <= allow) and np.abs(w).max() > 0
    cases = tc if isinstance(key, str) else cc
    terms = batch.tree_torque_terms_batch if isinstance(key, str) else batch.chain_torque_terms_batch
    w0, wa, _ = terms(model, q, qs, qss)
    tref = cases.reference(key)
    route = np.sum(qs * (wa - w0), -1)
    allow = mc.bound(key, "energy2") * ref["energy2_mag"] + np.sum(np.abs(qs) * (
        cases.bound(key, "wa") * tref["wa_mag"] + cases.bound(key, "w0") * tref["w0_mag"] + 2 * q.shape[-1] * EPS * (np.abs(wa) + np.abs(w0))), -1)
    off = np.abs(e2 - route)
    live = allow > 0
    print("%s: |energy2 - qs . (wa - w0)| at most %.3g of its allowance" % (key, float(np.max(off[live] / allow[live]))))
    assert np.all(off <= allow) and np.array_equal(off[~live], np.zeros((~live).sum()))


# ---- bit properties ---------------------------------------------------------------------------------------------------------

def _raw(model, q, qs, mount, mask, limit, want):
    """The C entry on host arrays with any subset of its outputs: (momentum, energy2, xbound), None where not asked for."""
    from toppra_amd import _capi, batch
    lib = _capi.load()
    links, parent, keep = model.as_tree(q)
    B, n1, d = q.shape
    q, qs = np.ascontiguousarray(q), np.ascontiguousarray(qs)
    outs = [np.full(shape, np.nan) if given else None for given, shape in zip(want, ((B, n1, 6), (B, n1), (B, n1, 2)))]
    lim = None if limit is None else np.ascontiguousarray(np.broadcast_to(limit, (B, 3)), dtype=np.float64)
    frame = mount.c_struct()
    rc = lib.tpr_tree_momentum_batch(ctypes.byref(links), parent.ctypes.data, ctypes.byref(frame), mask, B, n1 - 1, q.ctypes.data, qs.ctypes.data,
                                     None if lim is None else lim.ctypes.data, *[None if o is None else o.ctypes.data for o in outs], 0, None)
    assert rc == 0, lib.tpr_last_error()
    return outs


@pytest.mark.parametrize("key", (3, 17, "skip", "comb32"))
def test_each_output_is_the_same_whatever_else_is_asked_for(gpu, key):
    from toppra_amd import batch
    robot, q, qs, _ = mc.case(key)
    model, mount = bwr.robot_of(robot), _mount()
    mask = batch.link_mask(model, mc.link_set(key, "set"))
    rng = np.random.default_rng(4)
    limit = rng.uniform(0.5, 2.0, (q.shape[0], 3))
    h, e2, xb = _raw(model, q, qs, mount, mask, limit, (True, True, True))
    assert np.isfinite(h).all() and np.isfinite(e2).all() and not np.isnan(xb).any()
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        for lim in (limit, None) if not want[2] else (limit,):
            got = _raw(model, q, qs, mount, mask, lim, want)
            for a, b in zip(got, (h, e2, xb)):
                assert a is None or np.array_equal(a, b), want
    # other limits, a term switched off: momentum and energy2 do not move
    off = limit.copy()
    off[:, 1] = np.inf
    h2, e22, xb2 = _raw(model, q, qs, mount, mask, off, (True, True, True))
    assert np.array_equal(h2, h) and np.array_equal(e22, e2) and np.all(xb2[..., 1] >= xb[..., 1])
    assert np.array_equal(xb2, mr.xbound(h, e2, off))


@pytest.mark.parametrize("key", (1, 8, 32, "vee", "roots", "y18"))
def test_the_bound_is_the_minimum_of_three_host_divisions(gpu, key):
    from toppra_amd import batch
    robot, q, qs, _ = mc.case(key)
    model = bwr.robot_of(robot)
    B = q.shape[0]
    for links, limit in ((None, np.array([0.7, 1.3, 0.9])), (mc.link_set(key, "set"), np.random.default_rng(8).uniform(0.1, 3.0, (B, 3))),
                         (None, np.array([np.inf, 2.0, np.inf])), (None, np.full(3, np.inf))):
        h, e2, xb = batch.momentum_batch(model, q, qs, _mount(), links, limit)
        assert xb.shape == q.shape[:2] + (2,)
        assert np.array_equal(xb, mr.xbound(h, e2, limit)) and not xb[..., 0].any() and not np.signbit(xb[..., 0]).any()
        assert np.all(np.isposinf(xb[mc.still(key), :, 1]))  # a standstill: 1 / 0
        plain = batch.momentum_batch(model, q, qs, _mount(), links)
        assert len(plain) == 2 and np.array_equal(plain[0], h) and np.array_equal(plain[1], e2)
        if np.isinf(limit).all():
            assert np.all(np.isposinf(xb[..., 1]))


@pytest.mark.parametrize("key", (8, 32, "torso", "nested", "roots", "comb32"))
def test_a_link_set_is_the_full_sum_with_the_other_links_weightless(gpu, key):
    """Skipped links against links of mass 0 and inertia 0 that are walked and summed: every bit, the bound included."""
    from toppra_amd import batch
    robot, q, qs, _ = mc.case(key)
    links = mr.link_set(robot, mc.link_set(key, "set"))
    hollow = dict(robot, mass=np.array(robot["mass"]), inertia=np.array(robot["inertia"]))
    for i in range(len(robot["mass"])):
        if i not in links:
            hollow["mass"][i] = 0.0
            hollow["inertia"][i] = 0.0
    limit = np.array([0.4, 0.6, 0.8])
    a = batch.momentum_batch(bwr.robot_of(robot), q, qs, _mount(), links, limit)
    b = batch.momentum_batch(bwr.robot_of(hollow), q, qs, _mount(), None, limit)
    for x, y in zip(a, b):
        assert np.array_equal(x, y) and np.array_equal(np.signbit(x), np.signbit(y))
    assert np.abs(a[0]).max() > 0


@pytest.mark.parametrize("d", mc.DOFS)
def test_a_chain_and_the_tree_of_its_links_are_bit_equal(gpu, d):
    from toppra_amd import batch
    from toppra_amd.chain import KinematicTree
    chain, q, qs, _ = mc.case(d)
    sc = chain_ref.serial_chain(chain)
    tree = KinematicTree.from_chain(sc)
    limit = np.array([0.5, 0.25, 2.0])
    for links in (None, mc.link_set(d, "set"), [-1]):
        for a, b in zip(batch.momentum_batch(sc, q, qs, _mount(), links, limit), batch.momentum_batch(tree, q, qs, _mount(), links, limit)):
            assert np.array_equal(a, b)
    assert np.array_equal(sc.momentum(q, qs), tree.momentum(q, qs)) and np.array_equal(sc.kinetic_energy(q, qs), tree.kinetic_energy(q, qs))


@pytest.mark.parametrize("key", (1, 7, 32, "nested", "comb32"))
def test_device_tensors_and_views_give_the_host_call_s_bits(gpu, key):
    """torch tensors on the device, contiguous and as a non-contiguous view, a flattened shape, a single point; a device limit."""
    from toppra_amd import batch
    torch, dev = rs.torch_device()
    robot, q, qs, _ = mc.case(key)
    d = q.shape[-1]
    model, mount, links = bwr.robot_of(robot), _mount(), mc.link_set(key, "set")
    limit = np.random.default_rng(2).uniform(0.2, 2.0, (q.shape[0], 3))
    host = batch.momentum_batch(model, q, qs, mount, links, limit)
    tq, tqs = (torch.from_numpy(np.array(v)).to(dev) for v in (q, qs))
    for lim in (limit, torch.from_numpy(limit).to(dev)):
        for got, want in zip(batch.momentum_batch(model, tq, tqs, mount, links, lim), host):
            assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    views = [torch.repeat_interleave(t, 2, dim=1)[:, ::2] for t in (tq, tqs)]
    assert not views[0].is_contiguous()
    for got, want in zip(batch.momentum_batch(model, *views, mount, links, limit), host):
        assert np.array_equal(got.cpu().numpy(), want)
    flat = batch.momentum_batch(model, tq.reshape(-1, d), tqs.reshape(-1, d), mount, links)
    assert tuple(flat[0].shape) == (q.shape[0] * q.shape[1], 6) and np.array_equal(flat[0].cpu().numpy(), host[0].reshape(-1, 6))
    assert tuple(flat[1].shape) == (q.shape[0] * q.shape[1],) and np.array_equal(flat[1].cpu().numpy(), host[1].reshape(-1))
    one = batch.momentum_batch(model, q[0, 3], qs[0, 3], mount, links)
    assert one[0].shape == (6,) and one[1].shape == () and np.array_equal(one[0], host[0][0, 3]) and np.array_equal(one[1], host[1][0, 3])
    assert np.array_equal(model.momentum(tq, tqs, mount, links).cpu().numpy(), host[0])
    assert np.array_equal(model.kinetic_energy(tq, tqs, links).cpu().numpy(), 0.5 * host[1])


@pytest.mark.parametrize("kind", ("chain", "torso"))
def test_a_standstill_is_a_positive_zero_and_leaves_the_box(gpu, kind):
    """q' = 0 at a gridpoint: momentum, energy2 are +0, each division gives +inf and the stage keeps the 1e8 of the box; so does a
    trajectory that stands still throughout."""
    from toppra_amd import algorithm, batch, constraint
    key = 3 if kind == "chain" else "torso"
    robot, q, qs, qss = mc.case(key)
    model = bwr.robot_of(robot)
    qs = np.array(qs)
    qs[:, 7] = 0.0
    qs[:, 9] = -0.0  # (negative zeros in: the products vanish with either sign)
    h, e2, xb = batch.momentum_batch(model, q, qs, _mount(), None, np.array([0.3, 0.2, 0.1]))
    still = mc.still(key)
    for at in ((slice(None), 7), (slice(None), 9), (still, slice(None))):
        for v in (h[at], e2[at]):
            assert not v.any() and not np.signbit(v).any()
        assert np.all(np.isposinf(xb[at][..., 1])) and not xb[at][..., 0].any()
    B, n1, d = q.shape
    grid = np.linspace(0.0, 1.0, n1)
    alim = np.tile([-50.0, 50.0], (B, d, 1))
    con = constraint.BatchMomentumConstraint(model, linear=0.5, angular=0.4, energy=0.3, mount=_mount())
    low, high = algorithm.BatchTOPPRA.from_path_samples(grid, q, qs, qss, None, alim, constraints=[con]).stage_boxes()
    assert np.all(high[:, 7, 1] == 1e8) and np.all(high[:, 9, 1] == 1e8) and np.all(high[still, :, 1] == 1e8)
    moving = [b for b in range(B) if b != still]
    assert np.all(high[moving, 8, 1] < 1e8) and np.all(low[..., 1] == 0.0)


# ---- the constraint ---------------------------------------------------------------------------------------------------------

def _robot(kind):
    return cc.case(7)[0] if kind == "chain" else tc.case("torso")[0]


def _host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def _physical_limits(model, mount, links, args, per_traj, fraction=0.6):
    """{kind: a scalar or [B]} in physical units: ``fraction`` of each quantity's peak along the path at the speed the velocity
    limits allow -- so at that peak's gridpoint the bound lies below the velocity box and binds, and x = 0 stays feasible."""
    from toppra_amd import batch
    pe = batch.path_eval_batch(*args[:3])
    h, ke = model.momentum(pe["q"], pe["qs"], mount, links), model.kinetic_energy(pe["q"], pe["qs"], links)
    xmax = sor.velocity_box(pe["qs"], args[3])[1][..., 1]
    peaks = {"linear": np.sqrt((h[..., :3] ** 2).sum(-1) * xmax).max(-1), "angular": np.sqrt((h[..., 3:] ** 2).sum(-1) * xmax).max(-1),
             "energy": (ke * xmax).max(-1)}
    return {k: fraction * (v if per_traj else v.max()) for k, v in peaks.items()}, pe, h, ke


CONSTRAINT_CASES = [("numpy", False, "chain", ("linear",)), ("torch", True, "chain", ("angular",)), ("numpy", True, "chain", ("energy",)),
                    ("torch", False, "chain", KINDS), ("numpy", True, "chain", KINDS), ("torch", False, "torso", ("linear",)),
                    ("numpy", True, "torso", ("angular",)), ("torch", True, "torso", ("energy",)), ("numpy", False, "torso", KINDS),
                    ("torch", True, "torso", KINDS)]


@pytest.mark.parametrize("kind,per_traj,robot_kind,which", CONSTRAINT_CASES)
def test_the_constraint_equals_a_host_made_bound(gpu, kind, per_traj, robot_kind, which):
    """Against BatchBoundConstraint(xbound) with the bound made on the host from robot.momentum / kinetic_energy: stage_boxes() and
    every pass, bit for bit; status 0; the limit tightens a box below the velocity box."""
    from toppra_amd import algorithm, constraint
    robot = _robot(robot_kind)
    model, mount = bwr.robot_of(robot), _mount()
    links = None if robot_kind == "chain" else mc.link_set("torso", "set")
    data, args = rs.problem(len(robot["mass"]), seed=6)
    limits, pe, h, ke = _physical_limits(model, mount, links, args, per_traj)
    limits = {k: v for k, v in limits.items() if k in which}
    lim = np.full((cc.B, 3), np.inf)
    for k, v in limits.items():
        lim[:, KINDS.index(k)] = 2.0 * v if k == "energy" else v * v
    xbound = mr.xbound(h, 2.0 * ke, lim)
    ours_limits = dict(limits)
    if kind == "torch":
        torch, dev = rs.torch_device()
        args = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in args)
        xbound = torch.from_numpy(xbound).to(dev)
        if per_traj:
            ours_limits = {k: torch.from_numpy(v).to(dev) for k, v in limits.items()}
    con = constraint.BatchMomentumConstraint(model, mount=mount, links=links, **ours_limits)
    assert np.array_equal(np.broadcast_to(con.limit, (cc.B, 3)), lim)
    ours = algorithm.BatchTOPPRA(*args, constraints=[con])
    theirs = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchBoundConstraint(xbound=xbound)])
    for a, b in zip(ours.stage_boxes(), theirs.stage_boxes()):
        assert np.array_equal(_host(a), _host(b))
    results = []
    for inst in (ours, theirs):
        out = rs.run_passes(inst)
        results.append({k: ({n: _host(x) for n, x in v.items()} if isinstance(v, dict) else [_host(x) for x in v] if isinstance(v, (tuple, list))
                            else _host(v)) for k, v in out.items()})
    rs.same(results[0], results[1], "constraint vs host-made bound")
    for k in ("compute_parameterization", "compute_parameterization_sd"):
        assert np.all(results[0][k]["status"] == 0), k
    high = _host(ours.stage_boxes()[1])[..., 1]
    box = sor.velocity_box(_host(pe["qs"]), data["vlim"])[1][..., 1]
    assert np.all(high <= box) and (high < box).any(), "the limit tightens no box"
    if per_traj:  # (a limit of its own binds in every trajectory: at the peak it was taken from)
        assert all((high[b] < box[b]).any() for b in range(cc.B)), "a trajectory's limit never binds"


@pytest.mark.parametrize("robot_kind", ("chain", "torso"))
def test_all_three_limits_are_at_most_each_single_one(gpu, robot_kind):
    from toppra_amd import algorithm, constraint
    robot = _robot(robot_kind)
    model, mount = bwr.robot_of(robot), _mount()
    links = None if robot_kind == "chain" else mc.link_set("torso", "set")
    data, args = rs.problem(len(robot["mass"]), seed=6)
    limits = _physical_limits(model, mount, links, args, True)[0]
    boxes = lambda **kw: algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchMomentumConstraint(model, mount=mount, links=links, **kw)]).stage_boxes()[1]  # noqa: E731
    both = boxes(**limits)
    for k in KINDS:
        single = boxes(**{k: limits[k]})
        assert np.all(both <= single) and (both < single).any(), k
        assert np.array_equal(both[..., 0], single[..., 0])  # (the u column is nobody's)


def test_beside_second_order_constraints_and_a_point_speed_limit(gpu):
    """[torque, base wrench, point speed, momentum] on one 7-dof arm: the boxes are those of the two first-order constraints alone,
    the dense rows those of the list without the momentum limit; every pass runs and every trajectory is feasible."""
    from toppra_amd import algorithm, batch, constraint
    from toppra_amd.chain import ControlPoints
    robot = dict(_robot("chain"), gravity=np.array([0.0, 0.0, -9.81]))
    d = len(robot["mass"])
    model, mount = bwr.robot_of(robot), _mount()
    data, args = rs.problem(d, seed=8)
    limits, pe, _, _ = _physical_limits(model, mount, None, args, False)
    taumax = np.abs(model.torque_terms(pe["q"], pe["qs"], pe["qss"])[0]).max() + 20.0
    w0, wa, wb = model.base_wrench_terms(pe["q"], pe["qs"], pe["qss"], mount)
    peak = np.max([np.abs(v).max((0, 1)) for v in (w0, wa, wb)], 0)
    pts = ControlPoints([3, -1], [[0.1, 0.0, 0.2], [0.0, 0.1, 0.1]])
    # (0.45 of the points' peak squared speed at the velocity limits, beside 0.6 of the momentum's and the energy's peaks: chosen
    # with the numpy references so that each of the two first-order limits is the tighter one at some gridpoints -- at 0.35 the
    # speed limit hides the momentum limit everywhere, at 0.55 it is hidden itself; both are asserted below)
    speed = constraint.BatchPointSpeedConstraint(model, pts, 0.45 * (model.point_speeds(pe["q"], pe["qs"], pts) *
                                                                       sor.velocity_box(pe["qs"], data["vlim"])[1][..., 1:]).max())
    moment = constraint.BatchMomentumConstraint(model, mount=mount, **limits)
    second = [constraint.BatchJointTorqueConstraint(model, np.tile([-taumax, taumax], (d, 1)), np.zeros(d)),
              constraint.BatchBaseWrenchConstraint(model, mount, force=1.5 * peak[:3].max(), moment=1.5 * peak[3:].max())]
    full = algorithm.BatchTOPPRA(*args, constraints=[second[0], second[1], speed, moment])
    out = rs.run_passes(full)
    assert out["rows"][0].shape[-1] == 2 + 4 * d + 2 * d + 24
    first = algorithm.BatchTOPPRA(*args, constraints=[speed, moment]).stage_boxes()
    assert np.array_equal(out["rows"][3], first[0]) and np.array_equal(out["rows"][4], first[1])
    without = algorithm.BatchTOPPRA(*args, constraints=[second[0], second[1], speed]).dense_rows()
    for k in range(3):
        assert np.array_equal(out["rows"][k], without[k]) and np.isfinite(out["rows"][k]).all()
    assert (out["rows"][4][..., 1] < without[4][..., 1]).any(), "the momentum limit tightens no box beside the speed limit"
    alone = algorithm.BatchTOPPRA(*args, constraints=[moment]).stage_boxes()[1]
    assert (out["rows"][4][..., 1] < alone[..., 1]).any(), "the speed limit tightens no box beside the momentum limit"
    for k in ("compute_parameterization", "compute_parameterization_sd"):
        assert np.all(out[k]["status"] == 0), k
    # ... and the same list on a from_path_samples batch that carries q
    samples = algorithm.BatchTOPPRA.from_path_samples(data["grid"], pe["q"], pe["qs"], pe["qss"], data["vlim"], data["alim"],
                                                      constraints=[second[0], second[1], speed, moment])
    rows = samples.dense_rows()
    assert np.array_equal(rows[4], out["rows"][4]) and np.array_equal(rows[3], out["rows"][3])


# ---- the reference's fixtures ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_against_the_reference_s_fixtures(gpu, name):
    """The kernel's outputs within the stored accuracy bound; high[..., 1] within that bound composed through the division; every
    other box entry, and the return codes, equal; sd within the stored end-to-end tolerance (tools/make_momentum_golden.py)."""
    from toppra_amd import batch, constraint
    from toppra_amd.chain import Mount
    fx = golden(name)
    robot = rs.fixture_tree(fx)
    model, frame = tree_ref.kinematic_tree(robot), Mount(rotation=fx["mount_rot"], origin=fx["mount_origin"])
    links = [int(i) for i in fx["links"]]
    q, qs, _ = sor.path_samples(fx["coef"], fx["breaks"], fx["grid"])
    h, e2, xb = batch.momentum_batch(model, q, qs, frame, links, fx["limit"])
    rs.fixture_accuracy(name, fx, {"momentum": h, "energy2": e2}, {k: fx[k + "_mag"] for k in ("momentum", "energy2")})
    limits = {k: fx["limit_" + k] for k in KINDS if "limit_" + k in fx}
    assert len(limits) == 2 and all(v.shape == (q.shape[0],) for v in limits.values())
    con = constraint.BatchMomentumConstraint(model, mount=frame, links=links, **limits)
    assert np.array_equal(con.limit, fx["limit"])  # (the class squares and doubles as the generator did)
    inst = rs.fixture_instance(fx, con)
    low, high = inst.stage_boxes()
    tol = mr.xbound_tolerance(fx["momentum"], fx["momentum_mag"], fx["energy2"], fx["energy2_mag"], fx["limit"], *fx["acc_bound"])
    assert np.array_equal(low, fx["low"]) and np.array_equal(high[..., 0], fx["high"][..., 0])
    off = np.abs(high[..., 1] - fx["high"][..., 1])
    print("ACCURACY fixture %s high error_over_allowance %.3g" % (name, float(np.max(off[tol > 0] / tol[tol > 0]))))
    assert np.all(off <= tol)
    assert (fx["high"][..., 1] == fx["xbound"][..., 1]).sum(-1).min() >= (q.shape[1] + 3) // 4  # the bound, not the velocity box
    rs.fixture_sd(name, fx, inst)

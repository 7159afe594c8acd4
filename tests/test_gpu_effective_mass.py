"""The effective-mass kernel on the MI355X: speed2 and mobility against the np.longdouble restatement of its walk
(tests/effective_mass_ref.py) within the accuracy bound of tests/effective_mass_cases.py on every chain dof and every tree shape;
the bit properties -- a chain against the tree of its links, each output alone against all together, a point alone against inside
the 16-set and the set reversed, the bound as the host's divisions and minimum on the kernel's own outputs, the calling conventions,
the direction mode against the velocity mode --; a cross-kernel check (Cauchy-Schwarz against the momentum kernel's energy2; speed2
against the control-point speed kernel); the +0 of a standstill; and ``BatchContactEnergyConstraint`` against the same bound handed
to ``BatchBoundConstraint``, in every pass, alone and beside a torque and a momentum limit, and against the total-energy limit it
refines.

Accuracy: the metric is the relative error; the yardstick, per case, point set and quantity, the larger of the float64
restatement's and the float64 dense route's distance to the longdouble restatement; the bound 16 x that.
profiles/effective_mass_accuracy.json holds the yardsticks, the bounds and the fractions the kernel used."""
import ctypes

import numpy as np
import pytest

from tests import chain_cases as cc, chain_ref, control_points_cases as cpc, effective_mass_cases as ec, effective_mass_ref as er
from tests import rigid_support as rs, second_order_ref as sor, tree_ref
from tests.helpers import golden

pytestmark = pytest.mark.gpu
FIXTURES = ("contact_energy_d6_N40", "contact_energy_torso_d15_N30")
EPS = np.finfo(float).eps


def _host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else v


@pytest.mark.parametrize("key", ec.CASES)
def test_kernel_against_the_reference(gpu, key):
    """Every case, every point set; no negative zero; the trajectory that stands still is +0 throughout."""
    from toppra_amd import contact
    robot, q, qs = ec.case(key)
    model, ref = ec.robot_of(key), ec.reference(key)
    for which in ec.sets_of(key):
        pts = ec.control_points(key, which)
        s2, g, xb = contact.effective_mass_batch(model, q, qs, pts)
        assert xb is None and s2.shape == g.shape == q.shape[:2] + (len(pts),)
        for quantity, got in zip(ec.QUANTITIES, (s2, g)):
            name = ec.name_of(quantity, which)
            err, bound = ec.relative_error(got, ref[name]), ec.bound(key, name)
            print("ACCURACY case %s %s error %.3g yardstick %.3g bound %.3g fraction %.2f" % (key, name, err, ref["yardstick"][name], bound, err / bound))
            assert err <= bound, (key, name, err, bound)
            assert not np.signbit(got).any() and np.isfinite(got).all()
        still = np.flatnonzero(~np.asarray(qs).any((1, 2)))
        assert len(still) == 1 and not s2[still].any() and not g[still].any()
        moving = [b for b in range(q.shape[0]) if b != still[0]]
        assert np.all(s2[moving] > 0) and np.all(g[moving] > 0)
        # the robots' own methods are this entry
        with np.errstate(invalid="ignore"):
            assert np.array_equal(model.effective_mass(q, qs, pts), s2 / g, equal_nan=True)
        assert np.isnan(model.effective_mass(q, qs, pts)[still]).all()


# ---- bit properties ---------------------------------------------------------------------------------------------------------

def _raw(model, pts, q, qs, limit, want, directions=None):
    """The C entry on host arrays with any subset of its outputs: (speed2, mobility, xbound), None where not asked for."""
    from toppra_amd import contact
    lib = contact.load()
    links, parent, keep = model.as_tree(q)
    B, n1, d = q.shape
    P = len(pts)
    q = np.ascontiguousarray(q)
    qs = None if qs is None else np.ascontiguousarray(qs)
    outs = [np.full(shape, np.nan) if given else None for given, shape in zip(want, ((B, n1, P), (B, n1, P), (B, n1, 2)))]
    lim = None if limit is None else np.ascontiguousarray(np.broadcast_to(limit, (B, P, 2)), dtype=np.float64)
    u = None if directions is None else np.ascontiguousarray(directions, dtype=np.float64)
    c_pts = pts.c_struct(model)
    rc = lib.tpr_tree_effective_mass_batch(ctypes.byref(links), parent.ctypes.data, ctypes.byref(c_pts), None if u is None else u.ctypes.data,
                                           B, n1 - 1, q.ctypes.data, None if qs is None else qs.ctypes.data,
                                           None if lim is None else lim.ctypes.data, *[None if o is None else o.ctypes.data for o in outs], 0, None)
    assert rc == 0, lib.tpr_last_error()
    return outs


def _limit(B, P, seed=4):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.5, 2.0, (B, P)), rng.uniform(0.0, 0.5, (B, P))], -1)


@pytest.mark.parametrize("d", ec.DOFS)
def test_a_chain_and_the_tree_of_its_links_are_bit_equal(gpu, d):
    from toppra_amd import contact
    from toppra_amd.chain import KinematicTree
    _, q, qs = ec.case(d)
    sc = ec.robot_of(d)
    tree = KinematicTree.from_chain(sc)
    for which in ec.sets_of(d):
        pts = ec.control_points(d, which)
        limit = _limit(q.shape[0], len(pts))
        for a, b in zip(contact.effective_mass_batch(sc, q, qs, pts, limit), contact.effective_mass_batch(tree, q, qs, pts, limit)):
            assert np.array_equal(a, b)
        assert np.array_equal(sc.contact_energy(q, qs, pts, 5.0), tree.contact_energy(q, qs, pts, 5.0))


@pytest.mark.parametrize("key", (3, 17, "skip", "comb32"))
def test_each_output_is_the_same_whatever_else_is_asked_for(gpu, key):
    _, q, qs = ec.case(key)
    model, pts = ec.robot_of(key), ec.control_points(key, "set")
    limit = _limit(q.shape[0], len(pts))
    s2, g, xb = _raw(model, pts, q, qs, limit, (True, True, True))
    assert np.isfinite(s2).all() and np.isfinite(g).all() and not np.isnan(xb).any()
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        for lim in (limit, None) if not want[2] else (limit,):
            for a, b in zip(_raw(model, pts, q, qs, lim, want), (s2, g, xb)):
                assert a is None or np.array_equal(a, b), want
    # other limits: speed2 and mobility do not move
    s2b, gb, xbb = _raw(model, pts, q, qs, 2.0 * limit, (True, True, True))
    assert np.array_equal(s2b, s2) and np.array_equal(gb, g) and np.array_equal(xbb, er.xbound(s2, g, 2.0 * limit))


@pytest.mark.parametrize("key", (1, 7, 32, "torso", "comb32"))
def test_a_point_s_bits_do_not_depend_on_the_set(gpu, key):
    """Each point of the 16-set alone, and the set reversed, against the set: speed2 and mobility in every bit."""
    from toppra_amd import contact
    from toppra_amd.chain import ControlPoints
    _, q, qs = ec.case(key)
    model = ec.robot_of(key)
    links, offsets = ec.point_set(key, "full")
    s2, g, _ = contact.effective_mass_batch(model, q, qs, ec.control_points(key, "full"))
    r2, rg, _ = contact.effective_mass_batch(model, q, qs, ControlPoints(list(links)[::-1], offsets[::-1]))
    assert np.array_equal(r2[..., ::-1], s2) and np.array_equal(rg[..., ::-1], g)
    for p in (0, 5, 15):
        a2, ag, _ = contact.effective_mass_batch(model, q, qs, ControlPoints([links[p]], offsets[p:p + 1]))
        assert np.array_equal(a2[..., 0], s2[..., p]) and np.array_equal(ag[..., 0], g[..., p]), p


def test_a_root_without_a_point_is_skipped(gpu):
    """A forest's second root alone: the points on it give the bits they give beside points on the first root, whose tree is then
    walked too."""
    from toppra_amd import contact
    from toppra_amd.chain import ControlPoints
    roots = ec.robot_of("roots")
    _, rq, rqs = ec.case("roots")
    rl, ro = ec.point_set("roots", "set")
    both = contact.effective_mass_batch(roots, rq, rqs, ControlPoints(list(rl), ro))
    upper = [p for p, k in enumerate(rl) if k >= 9]
    assert 0 < len(upper) < len(rl)
    alone = contact.effective_mass_batch(roots, rq, rqs, ControlPoints([rl[p] for p in upper], ro[upper]))
    assert np.array_equal(alone[0], both[0][..., upper]) and np.array_equal(alone[1], both[1][..., upper])


@pytest.mark.parametrize("key", (1, 8, 32, "vee", "roots", "y18"))
def test_the_bound_is_the_host_s_divisions_and_minimum(gpu, key):
    from toppra_amd import contact
    _, q, qs = ec.case(key)
    model, pts = ec.robot_of(key), ec.control_points(key, "set")
    B, P = q.shape[0], len(pts)
    for limit in (np.array([1.0, 0.0]) * np.ones((P, 2)), _limit(B, P, 8)[0], _limit(B, P, 9)):
        s2, g, xb = contact.effective_mass_batch(model, q, qs, pts, limit)
        assert xb.shape == q.shape[:2] + (2,)
        assert np.array_equal(xb, er.xbound(s2, g, limit)) and not xb[..., 0].any() and not np.signbit(xb[..., 0]).any()
        still = np.flatnonzero(~np.asarray(qs).any((1, 2)))[0]
        assert np.all(np.isposinf(xb[still, :, 1])) and np.isfinite(np.delete(xb, still, 0)).all()
        assert np.array_equal(contact.effective_mass_bound_batch(model, q, qs, pts, limit), xb)
    # the direction mode's bound takes g for 1 / m_R
    u = np.tile([0.0, 0.6, 0.8], (P, 1))
    limit = _limit(B, P, 10)
    s2, g, xb = contact.effective_mass_batch(model, q, qs, pts, limit, directions=u)
    assert np.array_equal(xb, er.xbound(s2, g, limit, directed=True))


@pytest.mark.parametrize("key", (1, 7, 32, "nested", "comb32"))
def test_device_tensors_and_views_give_the_host_call_s_bits(gpu, key):
    """torch tensors on the device, contiguous and as a non-contiguous view, a flattened shape, a single point; a device limit."""
    from toppra_amd import contact
    torch, dev = rs.torch_device()
    _, q, qs = ec.case(key)
    d = q.shape[-1]
    model, pts = ec.robot_of(key), ec.control_points(key, "set")
    P = len(pts)
    limit = _limit(q.shape[0], P, 2)
    host = contact.effective_mass_batch(model, q, qs, pts, limit)
    tq, tqs = (torch.from_numpy(np.array(v)).to(dev) for v in (q, qs))
    for lim in (limit, torch.from_numpy(limit).to(dev)):
        for got, want in zip(contact.effective_mass_batch(model, tq, tqs, pts, lim), host):
            assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    views = [torch.repeat_interleave(t, 2, dim=1)[:, ::2] for t in (tq, tqs)]
    assert not views[0].is_contiguous()
    for got, want in zip(contact.effective_mass_batch(model, *views, pts, limit), host):
        assert np.array_equal(got.cpu().numpy(), want)
    flat = contact.effective_mass_batch(model, tq.reshape(-1, d), tqs.reshape(-1, d), pts)
    assert flat[2] is None and tuple(flat[0].shape) == (q.shape[0] * q.shape[1], P)
    assert np.array_equal(flat[0].cpu().numpy(), host[0].reshape(-1, P)) and np.array_equal(flat[1].cpu().numpy(), host[1].reshape(-1, P))
    one = contact.effective_mass_batch(model, q[0, 3], qs[0, 3], pts)
    assert one[0].shape == (P,) and np.array_equal(one[0], host[0][0, 3]) and np.array_equal(one[1], host[1][0, 3])
    energy = model.contact_energy(q, qs, pts, 4.0)
    assert np.array_equal(model.contact_energy(tq, tqs, pts, 4.0).cpu().numpy(), energy)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(energy, np.where(host[0] == 0, 0.0, 0.5 * host[0] / (0.25 + host[1] / host[0])))


@pytest.mark.parametrize("key", (3, 7, "torso"))
def test_the_direction_mode_along_the_velocity_is_the_velocity_mode(gpu, key):
    """With u = n / |n| made on the host for ONE gridpoint (a direction is fixed for a call), the direction mode's mobility is the
    velocity mode's g / s2 and its speed2 the velocity mode's.  Not bitwise: u is rounded, and g / s2 divides two rounded values --
    each side is within the mobility's bound of its exact value, s2 within its own, and u's three roundings and the host's
    normalisation move u' L u by a few ulp: the allowance is twice the mobility's bound plus speed2's plus 16 ulp, relative."""
    from toppra_amd import contact
    robot, q, qs = ec.case(key)
    model, pts = ec.robot_of(key), ec.control_points(key, "set")
    links, offsets = ec.point_set(key, "set")
    allow = 2 * ec.bound(key, "mobility") + ec.bound(key, "speed2") + 16 * EPS
    worst = 0.0
    for b, k in ((0, 0), (0, 11), (q.shape[0] - 1, q.shape[1] - 1)):
        q1, qs1 = q[b:b + 1, k:k + 1], qs[b:b + 1, k:k + 1]
        n = er.point_velocities(robot, links, offsets, q1, qs1)[0, 0]
        u = n / np.sqrt((n * n).sum(-1, keepdims=True))
        s2, g, _ = contact.effective_mass_batch(model, q1, qs1, pts)
        d2, dg, _ = contact.effective_mass_batch(model, q1, qs1, pts, directions=u)
        _, og, _ = contact.effective_mass_batch(model, q1, None, pts, directions=u)
        assert np.array_equal(og, dg)  # (without qs: the mobility alone, the same bits)
        rel = np.abs(dg - g / s2) / (g / s2)
        worst = max(worst, float(rel.max()) / allow, float((np.abs(d2 - s2) / s2).max()) / allow)
        assert np.all(rel <= allow) and np.all(np.abs(d2 - s2) <= allow * s2)
        assert np.array_equal(model.effective_mass(q1, None, pts, directions=u), 1.0 / dg)
    print("%s: direction mode against velocity mode at most %.3g of the allowance" % (key, worst))


# ---- against the siblings' kernels -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", (1, 2, 7, 32, "vee", "torso", "comb32"))
def test_the_total_energy_is_the_upper_envelope(gpu, key):
    """Cauchy-Schwarz across two kernels: speed2^2 <= mobility * energy2 (1 + both bounds), energy2 = q'' M q' from
    tpr_tree_momentum_batch.  "Both bounds": speed2 enters squared and mobility once, each with its relative bound here; energy2 is
    a sum whose committed bound (profiles/momentum_accuracy.json) is below 1e-15 of its magnitude -- 64 ulp cover it."""
    from toppra_amd import batch, contact
    _, q, qs = ec.case(key)
    model, pts = ec.robot_of(key), ec.control_points(key, "set")
    s2, g, _ = contact.effective_mass_batch(model, q, qs, pts)
    e2 = batch.momentum_batch(model, q, qs)[1][..., None]
    slack = 1.0 + 2 * ec.bound(key, "speed2") + ec.bound(key, "mobility") + 64 * EPS
    assert np.all(s2 * s2 <= g * e2 * slack)
    live = s2 > 0
    ratio = (s2 * s2)[live] / np.broadcast_to(g * e2, s2.shape)[live]
    print("%s: speed2^2 / (mobility energy2) in [%.4f, %.6f]" % (key, ratio.min(), ratio.max()))
    if key == 1:
        assert np.all(np.abs(ratio - 1.0) <= slack - 1.0)
    # at equal E_max the per-point bound is never below the total-energy bound
    E = 0.3
    xb = contact.effective_mass_bound_batch(model, q, qs, pts, np.array([2 * E, 0.0]) * np.ones((len(pts), 2)))
    total = batch.momentum_bound_batch(model, q, qs, np.array([np.inf, np.inf, 2 * E]))
    assert np.all(xb[..., 1] >= total[..., 1] * (2.0 - slack))


@pytest.mark.parametrize("d,which", ((1, "c"), (3, "b"), (7, "b"), (9, "d"), (32, "c")))
def test_speed2_is_the_control_point_kernel_s(gpu, d, which):
    """On the chains and point sets of tests/control_points_cases.py: speed2 within that family's bound of its reference, as
    chain_points_speed_batch is (the two kernels order the sums differently: not bitwise)."""
    from toppra_amd import batch, contact
    chain, q, qs, _ = cc.case(d)
    sc, pts = chain_ref.serial_chain(chain), cpc.control_points(d, which)
    ref = cpc.reference(d, which)
    with np.errstate(all="ignore"):
        mine = contact.effective_mass_batch(sc, q, qs, pts)[0]
    theirs = batch.chain_points_speed_batch(sc, q, qs, pts)
    for name, got in (("effective mass", mine), ("control points", theirs)):
        err, bound = cc.metric(got, ref["speed2"], ref["speed2_mag"]), cpc.bound(d, which, "speed2")
        print("d %d %s: %s speed2 error %.3g bound %.3g (%.2f of it)" % (d, which, name, err, bound, err / bound))
        assert err <= bound


# ---- a standstill ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", (3, "torso"))
def test_a_standstill_is_a_positive_zero_and_leaves_the_box(gpu, key):
    """q' = 0 at a gridpoint: speed2 is +0 (mobility too: the force along the velocity vanishes), the bound +inf, and the stage
    keeps the 1e8 of the box; so does a trajectory that stands still throughout."""
    from toppra_amd import algorithm, constraint, contact
    _, q, qs = ec.case(key)
    model, pts = ec.robot_of(key), ec.control_points(key, "set")
    qs = np.array(qs)
    qs[:, 7] = 0.0
    qs[:, 9] = -0.0  # (negative zeros in: the products vanish with either sign)
    s2, g, xb = contact.effective_mass_batch(model, q, qs, pts, np.array([0.4, 0.1]) * np.ones((len(pts), 2)))
    still = int(np.flatnonzero(~np.asarray(ec.case(key)[2]).any((1, 2)))[0])
    for at in ((slice(None), 7), (slice(None), 9), (still, slice(None))):
        for v in (s2[at], g[at]):
            assert not v.any() and not np.signbit(v).any()
        assert np.all(np.isposinf(xb[at][..., 1])) and not xb[at][..., 0].any()
    assert not np.isnan(xb).any()
    B, n1, d = q.shape
    grid = np.linspace(0.0, 1.0, n1)
    alim = np.tile([-50.0, 50.0], (B, d, 1))
    con = constraint.BatchContactEnergyConstraint(model, pts, 0.2, body_mass=10.0)
    low, high = algorithm.BatchTOPPRA.from_path_samples(grid, q, qs, np.zeros_like(q), None, alim, constraints=[con]).stage_boxes()
    assert np.all(high[:, 7, 1] == 1e8) and np.all(high[:, 9, 1] == 1e8) and np.all(high[still, :, 1] == 1e8)
    moving = [b for b in range(B) if b != still]
    assert np.all(high[moving, 8, 1] < 1e8) and np.all(low[..., 1] == 0.0)
    energy = model.contact_energy(q, qs, pts, 10.0)
    assert not energy[:, 7].any() and np.all(energy[moving, 8] > 0)


# ---- the constraint ----------------------------------------------------------------------------------------------------------------

def _setup(robot_kind, per_traj, seed=6, fraction=0.5):
    """(model, points, problem data, args, path samples, energy limits, body masses): the limits are ``fraction`` of each point's
    peak contact energy along the path at the speed the velocity limits allow -- so at that peak's gridpoint the bound lies below
    the velocity box and binds, and x = 0 stays feasible."""
    from toppra_amd import batch
    key = 7 if robot_kind == "chain" else "torso"
    model, pts = ec.robot_of(key), ec.control_points(key, "set")
    data, args = rs.problem(model.dof, seed=seed)
    pe = batch.path_eval_batch(*args[:3])
    body = np.linspace(2.0, 40.0, len(pts))
    body[-1] = np.inf
    xmax = sor.velocity_box(pe["qs"], args[3])[1][..., 1:]
    peak = (model.contact_energy(pe["q"], pe["qs"], pts, body) * xmax).max(1)  # [B, P]
    energy = fraction * (peak if per_traj else peak.max(0))
    return model, pts, data, args, pe, energy, body


@pytest.mark.parametrize("kind,per_traj,robot_kind", [("numpy", False, "chain"), ("torch", True, "chain"), ("numpy", True, "torso"),
                                                       ("torch", False, "torso")])
def test_the_constraint_equals_the_bound_handed_over(gpu, kind, per_traj, robot_kind):
    """Against BatchBoundConstraint(xbound) with the bound from effective_mass_bound_batch on the class's own limit: stage_boxes()
    and every pass, bit for bit; status 0; the limit tightens a box below the velocity box."""
    from toppra_amd import algorithm, constraint, contact
    model, pts, data, args, pe, energy, body = _setup(robot_kind, per_traj)
    P = len(pts)
    lim = np.stack([np.broadcast_to(2.0 * energy, (cc.B, P)), np.broadcast_to(1.0 / body, (cc.B, P))], -1)
    ours_energy = energy
    q, qs = pe["q"], pe["qs"]
    if kind == "torch":
        torch, dev = rs.torch_device()
        args = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in args)
        q, qs = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (q, qs))
        if per_traj:
            ours_energy = torch.from_numpy(energy).to(dev)
    con = constraint.BatchContactEnergyConstraint(model, pts, ours_energy, body_mass=body)
    assert np.array_equal(np.broadcast_to(con.limit, (cc.B, P, 2)), lim)
    xbound = contact.effective_mass_bound_batch(model, q, qs, pts, lim)
    assert np.array_equal(_host(xbound), er.xbound(*contact.effective_mass_batch(model, pe["q"], pe["qs"], pts)[:2], lim))
    ours = algorithm.BatchTOPPRA(*args, constraints=[con])
    theirs = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchBoundConstraint(xbound=xbound)])
    for a, b in zip(ours.stage_boxes(), theirs.stage_boxes()):
        assert np.array_equal(_host(a), _host(b))
    results = []
    for inst in (ours, theirs):
        out = rs.run_passes(inst)
        results.append({k: ({n: _host(x) for n, x in v.items()} if isinstance(v, dict) else [_host(x) for x in v] if isinstance(v, (tuple, list))
                            else _host(v)) for k, v in out.items()})
    rs.same(results[0], results[1], "constraint vs the bound handed over")
    for k in ("compute_parameterization", "compute_parameterization_sd"):
        assert np.all(results[0][k]["status"] == 0), k
    high = _host(ours.stage_boxes()[1])[..., 1]
    box = sor.velocity_box(pe["qs"], data["vlim"])[1][..., 1]
    assert np.all(high <= box) and (high < box).any(), "the limit tightens no box"
    if per_traj:  # (a limit of its own binds in every trajectory: at the peak it was taken from)
        assert all((high[b] < box[b]).any() for b in range(cc.B)), "a trajectory's limit never binds"
    # ... and a from_path_samples batch that carries q gives the same boxes
    samples = algorithm.BatchTOPPRA.from_path_samples(data["grid"], pe["q"], pe["qs"], pe["qss"], data["vlim"], data["alim"],
                                                      constraints=[constraint.BatchContactEnergyConstraint(model, pts, energy, body_mass=body)])
    assert np.array_equal(samples.stage_boxes()[1], _host(ours.stage_boxes()[1]))


@pytest.mark.parametrize("robot_kind", ("chain", "torso"))
def test_the_per_point_limit_is_never_slower_than_the_total_energy_limit(gpu, robot_kind):
    """At equal E_max, with a clamped body part (1 / m_body = 0: the comparison the Cauchy-Schwarz bound makes): every box of the
    per-point limit is at least the total-energy limit's, to the slack of the two kernels' bounds, some are larger, and the
    trajectory takes at most its duration."""
    from toppra_amd import algorithm, constraint
    model, pts, data, args, pe, _, _ = _setup(robot_kind, False)
    key = 7 if robot_kind == "chain" else "torso"
    xmax = sor.velocity_box(pe["qs"], args[3])[1][..., 1]
    # E_max: 0.3 of each trajectory's peak kinetic energy along its solution under the joint limits alone, so that the total-energy
    # limit holds every trajectory back (the velocity boxes are far above what the acceleration limits let a solution reach)
    free = algorithm.BatchTOPPRA(*args).compute_parameterization()
    assert np.all(free["status"] == 0)
    E = 0.3 * (model.kinetic_energy(pe["q"], pe["qs"]) * free["sd"] ** 2).max(-1)
    point = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchContactEnergyConstraint(model, pts, E[:, None] * np.ones(len(pts)))])
    total = algorithm.BatchTOPPRA(*args, constraints=[constraint.BatchMomentumConstraint(model, energy=E)])
    hp, ht = point.stage_boxes()[1][..., 1], total.stage_boxes()[1][..., 1]
    slack = 2 * ec.bound(key, "speed2") + ec.bound(key, "mobility") + 64 * EPS
    assert np.all(hp >= ht * (1.0 - slack)) and (hp > ht).any() and (ht < xmax).any()
    durations = []
    for inst in (point, total):
        out = inst.compute_parameterization()
        assert np.all(out["status"] == 0)
        sd = np.maximum(out["sd"], 1e-12)
        ds = np.diff(np.broadcast_to(data["grid"], sd.shape), axis=-1)
        durations.append((2.0 * ds / (sd[:, 1:] + sd[:, :-1])).sum(-1))
    print("%s: duration under the per-point limit / under the total-energy limit: %s" % (robot_kind, np.round(durations[0] / durations[1], 4)))
    assert np.all(durations[0] <= durations[1] * (1.0 + 1e-9)) and (durations[0] < durations[1]).any()


def test_beside_a_torque_and_a_momentum_limit(gpu):
    """[torque, momentum, contact energy] on one 7-dof arm: the boxes are those of the two first-order constraints alone, the dense
    rows those of the list without the contact limit; every pass runs and every trajectory is feasible."""
    from toppra_amd import algorithm, constraint
    model, pts, data, args, pe, energy, body = _setup("chain", False, seed=8)
    d = model.dof
    taumax = np.abs(model.torque_terms(pe["q"], pe["qs"], pe["qss"])[0]).max() + 20.0
    xmax = sor.velocity_box(pe["qs"], data["vlim"])[1][..., 1]
    moment = constraint.BatchMomentumConstraint(model, energy=0.9 * float((model.kinetic_energy(pe["q"], pe["qs"]) * xmax).max()))
    contact_limit = constraint.BatchContactEnergyConstraint(model, pts, energy, body_mass=body)
    torque = constraint.BatchJointTorqueConstraint(model, np.tile([-taumax, taumax], (d, 1)), np.zeros(d))
    full = algorithm.BatchTOPPRA(*args, constraints=[torque, moment, contact_limit])
    out = rs.run_passes(full)
    rs.passes_ran(out)
    first = algorithm.BatchTOPPRA(*args, constraints=[moment, contact_limit]).stage_boxes()
    assert np.array_equal(out["rows"][3], first[0]) and np.array_equal(out["rows"][4], first[1])
    without = algorithm.BatchTOPPRA(*args, constraints=[torque, moment]).dense_rows()
    for k in range(3):
        assert np.array_equal(out["rows"][k], without[k])
    assert (out["rows"][4][..., 1] < without[4][..., 1]).any(), "the contact limit tightens no box beside the momentum limit"
    alone = algorithm.BatchTOPPRA(*args, constraints=[contact_limit]).stage_boxes()[1]
    assert np.all(out["rows"][4][..., 1] <= alone[..., 1])


# ---- the reference's fixtures ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FIXTURES)
def test_against_the_reference_s_fixtures(gpu, name):
    """The kernel's outputs within the stored accuracy bound (relative: a quantity's magnitude is its own value); high[..., 1]
    within that bound composed through the divisions; every other box entry, and the return codes, equal; sd within the stored
    end-to-end tolerance (tools/make_effective_mass_golden.py)."""
    from toppra_amd import constraint, contact
    from toppra_amd.chain import ControlPoints
    fx = golden(name)
    model = tree_ref.kinematic_tree(rs.fixture_tree(fx))
    pts = ControlPoints([int(k) for k in fx["point_links"]], fx["point_offsets"])
    q, qs, _ = sor.path_samples(fx["coef"], fx["breaks"], fx["grid"])
    s2, g, xb = contact.effective_mass_batch(model, q, qs, pts, fx["limit"])
    rs.fixture_accuracy(name, fx, {"speed2": s2, "mobility": g}, {k: fx[k + "_mag"] for k in ("speed2", "mobility")})
    con = constraint.BatchContactEnergyConstraint(model, pts, fx["energy"], body_mass=fx["body_mass"])
    assert np.array_equal(con.limit, fx["limit"])  # (the class doubles and inverts as the generator did)
    inst = rs.fixture_instance(fx, con)
    low, high = inst.stage_boxes()
    tol = er.xbound_tolerance(fx["speed2"], fx["mobility"], fx["limit"], *fx["acc_bound"])
    assert np.array_equal(low, fx["low"]) and np.array_equal(high[..., 0], fx["high"][..., 0])
    off = np.abs(high[..., 1] - fx["high"][..., 1])
    print("ACCURACY fixture %s high error_over_allowance %.3g" % (name, float(np.max(off[tol > 0] / tol[tol > 0]))))
    assert np.all(off <= tol)
    assert (fx["high"][..., 1] == fx["xbound"][..., 1]).sum(-1).min() >= (q.shape[1] + 3) // 4  # the bound, not the velocity box
    rs.fixture_sd(name, fx, inst)

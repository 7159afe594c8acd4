"""The one recipe of the rigid-body fixtures: what tools/make_<family>_golden.py share.  Each of those commands runs the REAL
reference (hungpham2511/toppra) on two small stored problems and writes tests/golden/<fixture>.npz and
profiles/<family>_accuracy.json; a family file holds its robots and what is attached to them, its quantities, its choice of
limits and the constraint it hands to the reference.  The steps, each written once here:

 1. reference(): load the reference (built into oracle/_ref on demand) and map its return codes.  Loading happens on first use,
    never on import: importing this module, or a helper from it, runs nothing.
 2. draw_paths(): B paths through 5 waypoints and their joint limits, the reference's splines fitted and sampled on N + 1
    gridpoints.  The ORDER of the draws from the fixture's default_rng(seed) is part of the data: way, vmax, amax here, then the
    family's own draws (friction, jitter of the limits), then nothing else.  Scaling the waypoints draws nothing.
 3. gridpoint_terms(): w0 = f(q, 0, 0), wa = f(q, 0, q'), wb = f(q, q', q''), one gridpoint per call as the reference calls f.
 4. free_solutions(): the reference WITHOUT the family's constraint, [velocity, acceleration] through TOPPRA("seidel").
 5. The family chooses its limits from those solutions, in physical units.
 6. solve_reference(): [velocity, acceleration, the family's constraint] one trajectory at a time; collected are the dense rows
    after the acceleration block (or, for a constraint that only bounds x, the reference wrapper's own boxes), low, high, K, sd,
    u and the return codes.
 7. Every trajectory must be feasible (status 0), and the constraint active -- the reference's sd differs from its sd without
    it (assert_active): both asserted.
 8. yardstick(): acc_yardstick = the error of the float64 numpy reference against np.longdouble on the fixture's own terms, in
    the metric of tests/chain_cases.py; acc_bound = BOUND_FACTOR (16) x that.
 9. sd_tolerance(): the problem restated under oracle/ (tests/second_order_ref.py's rows, oracle.solve_dense_batch) and solved
    with every disturbed term moved by noise of the size of the accuracy bound -- uniform in +- its acc_bound x its all-absolute
    magnitude, over 20 seeds (1000 to 1019); sd_tol = 4 x the largest change of sd.  The disturbance is what the accuracy
    bound ALLOWS, not what a kernel shows, so sd_tol errs on the loose side.
10. save(): the .npz, data only, under 200 KB.
11. write_profile(): profiles/<family>_accuracy.json, keeping the `measured` entry a GPU run has written there.

No test and nothing run on the GPU imports this module or the family files.
"""
import functools
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

from oracle import oracle as orc, ref_loader  # noqa: E402
from tests import chain_cases, second_order_ref as sor, tree_cases, tree_ref  # noqa: E402

CHAIN_KEYS = ("joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity", "tool")
TREE_KEYS = ("parent", "joint_type", "axis", "rot", "trans", "mass", "com", "inertia", "gravity")
ROBOT_KEYS = TREE_KEYS[1:] + ("parent",)
SOLVED = ("rows_a", "rows_b", "rows_c", "low", "high", "K", "sd", "u", "status")
MAX_ROWS = 122  # (of a stage: what the dense-row kernels hold)


@functools.lru_cache(None)
def reference():
    """The reference's modules: .ta (toppra), .algo, .constraint, and .status, its return codes as the library's 0 / 1 / 2."""
    ta = ref_loader.load()
    if ta is None:
        raise SystemExit("reference not available")
    import toppra.algorithm as algo
    import toppra.constraint as constraint
    from toppra.algorithm.algorithm import ParameterizationReturnCode as RC
    return types.SimpleNamespace(ta=ta, algo=algo, constraint=constraint, status={RC.Ok: 0, RC.FailUncontrollable: 1, RC.ErrUnknown: 2})


def scara():
    """Two vertical revolute joints, a vertical prismatic joint, a vertical wrist: the last link keeps its z axis up."""
    d = 4
    eye = np.tile(np.eye(3), (d, 1, 1))
    return {"joint_type": np.array([0, 0, 1, 0], dtype=np.int32), "axis": np.tile([0.0, 0.0, 1.0], (d, 1)), "rot": eye,
            "trans": np.array([[0.0, 0.0, 0.4], [0.35, 0.0, 0.0], [0.3, 0.0, 0.0], [0.0, 0.0, -0.1]]),
            "mass": np.array([6.0, 4.0, 1.5, 0.5]), "com": np.array([[0.17, 0.0, 0.0], [0.15, 0.0, 0.0], [0.0, 0.0, -0.1], [0.0, 0.0, 0.0]]),
            "inertia": np.array([[0.02, 0.08, 0.08, 0, 0, 0], [0.01, 0.04, 0.04, 0, 0, 0], [0.005, 0.005, 0.001, 0, 0, 0],
                                 [0.0005, 0.0005, 0.0005, 0, 0, 0]], dtype=np.float64),
            "gravity": np.array([0.0, 0.0, -9.81]), "tool": np.array([0.05, 0.0, 0.02])}


SCARA_WAY = np.array([1.0, 1.0, 0.1, 1.0])  # (the scale of the SCARA's waypoints: the lift moves +- 15 cm)


def as_tree(chain):
    """A serial chain without its tool point, with the parent table of a tree."""
    tree = {k: v for k, v in chain.items() if k != "tool"}
    tree["parent"] = np.arange(len(tree["mass"]), dtype=np.int32) - 1
    return tree


def torso(gravity=None):
    """tests/tree_cases.py's torso shape -- a torso joint that carries two 7-dof arms -- with tree_ref.random_tree's links."""
    tree = tree_ref.random_tree(tree_cases.SHAPES["torso"], seed=77, gravity=True, massless=None)
    if gravity is not None:
        tree["gravity"] = np.array(gravity)
    return tree


def tilted(angle):
    """The rotation by ``angle`` about y: a frame that is not quite level."""
    return np.array([[np.cos(angle), 0.0, np.sin(angle)], [0.0, 1.0, 0.0], [-np.sin(angle), 0.0, np.cos(angle)]])


def signed_identity(firsts, width):
    """F [6 * len(firsts), width]: [I; -I] on the three components that begin at each of ``firsts``, in order."""
    F = np.zeros((6 * len(firsts), width))
    for k, first in enumerate(firsts):
        F[6 * k:6 * k + 3, first:first + 3], F[6 * k + 3:6 * k + 6, first:first + 3] = np.eye(3), -np.eye(3)
    return F


def surface_contact(B, mu, half):
    """F, g [B, 16] and what to store of a flat contact patch: the constraints' own surface_contact rows (no slip, no tip, no spin)."""
    from toppra_amd.constraint import BatchToolWrenchConstraint
    F, g1 = BatchToolWrenchConstraint.surface_contact_rows(mu, half)
    return F, np.broadcast_to(g1, (B, F.shape[0])).copy(), {"mu": np.array(mu), "half_extents": np.array(half)}


def draw_paths(rng, B, d, N, scale=1.0):
    """Step 2.  ``scale`` (a number or [d]) multiplies the waypoints."""
    knots = np.linspace(0, 1, 5)
    p = types.SimpleNamespace(B=B, d=d, N=N, knots=knots, grid=np.linspace(0, 1, N + 1))
    p.way = rng.uniform(-1.5, 1.5, (B, 5, d)) * scale
    vmax, amax = 2.0 + 2.0 * rng.random((B, d)), 6.0 + 4.0 * rng.random((B, d))
    p.vlim, p.alim = np.stack([-vmax, vmax], -1), np.stack([-amax, amax], -1)
    p.paths = [reference().ta.SplineInterpolator(knots, p.way[b]) for b in range(B)]
    p.q, p.qs, p.qss = (np.stack([path(p.grid, k) for path in p.paths]) for k in (0, 1, 2))
    p.coef = np.stack([np.asarray(path.cspl.c) for path in p.paths])
    p.breaks = np.asarray(p.paths[0].cspl.x)
    return p


def gridpoint_terms(f, p):
    """Step 3: {"w0", "wa", "wb"}, each [B, N+1, m]."""
    zero = np.zeros(p.d)
    return {"w0": np.array([[f(q_, zero, zero) for q_ in p.q[b]] for b in range(p.B)]),
            "wa": np.array([[f(q_, zero, s_) for q_, s_ in zip(p.q[b], p.qs[b])] for b in range(p.B)]),
            "wb": np.array([[f(q_, s_, ss_) for q_, s_, ss_ in zip(p.q[b], p.qs[b], p.qss[b])] for b in range(p.B)])}


def base_constraints(p, b, accel_scheme=1):
    c = reference().constraint
    return [c.JointVelocityConstraint(p.vlim[b]),
            c.JointAccelerationConstraint(p.alim[b], discretization_scheme=c.DiscretizationType(accel_scheme))]


def free_solutions(p):
    """Step 4: [(u, sd)] of the B trajectories."""
    free = []
    for b in range(p.B):
        inst = reference().algo.TOPPRA(base_constraints(p, b), p.paths[b], gridpoints=p.grid, solver_wrapper="seidel")
        sdd, sd, _ = inst.compute_parameterization(0, 0)
        assert sd is not None
        free.append((sdd, sd))
    return free


def along(terms, free, b, static=False):
    """[N, m]: the dynamic part (w - w0) of a quantity along trajectory b's solution without the constraint; with ``static``, w."""
    (sdd, sd), w0 = free[b], terms["w0"][b, :-1]
    return static * w0 + (terms["wa"][b, :-1] - w0) * sdd[:, None] + (terms["wb"][b, :-1] - w0) * (sd[:-1] ** 2)[:, None]


def assert_active(name, sds, free):
    for b, sd in enumerate(sds):
        assert not np.array_equal(sd, free[b][1]), "%s: the constraint is not active in trajectory %d" % (name, b)
        print("%s trajectory %d: largest sd %.4f, without the constraint %.4f" % (name, b, sd.max(), free[b][1].max()))


def reference_boxes(cons, path, grid):
    """low_arr, high_arr [N+1, 2] of the reference's wrapper on the first-order constraints of ``cons``."""
    from toppra.solverwrapper.cy_seidel_solverwrapper import seidelWrapper
    first = [c for c in cons if c.compute_constraint_params(path, grid)[0] is None]
    w = seidelWrapper(first, path, grid)
    nan = float("nan")
    low = np.array([w.solve_stagewise_optim(i, None, np.array([1.0, 1.0]), nan, nan, nan, nan) for i in range(len(grid))])
    high = np.array([w.solve_stagewise_optim(i, None, np.array([-1.0, -1.0]), nan, nan, nan, nan) for i in range(len(grid))])
    return low, high


def solve_reference(name, p, third, accel_scheme=1, free=None, rows=True):
    """Steps 6 and 7.  ``third(b)`` makes the family's constraint for trajectory b; with ``free`` (step 4) the constraint must be
    active.  Returns the stacked record, and the constraint lists."""
    from toppra_amd.solverwrapper import dense_rows
    ref, out, lists = reference(), {k: [] for k in SOLVED if rows or not k.startswith("rows_")}, []
    first = 2 + (4 if accel_scheme else 2) * p.d  # (the x_next pair, the acceleration block)
    for b in range(p.B):
        cons = base_constraints(p, b, accel_scheme) + [third(b)]
        inst = ref.algo.TOPPRA(cons, p.paths[b], gridpoints=p.grid, solver_wrapper="seidel")
        sdd, sd, _, K = inst.compute_parameterization(0, 0, return_data=True)
        st = ref.status[inst.problem_data.return_code]
        assert st == 0 and sd is not None, "%s: trajectory %d is not feasible in the reference (status %d)" % (name, b, st)
        if rows:
            dense = dense_rows(cons, p.paths[b], p.grid)
            assert dense["a"].shape[1] <= MAX_ROWS, dense["a"].shape
            for k in "abc":
                out["rows_" + k].append(dense[k][:, first:])
            low, high = dense["low"], dense["high"]
        else:
            low, high = reference_boxes(cons, p.paths[b], p.grid)
        for k, v in (("low", low), ("high", high), ("K", K), ("sd", sd), ("u", sdd), ("status", st)):
            out[k].append(v)
        lists.append(cons)
    if free is not None:
        assert_active(name, out["sd"], free)
    rec = {k: np.stack(v) for k, v in out.items()}
    rec["status"] = rec["status"].astype(np.int32)
    return rec, lists


def yardstick(ref, names, terms):
    """Step 8.  ``ref`` is the cases module's reference_of(...) on the fixture's inputs; its batched values must be the
    per-gridpoint ones.  Returns acc_yardstick, acc_bound [len(names)]."""
    assert all(np.array_equal(ref[k].reshape(terms[k].shape), terms[k]) for k in names), "batched reference differs from per-point calls"
    yard = np.array([ref["yardstick"][k] for k in names])
    assert np.all(yard > 0)
    return yard, chain_cases.BOUND_FACTOR * yard


def restated_rows(p, block, accel_scheme=1):
    """The restatement of a dense-row problem: solve(terms) with tests/second_order_ref.py's rows for ``block`` and the terms."""
    def solve(terms):
        rows = sor.dense_problem(p.coef, p.breaks, p.grid, p.vlim, p.alim, bool(accel_scheme), [dict(block, **terms)])
        return orc.solve_dense_batch(*(rows[k] for k in ("a", "b", "c", "low", "high", "deltas")))
    return solve


def sd_tolerance(name, rec, solve, terms, names, ref, bound, exact):
    """Step 9: sd_tol.  ``solve(terms)`` is the restatement; the terms in ``names`` are disturbed, the others (an exact zero) not.

    ``exact`` says how the restatement must compare with the reference before anything is disturbed.  True: sd equal in bits --
    where F is None or a signed identity, or the constraint only bounds x, both do the same arithmetic.  False: where F is dense
    the reference forms F a, F b, F c with numpy's dot, whose summation order is the BLAS's, while the restatement and the kernels
    sum a row in index order; the rows agree to rounding, not in bits, and so does sd, and the gap must vanish in sd_tol: it may
    not exceed what the disturbance moves sd by."""
    base = solve(terms)
    assert np.array_equal(base["status"], rec["status"]), "the restatement's return codes differ from the reference's"
    gap, worst = float(np.max(np.abs(base["sd"] - rec["sd"]))), 0.0
    for s in range(20):
        nrng = np.random.default_rng(1000 + s)
        noisy = {k: terms[k] + bd * ref[k + "_mag"].reshape(terms[k].shape) * nrng.uniform(-1.0, 1.0, terms[k].shape)
                 for bd, k in zip(bound, names)}
        got = solve(dict(terms, **noisy))
        assert np.array_equal(got["status"], rec["status"])
        worst = max(worst, float(np.max(np.abs(got["sd"] - base["sd"]))))
    print("%s: restatement vs reference sd %.3g, sd_tol %.3g" % (name, gap, 4.0 * worst))
    assert worst > 0
    if exact:
        assert np.array_equal(base["sd"], rec["sd"]), "%s: the restatement differs from the reference" % name
    assert gap <= worst, "%s: the restatement differs from the reference by more than the disturbance moves it" % name
    return 4.0 * worst


def save(name, rec):
    """Step 10.  The order of ``rec`` is the order of the archive's members."""
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 200 * 1024, os.path.getsize(path)
    return "%.0f KB" % (os.path.getsize(path) / 1024)


def finish(name, p, rec, solve, terms, names, ref, exact, robot, keys, attached, own, extra=(), **profile):
    """Steps 8 to 10 for a solved fixture ``rec``; returns its entry of the profile.  Stored, in this order: the solved record,
    the robot's ``keys``, ``attached``, the paths and joint limits, ``own``, the two tolerances, ``extra``."""
    yard, bound = yardstick(ref, names, terms)
    sd_tol = sd_tolerance(name, rec, solve, terms, names, ref, bound, exact)
    rec = dict(rec, **{k: np.asarray(robot[k]) for k in keys})
    rec.update(attached)
    rec.update(knots=p.knots, way=p.way, coef=p.coef, breaks=p.breaks, grid=p.grid, vlim=p.vlim, alim=p.alim)
    rec.update(own)
    rec.update(acc_yardstick=yard, acc_bound=bound, sd_tol=np.array(sd_tol))
    rec.update(extra)
    size = save(name, rec)
    print(name, "rows", rec["rows_a"].shape if "rows_a" in rec else None, "status", np.bincount(rec["status"], minlength=3),
          "acc_bound", bound, "sd_tol %.3g" % sd_tol, size)
    return dict({"yardstick": dict(zip(names, yard.tolist())), "bound": dict(zip(names, bound.tolist())), "sd_tol": sd_tol}, **profile)


def torque_fixture(name, rng, p, robot, keys, inv_dyn, ref, torque, torque_scheme, accel_scheme, per_traj_limits, own=()):
    """A fixture of a torque family, chain or tree: friction and then the limits drawn (step 5: the torque of standing still
    anywhere on the paths, and headroom to move, so every trajectory stays feasible), ``torque(limits, friction)`` -- the
    reference's JointTorqueConstraint as the family makes it -- solved.  Stored: taulim ([d, 2] shared or [B, d, 2]), fric, w0,
    wa, wb, torque_scheme, ``own``."""
    fric = 0.05 * rng.random(p.d)
    terms = gridpoint_terms(inv_dyn, p)
    taumax = 1.2 * np.abs(terms["w0"]).max(axis=(0, 1)) + 1.0 + rng.random((p.B, p.d) if per_traj_limits else p.d)
    taulim = np.stack([-taumax, taumax], -1)
    rec, lists = solve_reference(name, p, lambda b: torque(taulim[b] if per_traj_limits else taulim, fric), accel_scheme)
    if torque_scheme == 0:  # the constraint's own parameters are the numpy values through the reference's expressions
        for b, cons in enumerate(lists):
            a, bb = cons[2].compute_constraint_params(p.paths[b], p.grid)[:2]
            assert np.array_equal(a, terms["wa"][b] - terms["w0"][b]) and np.array_equal(bb, terms["wb"][b] - terms["w0"][b])
    block = {"F": None, "g": np.concatenate((taulim[..., 1], -taulim[..., 0]), -1), "friction": fric, "interpolation": bool(torque_scheme)}
    return finish(name, p, rec, restated_rows(p, block, accel_scheme), terms, ("w0", "wa", "wb"), ref, True, robot, keys, {},
                  dict(taulim=taulim, fric=fric, **terms, torque_scheme=np.array(torque_scheme), **dict(own)))


def second_order_fixture(name, p, free, third, F, g, scheme, terms, names, ref, exact, robot, keys, attached=(), own=(), extra=(), shape=None):
    """A fixture of a family whose constraint is F w <= g on a quantity w ([B, m] or one [m] of limits): ``third(b)`` -- the
    reference's SecondOrderConstraint as the family makes it -- solved, and active against ``free``.  Stored: ``own``, F, g, the
    terms in ``names`` (in ``shape`` where they have one of their own), scheme."""
    block = {"F": F, "g": np.broadcast_to(g, (p.B, F.shape[0])), "friction": None, "interpolation": bool(scheme)}
    assert np.all(np.einsum("mk,bnk->bnm", F, terms["w0"]) < block["g"][:, None, :]), "%s: standing still violates the limits" % name
    rec, _ = solve_reference(name, p, third, free=free)
    stored = {k: terms[k].reshape(shape or terms[k].shape) for k in names}
    return finish(name, p, rec, restated_rows(p, block), terms, names, ref, exact, robot, keys, dict(attached),
                  dict(own, F=F, g=g, **stored, scheme=np.array(scheme)), extra)


def write_profile(family, yardstick_of, cases, fixtures, metric_more="", **more):
    """Step 11.  What the kernels were measured to use (`measured`) is written by the GPU run, not here: it is kept."""
    path = os.path.join(ROOT, "profiles", family + "_accuracy.json")
    doc = dict({"metric": "|got - ref| / (|ref| with every product and sum in absolute value); yardstick = %s against np.longdouble "
                          "on the same inputs; bound = %g x yardstick%s" % (yardstick_of, chain_cases.BOUND_FACTOR, metric_more),
                "cases": cases, "fixtures": fixtures}, **more)
    if os.path.exists(path):
        with open(path) as fh:
            measured = json.load(fh).get("measured")
        if measured is not None:
            doc["measured"] = measured
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")

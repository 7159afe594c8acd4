"""What the GPU parity tests of the solver share (tests/test_gpu_parity.py, _fullsize, _pair, _instantiations, _scan_bookkeeping,
_slim_blocks, _extreme_limits, _robust_shapes with tests/robust_shapes.py): the bit-for-bit comparison of a result dict, the oracle's
flags for a constraint set, the unpacking of a problem, the kernel-tracer harness with its name matcher, the problem recipes more
than one module draws from -- the irregular batch, per-trajectory breakpoints and grids, boundary velocities on the 2^-10 lattice,
the limits at the edge of the number range that tests/test_oracle_vs_reference.py pins to the reference's stored outputs -- and the
batch sizes at which the library changes kernels.  A plain module: the tests import it, not each other; nothing here needs a GPU
until it is called."""
import contextlib
import csv
import functools
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The batch sizes of the automatic choice, restated from toppra_amd/csrc/tpr_kernels.hip -- a change there must be copied here; the
# values are otherwise nowhere in the tests.  pick_variant: family 3 (the certified lane kernels) solves from cert_auto_from(d)
# trajectories -- 9216 up to 8 dof, CERT_AUTO_FROM[d] at 9 .. 15 dof -- and family 5 (two trajectories per wave) serves
# kPairAutoMinBatch = 2560 .. 9215 trajectories up to 7 dof; tpr_solve_desired_duration_batch fuses TOPPRAsd from cert_auto_from(d)
# as well; tpr_feasible_sets_batch hands the feasible sets to family 3 from 8192 trajectories up to 8 dof and from cert_auto_from(d)
# above.  include/toppra_hip.h says the same in the paragraphs on tpr_problem.variant of tpr_solve_batch ("from 9216 trajectories
# (9..15 dof: 14336 .. 36864)") and of tpr_feasible_sets_batch ("from 8192 trajectories up to 8 dof, 14336 .. 36864 at 9 .. 15 dof").
CERT_SOLVE_FROM, CERT_FEASIBLE_FROM, PAIR_FROM = 9216, 8192, 2560
CERT_AUTO_FROM = {9: 14336, 10: 14336, 11: 15360, 12: 17408, 13: 22528, 14: 27648, 15: 36864}


# --------------------------------------------------------------------------------------------------------------------------
# comparison, flags, problems

def same(got, want, keys, what, kinds=None):
    """THE bit-for-bit comparison of two result dicts: equal shapes, `status` exact whenever `want` has one, every key of `keys`
    with np.array_equal(..., equal_nan=True) -- NaNs must coincide.  The AssertionError carries `what`, the key, how many
    trajectories (rows of the leading axis) differ and the first eight of them; with `kinds` [B], their kinds as well."""
    for k in (("status",) if "status" in want else ()) + tuple(k for k in keys if k != "status"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, "shape", g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=(k != "status")):
            differs = ~((g == w) | ((g != g) & (w != w) & (k != "status"))).reshape(g.shape[0] if g.ndim else 1, -1).all(axis=1)
            where = np.flatnonzero(differs)
            raise AssertionError((what, k, int(differs.sum()), where[:8].tolist(), None if kinds is None else sorted(set(np.asarray(kinds)[where]))))


def same_array(got, want, what, kinds=None):
    """`same` for one bare array."""
    same({"x": got}, {"x": want}, ("x",), what, kinds)


def oracle_flags(oracle, vel, interp, acc=True):
    """The oracle's `flags` for a constraint set and a discretisation -- the one place where the mapping lives.  Callers pass
    `vlim is not None` for `vel`.  (True, True) is oracle.DEFAULT_FLAGS, (True, False) is DEFAULT_FLAGS & ~FLAG_INTERP."""
    return (oracle.FLAG_VEL if vel else 0) | (oracle.FLAG_ACC if acc else 0) | (oracle.FLAG_INTERP if interp else 0)


def problem(data, vel=True):
    """(coef, breaks, grid, vlim or None, alim) of a problem dict."""
    return (data["coef"], data["breaks"], data["grid"], data["vlim"] if vel else None, data["alim"])


# --------------------------------------------------------------------------------------------------------------------------
# which kernel ran

@contextlib.contextmanager
def traced(child, *argv):
    """Runs the source string `child` with the arguments `argv` in a fresh child process under the kernel tracer (kernel trace and
    statistics, no counters) and yields (calls, tmp): the tracer's [(kernel name, dispatches)] and the temporary directory, which
    lives as long as the block -- "{tmp}" in an argument stands for it, so that the child can leave files there for the caller.
    The child prints "traced child done" as its last act."""
    rp = shutil.which("rocprofv3")
    assert rp, "rocprofv3 is not on PATH: the dispatch of the automatic choice cannot be traced (GPU tests do not skip here)"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    with tempfile.TemporaryDirectory(prefix="tpr_trace_") as tmp:
        cmd = ["timeout", "-k", "10", "240", rp, "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--output-format", "csv", "--",
               sys.executable, "-c", child] + [a.replace("{tmp}", tmp) for a in argv]
        run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert run.returncode == 0, (run.returncode, run.stdout[-3000:])
        assert "traced child done" in run.stdout, run.stdout[-3000:]
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats*.csv"), recursive=True)
        assert stats, ([os.path.join(r, f) for r, _, fs in os.walk(tmp) for f in fs], run.stdout[-2000:])
        calls = []
        for path in stats:
            with open(path, newline="") as fh:
                calls += [(r["Name"], int(r["Calls"])) for r in csv.DictReader(fh)]
        yield calls, tmp


def dispatches(calls, kernel, d=None):
    """Dispatches of `kernel` in the tracer's (name, calls) statistics: every kernel whose name holds `kernel`, or -- with d --
    tpr::<kernel><d, ...> alone (demangled names, or ...<kernel>ILi<d>E...).  The dof is the FIRST template argument of every
    kernel asked about with d (cert_solve_kernel, cert_feasible_kernel, group_solve_kernel, group_feasible_kernel,
    group_sd_forward_kernel, group_robust_kernel): the match relies on that."""
    return sum(c for n, c in calls if (kernel in n if d is None else (kernel + "<%d," % d in n or kernel + "ILi%dE" % d in n)))


# --------------------------------------------------------------------------------------------------------------------------
# problem recipes

def irregular_batch(B, d, N, n_waypoints, seed):
    """The irregular batch: non-uniform knots and grid, standing joints (8 %), asymmetric velocity limits with a positive lower one
    on 1 % of the joints, asymmetric acceleration limits, boundary velocities on 40 % of the trajectories at either end."""
    from toppra_amd import batch
    rng = np.random.default_rng(seed)
    nw = n_waypoints
    knots = np.concatenate([[0.0], np.sort(rng.random(nw - 2)) * 0.9 + 0.05, [1.0]])
    way = rng.standard_normal((B, nw, d))
    still = rng.random((B, d)) < 0.08
    way = np.where(still[:, None, :], way[:, :1, :], way)
    coef, breaks = batch.spline_coefficients(knots, way)
    grid = 0.6 * np.concatenate([[0.0], np.sort(rng.random(N - 1)), [1.0]]) + 0.4 * np.linspace(0, 1, N + 1)
    vhi = 5 + 25 * rng.random((B, d)); vlo = -(5 + 25 * rng.random((B, d)))
    vlo = np.where(rng.random((B, d)) < 0.01, 0.05 * rng.random((B, d)), vlo)
    ahi = 5 + 10 * rng.random((B, d)); alo = -(5 + 10 * rng.random((B, d)))
    sd0 = np.where(rng.random(B) < 0.4, 0.3 * rng.random(B), 0.0)
    sd1 = np.where(rng.random(B) < 0.4, 0.3 * rng.random(B), 0.0)
    return {"coef": coef, "breaks": breaks, "grid": grid, "vlim": np.ascontiguousarray(np.stack([vlo, vhi], -1)),
            "alim": np.ascontiguousarray(np.stack([alo, ahi], -1)), "sd0": sd0, "sd1": sd1, "knots": knots, "waypoints": way}


def own_breakpoints(data, seed):
    """Per-trajectory breakpoints [B][nseg+1] for the paths of `data`: every trajectory's interior knots moved by up to a quarter of
    the narrowest knot interval, and its spline fitted through the same waypoints on ITS knots (scipy's CubicSpline, one by one:
    batch.spline_coefficients fits shared knots only).  -> (coef [B][4][nseg][d], breaks [B][nseg+1])"""
    from scipy.interpolate import CubicSpline
    knots, way = data["knots"], data["waypoints"]
    B, nw, _ = way.shape
    rng = np.random.default_rng(seed)
    own = np.repeat(knots[None], B, axis=0)
    own[:, 1:-1] += rng.uniform(-0.25, 0.25, size=(B, nw - 2)) * np.diff(knots).min()
    coef = np.stack([CubicSpline(own[b], way[b]).c for b in range(B)])
    return np.ascontiguousarray(coef), np.ascontiguousarray(own)


def per_trajectory_grid(rng, B, N):
    """A non-uniform grid per trajectory [B][N+1], halfway between sorted random gridpoints and the uniform grid: one draw of
    (B, N - 1) from `rng`, the caller's generator at the caller's point in its stream (none for N = 1)."""
    inner = np.sort(rng.random((B, N - 1)), axis=1) * 0.8 + 0.1 if N > 1 else np.zeros((B, 0))
    return 0.5 * np.concatenate([np.zeros((B, 1)), inner, np.ones((B, 1))], axis=1) + 0.5 * np.linspace(0, 1, N + 1)[None, :]


def lattice_boundary_velocities(rng, B, start, end):
    """(sd_start, sd_end) [B]: non-zero on 30 % of the trajectories each, up to `start` / `end`, rounded to the 2^-10 lattice (their
    squares are exact).  Four draws of B from `rng`: the start's mask and values, then the end's."""
    sd0 = np.where(rng.random(B) < 0.3, np.round(start * rng.random(B) * 1024) / 1024, 0.0)
    sd1 = np.where(rng.random(B) < 0.3, np.round(end * rng.random(B) * 1024) / 1024, 0.0)
    return sd0, sd1


def instantiation_problem(B, d, N, seed, per_traj_grid):
    """make_synthetic_batch(B, d, N, seed) and, from one generator of the same seed, a grid per trajectory (where asked for: the grid
    is then read from global memory instead of the block's LDS copy) and boundary velocities up to 0.1 / 0.2 on the lattice.
    -> (data, grid, sd_start, sd_end)"""
    from toppra_amd import batch
    data = batch.make_synthetic_batch(B, d, N, seed=seed)
    rng = np.random.default_rng(seed)
    grid = per_trajectory_grid(rng, B, N) if per_traj_grid else data["grid"]
    return (data, grid) + lattice_boundary_velocities(rng, B, 0.1, 0.2)


def near_parallel_family(B, d, N, seed):
    """Adversarial for the certificates: one joint a copy of another, scaled or tilted by 1e-14 .. 1e-6, so that two non-twin rows
    are parallel to that accuracy at every gridpoint.  -> (coef, breaks, grid, vlim, alim, None, sd_end)"""
    from toppra_amd import batch
    rng = np.random.default_rng(900 + seed)
    way = rng.standard_normal((B, 5, d))
    eps = 10.0 ** rng.uniform(-14, -6, size=B)
    scale = rng.choice([1.0, -1.0, 0.5, 2.0, 3.0], size=B)
    src, dst = rng.integers(0, d, size=B), rng.integers(0, d, size=B)
    dst = np.where(dst == src, (src + 1) % d, dst)
    rows = np.arange(B)
    way[rows, :, dst] = way[rows, :, src] * (scale * (1 + eps))[:, None]
    twist = rng.random(B) < 0.5
    way[rows[twist], :, dst[twist]] += eps[twist, None] * rng.standard_normal((twist.sum(), 5))
    coef, breaks = batch.spline_coefficients(np.linspace(0, 1, 5), way)
    vmax = 10 + 20 * rng.random((B, d))
    amax = 10 + 2 * rng.random((B, d))
    amax[rows, dst] = amax[rows, src] * np.abs(scale) * (1 + 0.02 * rng.standard_normal(B))
    vmax[rows, dst] = vmax[rows, src] * np.abs(scale) * (1 + 0.02 * rng.standard_normal(B))
    vlim = np.ascontiguousarray(np.stack([-vmax, vmax], -1))
    alim = np.ascontiguousarray(np.stack([-amax, amax], -1))
    sd1 = np.where(rng.random(B) < 0.3, 0.2 * rng.random(B), 0.0)
    return coef, breaks, np.linspace(0, 1, N + 1), vlim, alim, None, sd1


# --------------------------------------------------------------------------------------------------------------------------
# limits at the edge of the number range (pinned: tests/test_oracle_vs_reference.py::test_extreme_limits_match_reference holds the
# oracle to what the reference computed on extreme_limit_problems, tests/golden/oracle_vs_reference_extreme.npz -- a change of any
# draw below is a change of that fixture)

EXTREME_KINDS = ("vinf", "ainf", "ainf_one", "vhuge", "ahuge", "vsub", "vtiny", "vneg", "inverted", "still", "shifted", "mix")
EXTREME_CASES = [(1, 30, 1), (3, 40, 2), (7, 60, 3), (12, 36, 4)]
EXTREME_TRIALS = 3
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN_NORMAL = float(np.finfo(np.float32).tiny)  # 2^-126: fp32 values below it are subnormal


def case_id(*params):
    return "_".join(str(p) for p in params)


def golden_path(test):
    return os.path.join(ROOT, "tests", "golden", "oracle_vs_reference_%s.npz" % test)


@functools.lru_cache(maxsize=None)
def _golden(test):
    with np.load(golden_path(test)) as z:
        return {k: z[k] for k in z.files}


def reference_outputs(test, case, trial):
    """The reference's arrays for one trial: {name: array} from the stored key '<case>__<trial>__<name>'."""
    prefix = "%s__%s__" % (case, trial)
    out = {k[len(prefix):]: v for k, v in _golden(test).items() if k.startswith(prefix)}
    assert out, "tests/golden/oracle_vs_reference_%s.npz holds nothing for %s" % (test, prefix)
    return out


def ordinary_problem(rng, d, nway=5):
    """(waypoints, vlim, alim) of one ordinary trajectory."""
    way = rng.standard_normal((nway, d))
    vmax = 10 + 20 * rng.random(d)
    amax = 10 + 2 * rng.random(d)
    return way, np.stack([-vmax, vmax], 1), np.stack([-amax, amax], 1)


def extreme_limit_problem(rng, kind, d, N, with_sd):
    """One problem whose limits sit at the edge of the number range (the table of kinds: extreme_limit_problems), and the
    ordinary problem it was made from: (knots, grid, waypoints, vlim, alim, sd_start, sd_end), (base waypoints, vlim, alim).
    Kind 'plain' is the base problem itself, drawn from the same stream; with_sd: non-zero boundary velocities.  No NaN
    anywhere."""
    way, vl, al = ordinary_problem(rng, d)
    base = (way.copy(), vl.copy(), al.copy())
    knots, grid = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    hit = rng.random(d) < 0.35
    hit[rng.integers(d)] = True                      # 30 - 40 % of the joints, at least one
    one = int(rng.choice(np.flatnonzero(hit)))       # the joint of the one-joint kinds
    # (every draw below is made for every kind, so that a kind's problem does not depend on the kinds before it)
    expo = rng.uniform(-23, -19, size=d)
    huge = np.where(rng.random(d) < 0.5, 1e38, 1e300)
    side, frac, s0 = rng.random() < 0.5, 0.01 + 0.05 * rng.random(), (5.0, -3.0, 1e3)[int(rng.integers(3))]
    order = rng.permutation(d)
    lattice = [np.round(0.2 * rng.random() * 1024) / 1024 for _ in range(2)]  # 2^-10 lattice: the squares are exact
    if kind == "vinf":
        vl[hit] = [-np.inf, np.inf]
    elif kind == "ainf":
        al[hit] = [-np.inf, np.inf]
    elif kind == "ainf_one":
        al[hit, 1] = np.inf
    elif kind == "vhuge":
        vl[hit] *= huge[hit, None]
    elif kind == "ahuge":
        al[hit] *= 1e300
    elif kind == "vsub":
        vl *= 10.0 ** expo[:, None]
    elif kind == "vtiny":
        vl[hit] *= 1e-30
    elif kind == "vneg":
        vl[one] = [frac * vl[one, 1], vl[one, 1]] if side else [vl[one, 0], frac * vl[one, 0]]
    elif kind == "inverted":
        al[one] = al[one, ::-1]
    elif kind == "still":
        way[:, hit] = way[:1, hit]
    elif kind == "shifted":
        knots, grid = s0 + knots, s0 + grid
    elif kind == "mix":
        j = [int(order[i % d]) for i in range(4)]
        vl[j[0]] = [-np.inf, np.inf]
        al[j[1], 1] = np.inf
        vl[j[2]] = base[1][j[2]] * 10.0 ** expo[j[2]]
        al[j[3]] = al[j[3]] * 1e300
    else:
        assert kind == "plain", kind
    sd0, sd1 = lattice if with_sd else (0.0, 0.0)
    return (knots, grid, way, vl, al, float(sd0), float(sd1)), base


def extreme_limit_problems(d, N, seed, trials=EXTREME_TRIALS):
    """Limits at the edge of the number range, on the ordinary problem ordinary_problem(rng, d) with 30 - 40 % of the joints (at
    least one) modified: `trials` x (kind, knots, grid, waypoints, vlim, alim, sd_start, sd_end) for every kind of

      vinf      vlim = (-inf, +inf)                       ainf      alim = (-inf, +inf)
      ainf_one  alim_hi = +inf only                       ahuge     alim x 1e300
      vhuge     vlim x 1e38 and x 1e300: quotients vlim / q' beyond FLT_MAX
      vsub      ALL vlim x 10^U(-23, -19): the fp32 square of sdmax is subnormal or underflows to 0
      vtiny     vlim x 1e-30: the square underflows to 0, x is pinned to 0
      vneg      vlim_hi < 0 or vlim_lo > 0 on one joint: a positive lower bound on sd, mostly infeasible
      inverted  alim_lo and alim_hi swapped on one joint: every stage infeasible
      still     the modified joints do not move (q' = q'' = 0: zero-normal rows, skipped in the velocity bound)
      shifted   knots and grid on [s0, s0 + 1], s0 in {5, -3, 1e3}
      mix       one joint each of vinf, ainf_one, vsub, ahuge in one trajectory

    Every third trial of a kind carries non-zero boundary velocities on the 2^-10 lattice."""
    rng = np.random.default_rng(31000 + seed)
    for kind in EXTREME_KINDS:
        for t in range(trials):
            yield (kind,) + extreme_limit_problem(rng, kind, d, N, t % 3 == 2)[0]


def extreme_limit_batch(B, d, N, seed, kinds=EXTREME_KINDS, shared_s0=None):
    """The same problems as one batch, for the batched entries and for tools/host_cert_hunt.py: trajectory b is of kind
    (kinds + ('plain',))[b % (len(kinds) + 1)] -- every 64-trajectory wave holds every kind next to ordinary trajectories, the
    `plain` controls at a fixed stride -- and every third round of kinds carries non-zero boundary velocities.
    dict(coef [B, 4, 4, d], breaks [B, 5], grid [B, N+1], vlim, alim [B, d, 2], sd0, sd1 [B], kinds [B], base): `base` holds
    the unmodified problems (coef, breaks, grid, vlim, alim) in the same layout.  With shared_s0 (a number) breaks [5] and grid
    [N+1] are one shifted set for the whole batch, and kind 'shifted' is an ordinary problem on it."""
    from toppra_amd.batch import spline_coefficients
    rng = np.random.default_rng(47000 + seed)
    names = tuple(kinds) + ("plain",)
    unit_k, unit_g = np.linspace(0, 1, 5), np.linspace(0, 1, N + 1)
    kind = [names[b % len(names)] for b in range(B)]
    out = {k: [] for k in ("knots", "grid", "way", "vlim", "alim", "sd0", "sd1")}
    base = {k: [] for k in ("way", "vlim", "alim")}
    for b in range(B):
        prob, (bw, bv, ba) = extreme_limit_problem(rng, kind[b], d, N, (b // len(names)) % 3 == 2)
        for k, v in zip(("knots", "grid", "way", "vlim", "alim", "sd0", "sd1"), prob):
            out[k].append(v)
        base["way"].append(bw); base["vlim"].append(bv); base["alim"].append(ba)
    out = {k: np.array(v) for k, v in out.items()}
    base = {k: np.array(v) for k, v in base.items()}
    if shared_s0 is not None:
        out["knots"], out["grid"] = shared_s0 + unit_k, shared_s0 + unit_g
        out["coef"], _ = spline_coefficients(out["knots"], out["way"])
        base.update(coef=spline_coefficients(out["knots"], base["way"])[0], breaks=out["knots"], grid=out["grid"])
    else:
        out["coef"] = np.empty((B, 4, 4, d))
        for k0 in np.unique(out["knots"][:, 0]):   # one batched fit per set of knots
            m = out["knots"][:, 0] == k0
            out["coef"][m], _ = spline_coefficients(out["knots"][m][0], out["way"][m])
        base.update(coef=spline_coefficients(unit_k, base["way"])[0], breaks=np.tile(unit_k, (B, 1)), grid=np.tile(unit_g, (B, 1)))
    out["breaks"] = out.pop("knots")
    out.update(kinds=np.array(kind), base=base)
    return out

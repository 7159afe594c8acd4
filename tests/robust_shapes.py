"""Problems and host-side checks shared by tests/test_gpu_robust_shapes.py (the robust kernels) and
tests/test_oracle_robust_independent.py (the CPU restatement of their method): nothing here needs a GPU.

A problem is the tuple (coef, breaks, grid, vlim or None, alim, sd_start or None, sd_end or None)."""
import numpy as np

from tests.solver_support import (EXTREME_KINDS, extreme_limit_batch, instantiation_problem, irregular_batch, oracle_flags, own_breakpoints,
                                  problem, same)
from toppra_amd import batch

ELL = [1e-3, 5e-2, 9e-3]  # examples/plot_robust_kinematics.py:26-28


def restatement(oracle, prob, interp, want_X):
    """prob: (coef, breaks, grid, vlim or None, alim, sd_start or None, sd_end or None).  The whole batch, every host thread."""
    coef, breaks, grid, vlim, alim, sd0, sd1 = prob
    return oracle.robust_solve_batch(coef, breaks, grid, vlim, alim, ELL, sd0, sd1, flags=oracle_flags(oracle, vlim is not None, interp),
                                     want_X=want_X, nthreads=0)


def keys(want_X):
    return ("K", "sd2", "u") + (("X",) if want_X else ())


def ok_share(ref):
    return float((ref["status"] == 0).mean())


def instantiation_case(d, per_traj_grid):
    """Part 1's batch: that of tests/test_gpu_instantiations.py (96 x d x 48; sd_start and sd_end non-zero on 30 %)."""
    data, grid, sd0, sd1 = instantiation_problem(96, d, 48, 1100 + d, per_traj_grid)
    return (data["coef"], data["breaks"], grid, data["vlim"], data["alim"], sd0, sd1)


def table_fits_lds(d, nseg):
    """robust_launch_group's condition for the rows-across-lanes kernel (tpr_group.hip.inc: GroupCfg::lds_doubles for a 64-thread
    block against kMaxDynamicLds): 64 / L trajectories, each with 3 (4 d + 6) doubles of rows and the spline table c0, c1, c2 per
    segment and dof plus the breakpoints.  L: 8 lanes per trajectory up to 8 dof, 16 above (for_dof)."""
    L = 8 if d <= 8 else 16
    return (64 // L) * (3 * (4 * d + 6) + 3 * nseg * d + nseg + 1) * 8 <= 65536


def last_fitting_nseg(d):
    nseg = 1
    while table_fits_lds(d, nseg + 1):
        nseg += 1
    return nseg


def block_threads(B, d, nseg):
    """group_launch_geometry's block size (tpr_group.hip.inc): the largest of 256 / 128 / 64 threads whose LDS fits, halved while the
    batch makes fewer than 4 x 256 blocks (shrink_block_to_batch).  A change there must be copied here: part 2 sits on it."""
    L = 8 if d <= 8 else 16
    table = table_fits_lds(d, nseg)
    threads = 64
    for t in (256, 128):
        if (t // L) * (3 * (4 * d + 6) + (3 * nseg * d + nseg + 1 if table else 0)) * 8 <= 65536:
            threads = t
            break
    while threads > 64 and B * L // threads < 4 * 256:
        threads //= 2
    return threads


def table_case(d, n_waypoints, own, B=64, N=24):
    """Part 3 / 6: the irregular batch on a spline of n_waypoints - 1 segments, on shared or per-trajectory breakpoints and grid.  Its
    boundary velocities (up to 0.3 on 40 % of the trajectories at either end) are drawn for paths of five or six waypoints.  Through n
    waypoints on random knots the end intervals are ~ 1 / n long, q'' there grows like n^2, and the admissible sd at the ends is
    ~ sqrt(amax / |q''|) ~ 3 / n, often less where two knots nearly coincide: the velocities are scaled by 1 / n, to a tenth of
    that.  (Unscaled, every trajectory with one fails at its first or last stage and under half of a batch is solved; with none,
    0.9 .. 1.0 of it.)"""
    data = irregular_batch(B, d, N, n_waypoints, seed=100 * d + n_waypoints)
    coef, breaks, grid = data["coef"], data["breaks"], data["grid"]
    if own:  # ... and a grid per trajectory with them: the interior gridpoints moved by up to a quarter of the narrowest interval
        coef, breaks = own_breakpoints(data, seed=d + n_waypoints)
        grid = np.repeat(grid[None], B, axis=0)
        grid[:, 1:-1] += np.random.default_rng(d + n_waypoints).uniform(-0.25, 0.25, size=(B, N - 1)) * np.diff(data["grid"]).min()
    scale = 1.0 / n_waypoints
    return (coef, breaks, grid, data["vlim"], data["alim"], scale * data["sd0"], scale * data["sd1"])


def many_dof_case(d, B=64, N=24):
    """Part 4 / 6: the irregular batch at 17..32 dof, six waypoints."""
    data = irregular_batch(B, d, N, 6, seed=3000 + d)
    return problem(data) + (data["sd0"], data["sd1"])


PARITY_CASES = ["per-trajectory grid, 10 dof", "long table, 7 dof, 43 waypoints", "20 dof"]


def parity_cases():
    """Part 6: name -> (prob, interpolation) for the independent solver; B <= 16."""
    c = instantiation_case(10, True)
    grid10 = (c[0][:16], c[1]) + tuple(x[:16] for x in c[2:])
    assert grid10[2].shape == (16, 49) and grid10[1].ndim == 1
    return {"per-trajectory grid, 10 dof": (grid10, True),
            "long table, 7 dof, 43 waypoints": (table_case(7, 43, False, B=12), True),
            "20 dof": (many_dof_case(20, B=12), False)}  # (the names: PARITY_CASES)


def as_checker_data(prob):
    coef, breaks, grid, vlim, alim, _, _ = prob
    return {"coef": coef, "breaks": breaks, "grid": grid, "vlim": vlim, "alim": alim}


def relaxed_twins(d, seed, slow, B=64, N=30):
    """Part 9's metamorphic pair on make_synthetic_batch(B, d, N): roughly a third of the joints of every trajectory -- at least
    one, never all -- lose their acceleration limits, written as +-inf in one problem and as 1e300 x the limit in the other.
    slow: the chosen joints' waypoints are scaled by 1e-5, so that |a| = |q'| < ru on their rows (rob_row_interval's A < 0 branch).
    -> (base problem, the +-inf problem, the 1e300 problem, chosen [B][d])"""
    assert d >= 3
    data = batch.make_synthetic_batch(B, d, N, seed=seed)
    rng = np.random.default_rng(seed)
    chosen = np.argsort(rng.random((B, d)), axis=1) < max(1, d // 3)   # ranks of a random permutation: exactly d // 3 per row
    coef = data["coef"]
    if slow:
        from scipy.interpolate import CubicSpline
        way = np.where(chosen[:, None, :], 1e-5 * data["waypoints"], data["waypoints"])
        coef, _ = batch.spline_coefficients(data["knots"], way)
        cs = CubicSpline(data["knots"], way.transpose(1, 0, 2))
        q1, q2 = cs(data["grid"], 1).transpose(1, 0, 2), cs(data["grid"], 2).transpose(1, 0, 2)   # [B][N+1][d]
        worst = np.maximum(np.abs(q1), np.abs(q1 + 2.0 / N * q2)).max(axis=1)                     # rows at s_i and the x_next rows
        assert (worst[chosen] < ELL[0]).all() and (worst[~chosen] > ELL[0]).all()
    alim = data["alim"]
    rng = np.random.default_rng(seed + 1)
    sd1 = np.where(rng.random(B) < 0.3, 0.2 * rng.random(B), 0.0)
    probs = [(coef, data["breaks"], data["grid"], data["vlim"], a, None, sd1)
             for a in (alim, np.where(chosen[..., None], np.sign(alim) * np.inf, alim), np.where(chosen[..., None], alim * 1e300, alim))]
    assert np.isinf(probs[1][4]).sum() == 2 * chosen.sum() and np.isfinite(probs[2][4]).all() and (np.abs(probs[2][4]) > 1e300).sum() == 2 * chosen.sum()
    return probs[0], probs[1], probs[2], chosen


RELAXED_CASES = [(3, False), (7, False), (12, False), (7, True), (12, True)]  # d, slow


def check_relaxed_twins(solve, d, slow):
    """solve(prob, interp, want_X) -> outputs.  Limits written as 1e300 x the ordinary ones and as +-inf: identical bits in every
    output, and status 0 wherever the problem with its ordinary limits has it (dropping rows only widens every set) -- not on all 64:
    a few trajectories of make_synthetic_batch are uncontrollable under their velocity limits and the limits of the untouched
    joints, and stay so; at least 0.9 of the batch must be solved with the ordinary limits, hence in both relaxed forms."""
    base, inf, huge, _ = relaxed_twins(d, 500 + d, slow)
    for interp in (True, False):
        b, i, h = (solve(p, interp, True) for p in (base, inf, huge))
        same(h, i, keys(True), (d, slow, interp, "1e300 vs inf"))
        assert (h["status"][b["status"] == 0] == 0).all(), (d, slow, interp, np.flatnonzero((b["status"] == 0) & (h["status"] != 0))[:6])
        assert (b["status"] == 0).mean() >= 0.9, (d, slow, interp)


def extreme_case(d, N):
    """Part 9: 16 rounds of the twelve kinds and the `plain` control; breakpoints and grid per trajectory."""
    data = extreme_limit_batch(208, d, N, d)
    return data, problem(data) + (data["sd0"], data["sd1"])


EXTREME_SHAPES = [(7, 24), (12, 16), (3, 20)]


def inf_twin(data, prob):
    """The same batch with every acceleration limit beyond 1e200 (kinds `ahuge` and `mix`) written as +-inf."""
    alim = prob[4]
    far = np.isfinite(alim) & (np.abs(alim) > 1e200)
    assert far[data["kinds"] == "ahuge"].any(axis=(1, 2)).all() and not far[~np.isin(data["kinds"], ("ahuge", "mix"))].any()
    return prob[:4] + (np.where(far, np.sign(alim) * np.inf, alim),) + prob[5:]


def check_extreme_counts(ref, twin, kinds):
    """On a solver's output for the extreme batch and for its +-inf twin: `ahuge` is solved wherever its twin is, and the batch is
    not vacuous."""
    ahuge = kinds == "ahuge"
    assert (ref["status"][ahuge][twin["status"][ahuge] == 0] == 0).all(), np.flatnonzero(ahuge & (twin["status"] == 0) & (ref["status"] != 0))
    assert (twin["status"][ahuge] == 0).sum() >= 8
    assert (ref["status"][kinds == "inverted"] == 1).all() and (ref["status"][kinds == "plain"] == 0).sum() >= 8
    return {k: int((ref["status"][kinds == k] == 0).sum()) for k in EXTREME_KINDS + ("plain",)}

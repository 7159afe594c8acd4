"""EVERY instantiation of the certified lane kernels (kernel family 3) is executed at least once against another kernel family.

Why: these kernels sit at the edge of the register file, and twice a value-identical change of unrelated
code made ONE instantiation return wrong results on every input (round 3: feasible sets at 11 / 13 dof; round 5: the forward
profiles of <5 dof, TOPPRAsd>) while its neighbours stayed right.  Such a defect is input-independent, so a small random batch
through each (dof, sd output, grid in LDS or per trajectory, Interpolation or Collocation) instantiation of cert_solve_kernel,
cert_feasible_kernel and the TOPPRAsd launch -- compared bit for bit with the rows-across-lanes kernels, which share no device code
with them beyond the row generation -- is a cheap net under all of them (15 dofs x 8 + 15 x 4 + 15 x 4 launches of 96 trajectories).
Round 6: the net is self-standing -- per dof one 96 x 48 batch of each discretisation also goes through the CPU restatement of
the reference (oracle/), so a defect in what the two kernel families SHARE (row generation, the division / square-root
sequences of tpr_device.hpp) cannot pass it either.  What a failure here usually is: profiles/r06_miscompile_root_cause.md."""
import numpy as np
import pytest

from tests.solver_support import instantiation_problem, oracle_flags, per_trajectory_grid, problem, same, same_array
from toppra_amd import batch

pytestmark = pytest.mark.gpu
B, N = 96, 48  # one full 64-lane block and a partial one


def _problem(d, seed, per_traj_grid):
    """-> (coef, breaks, grid, vlim, alim), sd_start, sd_end"""
    data, grid, sd0, sd1 = instantiation_problem(B, d, N, seed, per_traj_grid)
    return problem(dict(data, grid=grid)), sd0, sd1


@pytest.mark.parametrize("d", range(1, 16))
def test_every_solve_instantiation(gpu, oracle, d):
    for per_traj_grid in (False, True):
        prob, sd0, sd1 = _problem(d, 700 + d, per_traj_grid)
        for interp in (True, False):
            for want_sd in (False, True):
                want = batch.solve_batch(*prob, sd0, sd1, interp, want_sd=want_sd, variant=2)
                got = batch.solve_batch(*prob, sd0, sd1, interp, want_sd=want_sd, variant=3)
                what = (d, per_traj_grid, interp, want_sd)
                same(got, want, ("K", "sd2", "u") + (("sd",) if want_sd else ()), what)
                assert (want["status"] == 0).mean() > 0.5, what
            if not per_traj_grid:  # ... and the rows-across-lanes answer against the CPU restatement of the reference
                ref = oracle.solve_batch(*prob, sd0, sd1, flags=oracle_flags(oracle, True, interp), nthreads=4)
                same(want, ref, ("K", "sd2", "u"), (d, interp, "oracle"))


@pytest.mark.parametrize("d", range(1, 16))
def test_every_feasible_sets_and_toppra_sd_instantiation(gpu, d):
    for per_traj_grid in (False, True):
        prob, sd0, sd1 = _problem(d, 800 + d, per_traj_grid)
        desired = np.random.default_rng(d).uniform(0.5, 5.0, size=B)
        for interp in (True, False):
            what = (d, per_traj_grid, interp)
            X2 = batch.feasible_sets_batch(*prob, interp, variant=2)
            same_array(batch.feasible_sets_batch(*prob, interp, variant=3), X2, what + ("X",))
            a = batch.solve_desired_duration_batch(*prob, desired, sd0, sd1, variant=2, interpolation=interp)
            b = batch.solve_desired_duration_batch(*prob, desired, sd0, sd1, variant=3, interpolation=interp)
            same(b, a, ("K", "sd2", "sd", "u", "alpha"), what)


def _tight_joint_problem(d, seed):
    """4 d trajectories in which ONE joint's rows bind the stage LPs: joint j % d gets acceleration limits a fiftieth of the others'
    -- both signs, the upper one only (the + rows: c = -amax), the lower one only (the - rows: c = amin), or both with a velocity
    limit that binds as well.  Round 6's 15-dof incident (profiles/r06_dof15_unsplit_unit_incident.log) was a register tuple of ONE
    joint's limits restored with a stale low dword: wrong only where that joint's + row bound the forward LP, i.e. on a fifth of a
    random batch at isolated stages.  Here every joint's every kind of row binds at most stages of some trajectory."""
    Bt = 4 * d
    data = batch.make_synthetic_batch(Bt, d, N, seed=seed)
    alim = np.array(data["alim"], dtype=np.float64)   # [B][d][2] = (amin, amax)
    vlim = np.array(data["vlim"], dtype=np.float64)
    for j in range(Bt):
        k, kind = j % d, j // d
        if kind in (0, 1, 3):
            alim[j, k, 1] *= 0.02
        if kind in (0, 2, 3):
            alim[j, k, 0] *= 0.02
        if kind == 3:
            vlim[j, k] *= 0.05
    return dict(data, alim=alim, vlim=vlim)


@pytest.mark.parametrize("d", range(1, 16))
def test_every_joints_rows_bind_somewhere(gpu, oracle, d):
    data = _tight_joint_problem(d, 900 + d)
    desired = np.random.default_rng(50 + d).uniform(2.0, 40.0, size=4 * d)
    own_grids = per_trajectory_grid(np.random.default_rng(60 + d), 4 * d, N)
    # every instantiation: grid shared (in LDS up to 8 dof) / per trajectory, Interpolation / Collocation, with / without the sd output
    for grid, interp in ((data["grid"], True), (data["grid"], False), (own_grids, True), (own_grids, False)):
        prob = problem(dict(data, grid=grid))
        want = batch.solve_batch(*prob, None, None, interp, variant=2)
        got = batch.solve_batch(*prob, None, None, interp, variant=3)
        got_sd = batch.solve_batch(*prob, None, None, interp, want_sd=True, variant=3)
        same(got_sd, want, ("K", "sd2", "u"), (d, interp, grid.ndim, "family 3 with sd output"))
        ref = oracle.solve_batch(*prob, None, None, flags=oracle_flags(oracle, True, interp), nthreads=4)
        assert (ref["status"] == 0).mean() > 0.5, (d, interp, grid.ndim)
        same(want, ref, ("K", "sd2", "u"), (d, interp, "family 2 vs oracle"))
        same(got, ref, ("K", "sd2", "u"), (d, interp, "family 3 vs oracle"))
        for v in (1, 4) + ((5,) if d <= 7 else ()):  # (the other families on the same batch: one trajectory per lane / wave, two per wave)
            same(batch.solve_batch(*prob, None, None, interp, variant=v), ref, ("K", "sd2", "u"), (d, interp, "family %d vs oracle" % v))
        X2 = batch.feasible_sets_batch(*prob, interp, variant=2)
        same_array(batch.feasible_sets_batch(*prob, interp, variant=3), X2, (d, interp, "X"))
        a = batch.solve_desired_duration_batch(*prob, desired, None, None, variant=2, interpolation=interp)
        b = batch.solve_desired_duration_batch(*prob, desired, None, None, variant=3, interpolation=interp)
        same(b, a, ("K", "sd2", "sd", "u", "alpha"), (d, interp, "TOPPRAsd"))

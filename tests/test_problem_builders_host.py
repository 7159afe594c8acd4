"""What the Python layer of the solver stack promises without a device: the problems the three builders of ``_capi`` make, what
they refuse and in which order, the public signatures, and the declared C signatures.  Every expected value here is a literal
recorded before the builders, the pass bodies and the wrappers were folded onto shared helpers: this file is the evidence that
the fold moved nothing."""
import inspect
import itertools
import os

import numpy as np
import pytest
from scipy.interpolate import PPoly

from toppra_amd import _capi, algorithm, batch, solverwrapper

B, D, N = 3, 2, 4
DATA = batch.make_synthetic_batch(B, D, N)
Q, QS, QSS = (np.stack([PPoly(DATA["coef"][b], DATA["breaks"])(DATA["grid"], nu) for b in range(B)]) for nu in (0, 1, 2))


def _collocation_rows():
    """a, b, c, low, high, deltas of [acceleration limits] under Collocation: nC = 2 + 2 d = 6."""
    a, b, c = (np.zeros((B, N + 1, 2 + 2 * D)) for _ in range(3))
    a[..., 2:2 + D], a[..., 2 + D:] = QS, -QS
    b[..., 2:2 + D], b[..., 2 + D:] = QSS, -QSS
    c[..., 2:2 + D], c[..., 2 + D:] = -DATA["alim"][:, None, :, 1], DATA["alim"][:, None, :, 0]
    return a, b, c, np.full((B, N + 1, 2), -1e8), np.full((B, N + 1, 2), 1e8), np.diff(DATA["grid"])


ROWS = _collocation_rows()
SD = {"absent": None, "scalar": 0.25, "vector": np.array([0.1, 0.2, 0.3])}
BOOL = (False, True)


def _per_traj(x, on):
    return np.tile(x, (B, 1)) if on else x


def _check_tail(p, keep, head, sd_start, sd_end, active):
    """``keep`` is ``head`` arrays, then sd_start, sd_end, active where given, in that order; a pointer of the structure is
    null exactly when its array was not given and points to its ``keep`` entry otherwise; keep is C-contiguous fp64 (int32: active)."""
    names = list(head) + [n for n, v in (("sd_start", sd_start), ("sd_end", sd_end), ("active", active)) if v is not None]
    assert len(keep) == len(names)
    for name, arr in zip(names, keep):
        if arr is None:
            assert getattr(p, name) is None, name
            continue
        assert isinstance(arr, np.ndarray) and arr.flags["C_CONTIGUOUS"], name
        assert arr.dtype == (np.int32 if name == "active" else np.float64), name
        assert getattr(p, name) == arr.ctypes.data, name
    for name in ("vlim", "alim", "sd_start", "sd_end", "active"):
        if hasattr(p, name) and name not in names:
            assert getattr(p, name) is None, name
    for name, given in (("sd_start", sd_start), ("sd_end", sd_end)):
        if given is not None:
            got = keep[names.index(name)]
            assert got.shape == (B,) and np.array_equal(got, np.broadcast_to(given, (B,)))
    if active is not None:
        assert keep[-1] is active


def test_make_problem_accepts():
    count = 0
    for v, a, interp, pb, pg, squared, strict, sound, act in itertools.product(BOOL, repeat=9):
        for k0, k1 in itertools.product(SD, repeat=2):
            active = np.zeros((B, 4), dtype=np.int32) if act else None
            vlim, alim = DATA["vlim"] if v else None, DATA["alim"] if a else None
            p, keep = _capi.make_problem(DATA["coef"], _per_traj(DATA["breaks"], pb), _per_traj(DATA["grid"], pg), vlim, alim,
                                         SD[k0], SD[k1], interp, strict=strict, active=active, squared=squared, sound=sound)
            assert p.flags == 1 * v + 2 * a + 4 * (a and interp) + 16 * pb + 32 * pg + 128 * strict + 256 * squared + 512 * sound
            assert (p.B, p.d, p.nseg, p.N, p.variant) == (3, 2, 4, 4, 0)
            head = ["coef", "breaks", "grid"] + ["vlim"] * v + ["alim"] * a
            _check_tail(p, keep, head, SD[k0], SD[k1], active)
            assert keep[1].shape == ((3, 5) if pb else (5,)) and keep[2].shape == ((3, 5) if pg else (5,))
            count += 1
    assert count == 4608
    p, keep = _capi.make_problem(DATA["coef"], DATA["breaks"], DATA["grid"], DATA["vlim"], DATA["alim"])
    assert p.flags == 7
    grids = np.tile(DATA["grid"], (B, 1))
    p, keep = _capi.make_problem(DATA["coef"], np.tile(DATA["breaks"], (B, 1)), grids, DATA["vlim"], DATA["alim"], variant=3,
                                 strict=True, squared=True, sound=True)
    assert p.flags == 951 and p.variant == 3
    # float32 and strided inputs are converted, and an outer keep list is extended in place
    outer = ["mine"]
    p, keep = _capi.make_problem(DATA["coef"].astype(np.float32), DATA["breaks"], grids[:, ::1].T.copy().T, None, None, keep=outer)
    assert keep is outer and keep[0] == "mine" and len(keep) == 4 and p.flags == 32
    assert all(arr.dtype == np.float64 and arr.flags["C_CONTIGUOUS"] for arr in keep[1:])
    # the dof limit of a spline-table problem is the library's: the builder takes 33 dof
    assert _capi.make_problem(np.zeros((1, 4, 1, 33)), [0.0, 1.0], [0.0, 0.5, 1.0], None, None)[0].d == 33


def test_make_dense_problem_accepts():
    a, b, c, low, high, deltas = ROWS
    for per_traj, squared, act in itertools.product(BOOL, repeat=3):
        for k0, k1 in itertools.product(SD, repeat=2):
            active = np.zeros((B, 4), dtype=np.int32) if act else None
            p, keep = _capi.make_dense_problem(a, b, c, low, high, _per_traj(deltas, per_traj), SD[k0], SD[k1], squared=squared,
                                               active=active)
            assert p.flags == 256 * squared and (p.B, p.N, p.nC) == (3, 4, 6)
            _check_tail(p, keep, ["a", "b", "c", "low", "high", "deltas"], SD[k0], SD[k1], active)
            assert keep[5].shape == (3, 4) and np.array_equal(keep[5], np.tile(deltas, (B, 1)))
    for nC in (2, 122):
        rows = [np.zeros((B, N + 1, nC))] * 3
        assert _capi.make_dense_problem(*rows, low, high, deltas)[0].nC == nC


def test_make_sampled_problem_accepts():
    for v, a, interp, pg, squared, act, with_q, with_qss in itertools.product(BOOL, repeat=8):
        for k0, k1 in itertools.product(SD, repeat=2):
            active = np.zeros((B, 4), dtype=np.int32) if act else None
            vlim, alim = DATA["vlim"] if v else None, DATA["alim"] if a else None
            p, keep = _capi.make_sampled_problem(_per_traj(DATA["grid"], pg), Q if with_q else None, QS, QSS if with_qss else None,
                                                 vlim, alim, SD[k0], SD[k1], interp, active=active, squared=squared,
                                                 solver=with_qss)
            assert p.flags == 1 * v + 2 * a + 4 * (a and interp) + 32 * pg + 256 * squared
            assert (p.B, p.d, p.N) == (3, 2, 4)
            _check_tail(p, keep, ["grid", "q", "qs", "qss"] + ["vlim"] * v + ["alim"] * a, SD[k0], SD[k1], active)
            assert (keep[1] is None) == (not with_q) and (keep[3] is None) == (not with_qss)
    # the row limit is the solver passes' alone: 30 dof under Interpolation, 32 under Collocation, any dof up to 32 without them
    for d, interp, solver in ((30, True, True), (32, False, True), (31, True, False), (32, True, False)):
        z = np.zeros((B, N + 1, d))
        p, _ = _capi.make_sampled_problem(DATA["grid"], None, z, z, None, np.zeros((B, d, 2)), interpolation=interp, solver=solver)
        assert p.d == d and p.flags == 2 + 4 * interp


def test_make_boxed_problem_accepts():
    low, high = ROWS[3], ROWS[4]
    active = np.zeros((B, 4), dtype=np.int32)
    p, keep, lo, hi = _capi.make_boxed_problem(DATA["grid"], QS, QSS, DATA["alim"], low, high, 0.5, None, False, active=active,
                                               squared=True)
    assert p.flags == 2 + 256 and p.vlim is None and p.q is None and p.sd_end is None and p.active == active.ctypes.data
    assert len(keep) == 9 and keep[-2] is lo and keep[-1] is hi and keep[-3] is active
    assert np.array_equal(lo, low) and np.array_equal(hi, high) and lo.flags["C_CONTIGUOUS"]


def test_rows_per_stage_and_the_wrappers_row_counts():
    alim = DATA["alim"]
    assert [_capi.sampled_rows_per_stage(7, *args) for args in ((None, True), (None, False), (alim, True), (alim, False))] == [2, 2, 30, 16]
    blocks = [{"w0": np.zeros((B, N + 1, 2))}, {"w0": np.zeros((B, N + 1, 3)), "F": np.zeros((5, 3)), "interpolation": False}]
    assert batch.second_order_rows_per_stage(2, alim, True, blocks) == 2 + 8 + 8 + 5
    assert batch.second_order_rows_per_stage(2, None, True, blocks[:1]) == 2 + 8
    assert batch.second_order_rows_per_stage(2, alim, False, ()) == 6
    import toppra_amd as ta
    path = ta.SplineInterpolator(DATA["knots"], DATA["waypoints"][0])
    vel, acc = ta.constraint.JointVelocityConstraint(DATA["vlim"][0]), ta.constraint.JointAccelerationConstraint(DATA["alim"][0])
    assert solverwrapper.hipSeidelWrapper([vel, acc], path, DATA["grid"]).nC == 10
    assert solverwrapper.hipSeidelWrapper([vel], path, DATA["grid"]).nC == 2
    assert solverwrapper.hipSampledSeidelWrapper([vel, acc], path, DATA["grid"]).nC == 10
    acc.set_discretization_type(0)
    assert solverwrapper.hipSeidelWrapper([acc], path, DATA["grid"]).nC == 6


# ---- refusals: (what is replaced in the good call, exception, message) --------------------------------------------------------
F32_ACTIVE = np.zeros((B, 4), dtype=np.float32)
STRIDED_ACTIVE = np.zeros((B, 8), dtype=np.int32)[:, ::2]
NOT_INCREASING = np.array([0.0, 0.25, 0.25, 0.75, 1.0])
ACTIVE_TEXT = "active must be a C-contiguous int32 array [B, 4] (it is updated in place)"


def _table(**kw):
    args = dict(coef=DATA["coef"], breaks=DATA["breaks"], grid=DATA["grid"], vlim=DATA["vlim"], alim=DATA["alim"])
    args.update(kw)
    return _capi.make_problem(args.pop("coef"), args.pop("breaks"), args.pop("grid"), args.pop("vlim"), args.pop("alim"), **args)


def _dense(**kw):
    args = dict(zip(("a", "b", "c", "low", "high", "deltas"), ROWS))
    args.update(kw)
    return _capi.make_dense_problem(*[args.pop(k) for k in ("a", "b", "c", "low", "high", "deltas")], **args)


def _sampled(**kw):
    args = dict(grid=DATA["grid"], q=Q, qs=QS, qss=QSS, vlim=DATA["vlim"], alim=DATA["alim"])
    args.update(kw)
    return _capi.make_sampled_problem(*[args.pop(k) for k in ("grid", "q", "qs", "qss", "vlim", "alim")], **args)


def _boxed(**kw):
    args = dict(grid=DATA["grid"], qs=QS, qss=QSS, alim=DATA["alim"], low=ROWS[3], high=ROWS[4])
    args.update(kw)
    return _capi.make_boxed_problem(*[args.pop(k) for k in ("grid", "qs", "qss", "alim", "low", "high")], **args)


def _wide(d):
    z = np.zeros((B, N + 1, d))
    return dict(q=None, qs=z, qss=z, vlim=None, alim=np.zeros((B, d, 2)))


REFUSED = [
    (_table, dict(coef=DATA["coef"][0]), ValueError, "coef must have shape [B, 4, nseg, d]"),
    (_table, dict(coef=DATA["coef"][:, :3]), ValueError, "coef must have shape [B, 4, nseg, d]"),
    (_table, dict(grid=DATA["grid"][None, None]), ValueError, "grid must have shape [N+1] or [B, N+1] with B = 3, got (1, 1, 5)"),
    (_table, dict(grid=np.tile(DATA["grid"], (4, 1))), ValueError, "grid must have shape [N+1] or [B, N+1] with B = 3, got (4, 5)"),
    (_table, dict(breaks=np.tile(DATA["breaks"], (2, 1))), ValueError,
     "breaks must have shape [nseg+1] or [B, nseg+1] with B = 3, got (2, 5)"),
    (_table, dict(breaks=DATA["breaks"][None, None]), ValueError,
     "breaks must have shape [nseg+1] or [B, nseg+1] with B = 3, got (1, 1, 5)"),
    (_table, dict(grid=np.array([0.0])), ValueError, "grid needs at least two gridpoints"),
    (_table, dict(grid=NOT_INCREASING), ValueError, "grid must be strictly increasing"),
    (_table, dict(grid=np.tile(NOT_INCREASING, (3, 1))), ValueError, "grid must be strictly increasing"),
    (_table, dict(breaks=DATA["breaks"][:-1]), ValueError, "breaks must have nseg+1 entries"),
    (_table, dict(vlim=DATA["vlim"][:, :, :1]), ValueError, "vlim must have shape [B, d, 2] = [3, 2, 2], got (3, 2, 1)"),
    (_table, dict(vlim=DATA["vlim"][0]), ValueError, "vlim must have shape [B, d, 2] = [3, 2, 2], got (2, 2)"),
    (_table, dict(alim=DATA["alim"][:, :1]), ValueError, "alim must have shape [B, d, 2] = [3, 2, 2], got (3, 1, 2)"),
    (_table, dict(sd_start=np.zeros(B + 1)), ValueError, "sd_start must be a scalar or have shape [B] = [3], got (4,)"),
    (_table, dict(sd_end=np.zeros((B, 1))), ValueError, "sd_end must be a scalar or have shape [B] = [3], got (3, 1)"),
    (_table, dict(active=F32_ACTIVE), ValueError, ACTIVE_TEXT),
    (_table, dict(active=STRIDED_ACTIVE), ValueError, ACTIVE_TEXT),
    (_table, dict(active=np.zeros((B, 3), dtype=np.int32)), ValueError, ACTIVE_TEXT),
    (_table, dict(active=[[0, 0, 0, 0]] * B), ValueError, ACTIVE_TEXT),
    # two faults at once: which refusal wins
    (_table, dict(coef=DATA["coef"][:, :3], grid=NOT_INCREASING), ValueError, "coef must have shape [B, 4, nseg, d]"),
    (_table, dict(grid=NOT_INCREASING, breaks=DATA["breaks"][:-1]), ValueError, "grid must be strictly increasing"),
    (_table, dict(breaks=DATA["breaks"][:-1], vlim=DATA["vlim"][0]), ValueError, "breaks must have nseg+1 entries"),
    (_table, dict(vlim=DATA["vlim"][0], alim=DATA["alim"][0]), ValueError, "vlim must have shape [B, d, 2] = [3, 2, 2], got (2, 2)"),
    (_table, dict(alim=DATA["alim"][0], sd_start=np.zeros(B + 1)), ValueError, "alim must have shape [B, d, 2] = [3, 2, 2], got (2, 2)"),
    (_table, dict(sd_start=np.zeros(B + 1), sd_end=np.zeros(B + 2)), ValueError,
     "sd_start must be a scalar or have shape [B] = [3], got (4,)"),
    (_table, dict(sd_end=np.zeros(B + 1), active=F32_ACTIVE), ValueError, "sd_end must be a scalar or have shape [B] = [3], got (4,)"),

    (_dense, dict(a=ROWS[0][0]), ValueError, "a must have shape [B, N+1, nC]"),
    (_dense, dict(a=ROWS[0][:, :1]), ValueError, "dense rows need at least two gridpoints"),
    (_dense, dict(a=ROWS[0][..., :1]), ValueError, "nC = 1 rows per stage (incl. the two x_next rows) is outside 2..122"),
    (_dense, dict(a=np.zeros((B, N + 1, 123))), ValueError, "nC = 123 rows per stage (incl. the two x_next rows) is outside 2..122"),
    (_dense, dict(b=ROWS[1][..., :5]), ValueError, "b must have shape (3, 5, 6), got (3, 5, 5)"),
    (_dense, dict(c=ROWS[2][:2]), ValueError, "c must have shape (3, 5, 6), got (2, 5, 6)"),
    (_dense, dict(low=ROWS[3][..., :1]), ValueError, "low must have shape (3, 5, 2), got (3, 5, 1)"),
    (_dense, dict(high=ROWS[4][:, :4]), ValueError, "high must have shape (3, 5, 2), got (3, 4, 2)"),
    (_dense, dict(deltas=ROWS[5][:3]), ValueError, "deltas must have N = 4 entries"),
    (_dense, dict(deltas=np.tile(ROWS[5], (2, 1))), ValueError, "deltas must have shape [N] or [B, N] = [3, 4], got (2, 4)"),
    (_dense, dict(deltas=np.tile(ROWS[5], (1, 3, 1))), ValueError, "deltas must have shape [N] or [B, N] = [3, 4], got (1, 3, 4)"),
    (_dense, dict(sd_start=np.zeros(B + 1)), ValueError, "sd_start must be a scalar or have shape [B] = [3], got (4,)"),
    (_dense, dict(sd_end=np.zeros((1, B))), ValueError, "sd_end must be a scalar or have shape [B] = [3], got (1, 3)"),
    (_dense, dict(active=F32_ACTIVE), ValueError, ACTIVE_TEXT),
    (_dense, dict(active=STRIDED_ACTIVE), ValueError, ACTIVE_TEXT),
    (_dense, dict(a=np.zeros((B, 1, 123))), ValueError, "dense rows need at least two gridpoints"),
    (_dense, dict(a=np.zeros((B, N + 1, 123)), low=ROWS[3][..., :1]), ValueError,
     "nC = 123 rows per stage (incl. the two x_next rows) is outside 2..122"),
    (_dense, dict(c=ROWS[2][:2], low=ROWS[3][..., :1]), ValueError, "c must have shape (3, 5, 6), got (2, 5, 6)"),
    (_dense, dict(high=ROWS[4][:, :4], deltas=ROWS[5][:3]), ValueError, "high must have shape (3, 5, 2), got (3, 4, 2)"),
    (_dense, dict(deltas=ROWS[5][:3], sd_start=np.zeros(B + 1)), ValueError, "deltas must have N = 4 entries"),
    (_dense, dict(sd_start=np.zeros(B + 1), active=F32_ACTIVE), ValueError, "sd_start must be a scalar or have shape [B] = [3], got (4,)"),

    (_sampled, dict(qs=QS[0]), ValueError, "qs must have shape [B, N+1, d], got (5, 2)"),
    (_sampled, dict(qs=QS[:, :1]), ValueError, "a sampled path needs at least two gridpoints"),
    (_sampled, _wide(33), NotImplementedError, "dof 33 is outside 1..32"),
    (_sampled, dict(qs=QS[..., :0]), NotImplementedError, "dof 0 is outside 1..32"),
    (_sampled, dict(qss=None), ValueError, "the solver passes need qss = path(grid, 2)"),
    (_sampled, dict(qss=QSS[..., :1]), ValueError, "qss must have the shape of qs, [B, N+1, d] = [3, 5, 2], got (3, 5, 1)"),
    (_sampled, dict(q=Q[:2]), ValueError, "q must have the shape of qs, [B, N+1, d] = [3, 5, 2], got (2, 5, 2)"),
    (_sampled, dict(grid=DATA["grid"][:4]), ValueError, "grid must have shape [N+1] or [B, N+1] = [3, 5], got (4,)"),
    (_sampled, dict(grid=np.tile(DATA["grid"], (2, 1))), ValueError, "grid must have shape [N+1] or [B, N+1] = [3, 5], got (2, 5)"),
    (_sampled, dict(grid=NOT_INCREASING), ValueError, "grid must be strictly increasing"),
    (_sampled, _wide(31), NotImplementedError, "31 dof under Interpolation: 126 constraint rows per stage (incl. the two x_next rows), "
     "the sampled passes hold 122 (30 dof; 32 under Collocation)"),
    (_sampled, dict(vlim=DATA["vlim"][:, :, :1]), ValueError, "vlim must have shape [B, d, 2] = [3, 2, 2], got (3, 2, 1)"),
    (_sampled, dict(alim=DATA["alim"][:, :1]), ValueError, "alim must have shape [B, d, 2] = [3, 2, 2], got (3, 1, 2)"),
    (_sampled, dict(sd_start=np.zeros(B + 1)), ValueError, "sd_start must be a scalar or have shape [B] = [3], got (4,)"),
    (_sampled, dict(sd_end=np.zeros((B, 1))), ValueError, "sd_end must be a scalar or have shape [B] = [3], got (3, 1)"),
    (_sampled, dict(active=F32_ACTIVE), ValueError, ACTIVE_TEXT),
    (_sampled, dict(active=STRIDED_ACTIVE), ValueError, ACTIVE_TEXT),
    (_sampled, dict(_wide(33), qss=None), NotImplementedError, "dof 33 is outside 1..32"),
    (_sampled, dict(qss=None, q=Q[:2]), ValueError, "the solver passes need qss = path(grid, 2)"),
    (_sampled, dict(qss=QSS[..., :1], q=Q[:2]), ValueError, "qss must have the shape of qs, [B, N+1, d] = [3, 5, 2], got (3, 5, 1)"),
    (_sampled, dict(q=Q[:2], grid=NOT_INCREASING), ValueError, "q must have the shape of qs, [B, N+1, d] = [3, 5, 2], got (2, 5, 2)"),
    (_sampled, dict(_wide(31), vlim=np.zeros((B, 2, 2))), NotImplementedError,
     "31 dof under Interpolation: 126 constraint rows per stage (incl. the two x_next rows), the sampled passes hold 122 "
     "(30 dof; 32 under Collocation)"),
    (_sampled, dict(_wide(31), grid=NOT_INCREASING), ValueError, "grid must be strictly increasing"),
    (_sampled, dict(vlim=DATA["vlim"][0], alim=DATA["alim"][0]), ValueError, "vlim must have shape [B, d, 2] = [3, 2, 2], got (2, 2)"),
    (_sampled, dict(alim=DATA["alim"][0], sd_end=np.zeros(B + 1)), ValueError, "alim must have shape [B, d, 2] = [3, 2, 2], got (2, 2)"),
    (_sampled, dict(sd_end=np.zeros(B + 1), active=F32_ACTIVE), ValueError, "sd_end must be a scalar or have shape [B] = [3], got (4,)"),

    (_boxed, dict(vlim=DATA["vlim"]), NotImplementedError, "the boxed passes take no vlim: the boxes carry every first-order constraint "
     "-- make the limits a (\"vlim\", vlim) source of stage_boxes_batch"),
    (_boxed, dict(vlim=DATA["vlim"], qs=QS[0]), NotImplementedError, "the boxed passes take no vlim: the boxes carry every first-order "
     "constraint -- make the limits a (\"vlim\", vlim) source of stage_boxes_batch"),
    (_boxed, dict(low=ROWS[3][..., :1]), ValueError, "low must have shape [B, N+1, 2] = [3, 5, 2], got (3, 5, 1)"),
    (_boxed, dict(high=np.full((B, N + 1, 2), np.nan)), ValueError, "high holds NaN (use +-inf for 'no bound')"),
    (_boxed, dict(active=F32_ACTIVE, low=ROWS[3][..., :1]), ValueError, ACTIVE_TEXT),
    (_boxed, dict(low=ROWS[3][..., :1], high=np.full((B, N + 1, 2), np.nan)), ValueError,
     "low must have shape [B, N+1, 2] = [3, 5, 2], got (3, 5, 1)"),
]


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_refused_problem(case):
    build, bad, exc, text = REFUSED[case]
    with pytest.raises(exc) as err:
        build(**bad)
    assert type(err.value) is exc and str(err.value) == text


def _too_many_rows():
    """A second-order block of 60 rows under Interpolation beside the acceleration block: 2 + 8 + 120 = 130 rows."""
    return [{"w0": np.zeros((B, N + 1, D)), "wa": np.zeros((B, N + 1, D)), "wb": np.zeros((B, N + 1, D)), "F": np.zeros((60, D)),
             "g": np.zeros(60)}]


ROW_LIMIT_TEXT = "130 constraint rows per stage (incl. the two x_next rows): the dense-row kernels hold 122"


def test_the_generic_row_limit_is_refused_before_any_launch():
    """The row builders and BatchTOPPRA refuse from shapes alone: no device is touched before the refusal."""
    with pytest.raises(NotImplementedError) as err:
        batch.second_order_rows_batch(DATA["coef"], DATA["breaks"], DATA["grid"], DATA["vlim"], DATA["alim"], _too_many_rows())
    assert str(err.value) == ROW_LIMIT_TEXT
    with pytest.raises(NotImplementedError) as err:
        batch.sampled_rows_batch(DATA["grid"], QS, QSS, DATA["vlim"], DATA["alim"], _too_many_rows())
    assert str(err.value) == ROW_LIMIT_TEXT
    with pytest.raises(ValueError) as err:  # the samples are checked before the blocks, the blocks before the limit
        batch.sampled_rows_batch(DATA["grid"], QS, None, DATA["vlim"], DATA["alim"], _too_many_rows())
    assert str(err.value) == "the rows need qss = path(grid, 2)"
    with pytest.raises(ValueError) as err:
        batch.second_order_rows_batch(DATA["coef"][0], DATA["breaks"], DATA["grid"], DATA["vlim"], DATA["alim"], _too_many_rows())
    assert str(err.value) == "coef must have shape [B, 4, nseg, d]"
    from toppra_amd.constraint import BatchSecondOrderConstraint
    blk = _too_many_rows()[0]
    con = BatchSecondOrderConstraint(lambda q, qd, qdd: qdd, F=blk["F"], g=blk["g"])
    for make in (lambda: algorithm.BatchTOPPRA(DATA["coef"], DATA["breaks"], DATA["grid"], DATA["vlim"], DATA["alim"], constraints=[con]),
                 lambda: algorithm.BatchTOPPRA.from_path_samples(DATA["grid"], Q, QS, QSS, DATA["vlim"], DATA["alim"], constraints=[con])):
        with pytest.raises(NotImplementedError) as err:
            make()
        assert str(err.value) == ROW_LIMIT_TEXT
    with pytest.raises(ValueError) as err:
        algorithm.BatchTOPPRA(DATA["coef"][0], DATA["breaks"], DATA["grid"], DATA["vlim"], DATA["alim"], constraints=[con])
    assert str(err.value) == "coef must have shape [B, 4, nseg, d]"


SIGNATURES = {
    "solve_batch": "(coef, breaks, grid, vlim, alim, sd_start=None, sd_end=None, interpolation=True, want_sd=False, variant=0, strict=False, want_K=True, want_u=True, active=None, sound=False)",
    "controllable_sets_batch": "(coef, breaks, grid, vlim, alim, sdmin, sdmax, interpolation=True, active=None, squared=False, variant=0, strict=False, sound=False)",
    "feasible_sets_batch": "(coef, breaks, grid, vlim, alim, interpolation=True, active=None, variant=0, strict=False, sound=False)",
    "reachable_sets_batch": "(coef, breaks, grid, vlim, alim, sdmin, sdmax, interpolation=True, want_X=False, squared=False)",
    "constraint_params_batch": "(coef, breaks, grid, vlim, alim, interpolation=True)",
    "make_synthetic_batch": "(B, d, N, seed=20240924, n_waypoints=5)",
    "spline_coefficients": "(knots, waypoints, bc_type='not-a-knot')",
    "spline_fit_batch": "(knots, waypoints, bc_type='not-a-knot')",
    "solve_batch_timed": "(coef, breaks, grid, vlim, alim, out, reps, sd_start=None, sd_end=None, interpolation=True, variant=0, strict=False, sound=False)",
    "const_accel_times_batch": "(grid, sd)",
    "const_accel_eval_batch": "(coef, breaks, grid, sd, ts, us, times, order=0)",
    "solve_desired_duration_batch": "(coef, breaks, grid, vlim, alim, desired_duration, sd_start=None, sd_end=None, atol=1e-05, variant=0, interpolation=True, squared=False)",
    "robust_solve_batch": "(coef, breaks, grid, vlim, alim, ellipsoid, sd_start=None, sd_end=None, interpolation=True, want_X=False, variant=0)",
    "param_spline_batch": "(coef, breaks, grid, sd, variant=0)",
    "ppoly_eval_batch": "(coef, breaks, times, order=0, counts=None)",
    "path_eval_batch": "(coef, breaks, grid, orders=(0, 1, 2))",
    "second_order_rows_batch": "(coef, breaks, grid, vlim, alim, blocks, interpolation=True)",
    "sampled_rows_batch": "(grid, qs, qss, vlim, alim, blocks=(), interpolation=True)",
    "solve_sampled_batch": "(grid, qs, qss, vlim, alim, sd_start=None, sd_end=None, interpolation=True, want_sd=False, squared=False, active=None)",
    "controllable_sets_sampled_batch": "(grid, qs, qss, vlim, alim, sdmin, sdmax, interpolation=True, squared=False, active=None)",
    "feasible_sets_sampled_batch": "(grid, qs, qss, vlim, alim, interpolation=True, active=None)",
    "reachable_sets_sampled_batch": "(grid, qs, qss, vlim, alim, sdmin, sdmax, interpolation=True, want_X=False, active=None, squared=False)",
    "solve_desired_duration_sampled_batch": "(grid, qs, qss, vlim, alim, desired_duration, sd_start=None, sd_end=None, atol=1e-05, interpolation=True, active=None, squared=False)",
    "param_spline_samples_batch": "(grid, q, qs, sd)",
    "stage_boxes_batch": "(qs, sources, N=None)",
    "solve_sampled_boxed_batch": "(grid, qs, qss, alim, low, high, sd_start=None, sd_end=None, interpolation=True, want_sd=False, squared=False, active=None, vlim=None)",
    "solve_desired_duration_sampled_boxed_batch": "(grid, qs, qss, alim, low, high, desired_duration, sd_start=None, sd_end=None, atol=1e-05, interpolation=True, active=None, squared=False, vlim=None)",
    "controllable_sets_sampled_boxed_batch": "(grid, qs, qss, alim, low, high, sdmin, sdmax, interpolation=True, squared=False, active=None, vlim=None)",
    "feasible_sets_sampled_boxed_batch": "(grid, qs, qss, alim, low, high, interpolation=True, active=None, vlim=None)",
    "reachable_sets_sampled_boxed_batch": "(grid, qs, qss, alim, low, high, sdmin, sdmax, interpolation=True, want_X=False, active=None, squared=False, vlim=None)",
    "chain_inverse_dynamics_batch": "(chain, q, qd, qdd)",
    "chain_torque_terms_batch": "(chain, q, qs, qss)",
    "chain_tool_bound_batch": "(chain, q, qs, limit=None, S=None)",
    "chain_tool_acceleration_batch": "(chain, q, qd, qdd)",
    "chain_tool_acceleration_terms_batch": "(chain, q, qs, qss)",
    "chain_tool_wrench_batch": "(chain, q, qd, qdd, payload)",
    "chain_tool_wrench_terms_batch": "(chain, q, qs, qss, payload)",
    "chain_points_speed_batch": "(chain, q, qs, points, limit=None)",
    "chain_points_acceleration_batch": "(chain, q, qd, qdd, points)",
    "chain_points_acceleration_terms_batch": "(chain, q, qs, qss, points)",
    "tree_inverse_dynamics_batch": "(tree, q, qd, qdd)",
    "tree_torque_terms_batch": "(tree, q, qs, qss)",
    "base_wrench_batch": "(robot, q, qd, qdd, mount=None)",
    "base_wrench_terms_batch": "(robot, q, qs, qss, mount=None)",
    "joint_wrench_batch": "(robot, q, qd, qdd, sections)",
    "joint_wrench_terms_batch": "(robot, q, qs, qss, sections)",
    "momentum_batch": "(robot, q, qs, mount=None, links=None, limit=None)",
    "momentum_bound_batch": "(robot, q, qs, limit, mount=None, links=None)",
    "link_mask": "(robot, links=None)",
}
CLASS_SIGNATURES = {
    "BatchTOPPRA.__init__": "(self, coef, breaks, gridpoints, vlim, alim, interpolation=True, constraints=None)",
    "BatchTOPPRA.compute_controllable_sets": "(self, sdmin, sdmax)",
    "BatchTOPPRA.compute_feasible_sets": "(self)",
    "BatchTOPPRA.compute_parameterization": "(self, sd_start=None, sd_end=None, want_sd=True, variant=0, want_K=True, want_u=True)",
    "BatchTOPPRA.compute_parameterization_sd": "(self, desired_duration, sd_start=None, sd_end=None, atol=1e-05)",
    "BatchTOPPRA.compute_reachable_sets": "(self, sdmin, sdmax)",
    "BatchTOPPRA.compute_trajectory": "(self, sd_start=None, sd_end=None, parametrizer='ParametrizeSpline')",
    "BatchTOPPRA.compute_trajectory_samples": "(self, times, sd_start=None, sd_end=None, fractions=True, orders=(0,))",
    "BatchTOPPRA.dense_rows": "(self)",
    "BatchTOPPRA.from_path_samples": "(gridpoints, q, qs, qss, vlim, alim, interpolation=True, constraints=None)",
    "BatchTOPPRA.from_waypoints": "(knots, waypoints, gridpoints, vlim, alim, bc_type='not-a-knot', gpu_fit=True, **kw)",
    "BatchTOPPRA.return_codes": "(status)",
    "BatchTOPPRA.stage_boxes": "(self)",
    "hipSeidelWrapper.__init__": "(self, constraint_list, path, path_discretization, solve_lp1d=0)",
    "hipSeidelWrapper.close_solver": "(self)",
    "hipSeidelWrapper.controllable_sets": "(self, sdmin, sdmax)",
    "hipSeidelWrapper.feasible_sets": "(self)",
    "hipSeidelWrapper.get_deltas": "(self)",
    "hipSeidelWrapper.get_no_stages": "(self)",
    "hipSeidelWrapper.get_no_vars": "(self)",
    "hipSeidelWrapper.parameterization": "(self, sd_start, sd_end)",
    "hipSeidelWrapper.parameterization_sd": "(self, sd_start, sd_end, desired_duration, atol=1e-05)",
    "hipSeidelWrapper.reachable_sets": "(self, sdmin, sdmax)",
    "hipSeidelWrapper.setup_solver": "(self)",
    "hipSeidelWrapper.solve_stagewise_optim": "(self, i, H, g, x_min, x_max, x_next_min, x_next_max)",
    "hipDenseSeidelWrapper.__init__": "(self, constraint_list, path, path_discretization, solve_lp1d=1, active=None)",
    "hipDenseSeidelWrapper.close_solver": "(self)",
    "hipDenseSeidelWrapper.controllable_sets": "(self, sdmin, sdmax)",
    "hipDenseSeidelWrapper.feasible_sets": "(self)",
    "hipDenseSeidelWrapper.get_deltas": "(self)",
    "hipDenseSeidelWrapper.get_no_stages": "(self)",
    "hipDenseSeidelWrapper.get_no_vars": "(self)",
    "hipDenseSeidelWrapper.parameterization": "(self, sd_start, sd_end)",
    "hipDenseSeidelWrapper.parameterization_sd": "(self, sd_start, sd_end, desired_duration, atol=1e-05)",
    "hipDenseSeidelWrapper.reachable_sets": "(self, sdmin, sdmax)",
    "hipDenseSeidelWrapper.setup_solver": "(self)",
    "hipDenseSeidelWrapper.solve_stagewise_optim": "(self, i, H, g, x_min, x_max, x_next_min, x_next_max)",
    "hipSampledSeidelWrapper.__init__": "(self, constraint_list, path, path_discretization, solve_lp1d=1)",
    "hipSampledSeidelWrapper.close_solver": "(self)",
    "hipSampledSeidelWrapper.controllable_sets": "(self, sdmin, sdmax)",
    "hipSampledSeidelWrapper.feasible_sets": "(self)",
    "hipSampledSeidelWrapper.get_deltas": "(self)",
    "hipSampledSeidelWrapper.get_no_stages": "(self)",
    "hipSampledSeidelWrapper.get_no_vars": "(self)",
    "hipSampledSeidelWrapper.parameterization": "(self, sd_start, sd_end)",
    "hipSampledSeidelWrapper.parameterization_sd": "(self, sd_start, sd_end, desired_duration, atol=1e-05)",
    "hipSampledSeidelWrapper.reachable_sets": "(self, sdmin, sdmax)",
    "hipSampledSeidelWrapper.setup_solver": "(self)",
    "hipSampledSeidelWrapper.solve_stagewise_optim": "(self, i, H, g, x_min, x_max, x_next_min, x_next_max)",
    "hipRobustWrapper.__init__": "(self, constraint_list, path, path_discretization)",
    "hipRobustWrapper.close_solver": "(self)",
    "hipRobustWrapper.controllable_sets": "(self, sdmin, sdmax)",
    "hipRobustWrapper.feasible_sets": "(self)",
    "hipRobustWrapper.get_deltas": "(self)",
    "hipRobustWrapper.get_no_stages": "(self)",
    "hipRobustWrapper.get_no_vars": "(self)",
    "hipRobustWrapper.parameterization": "(self, sd_start, sd_end)",
    "hipRobustWrapper.setup_solver": "(self)",
    "hipRobustWrapper.solve_stagewise_optim": "(self, i, H, g, x_min, x_max, x_next_min, x_next_max)",
}
ARGTYPES = {
    "tpr_init": 1, "tpr_device_count": None, "tpr_last_error": None, "tpr_version": None, "tpr_abi_sizes": 3,
    "tpr_solve_batch": 3, "tpr_controllable_sets_batch": 5, "tpr_feasible_sets_batch": 3, "tpr_constraint_params_batch": 10,
    "tpr_solve_stagewise_batch": 8, "tpr_lp1d_batch": 12, "tpr_lp2d_batch": 14, "tpr_solve_batch_timed": 5,
    "tpr_spline_fit_batch": 13, "tpr_const_accel_times_batch": 5, "tpr_const_accel_eval_batch": 9,
    "tpr_solve_desired_duration_batch": 6, "tpr_robust_solve_batch": 5, "tpr_param_spline_batch": 6,
    "tpr_ppoly_eval_batch": 12, "tpr_reachable_sets_batch": 6, "tpr_solve_dense_batch": 3,
    "tpr_controllable_sets_dense_batch": 5, "tpr_feasible_sets_dense_batch": 3, "tpr_solve_desired_duration_dense_batch": 6,
    "tpr_reachable_sets_dense_batch": 6, "tpr_param_spline_sample_batch": 11, "tpr_path_eval_batch": 5,
    "tpr_second_order_rows_batch": 10, "tpr_second_order_block_bytes": 0, "tpr_sampled_problem_bytes": 0,
    "tpr_sampled_rows_batch": 11, "tpr_solve_sampled_batch": 3, "tpr_controllable_sets_sampled_batch": 5,
    "tpr_feasible_sets_sampled_batch": 3, "tpr_reachable_sets_sampled_batch": 6,
    "tpr_solve_desired_duration_sampled_batch": 6, "tpr_param_spline_samples_batch": 6, "tpr_bound_source_bytes": 0,
    "tpr_stage_boxes_batch": 10, "tpr_solve_sampled_boxed_batch": 5, "tpr_solve_desired_duration_sampled_boxed_batch": 8,
    "tpr_controllable_sets_sampled_boxed_batch": 7, "tpr_feasible_sets_sampled_boxed_batch": 5,
    "tpr_reachable_sets_sampled_boxed_batch": 8, "tpr_chain_bytes": 0, "tpr_chain_inverse_dynamics_batch": 8,
    "tpr_chain_torque_terms_batch": 11, "tpr_chain_tool_velocity_batch": 11, "tpr_chain_tool_acceleration_batch": 8,
    "tpr_chain_tool_acceleration_terms_batch": 10, "tpr_payload_bytes": 0, "tpr_chain_tool_wrench_batch": 9,
    "tpr_chain_tool_wrench_terms_batch": 12, "tpr_chain_points_bytes": 0, "tpr_chain_points_speed_batch": 11,
    "tpr_chain_points_acceleration_batch": 9, "tpr_chain_points_acceleration_terms_batch": 11,
    "tpr_tree_inverse_dynamics_batch": 9, "tpr_tree_torque_terms_batch": 12, "tpr_mount_bytes": 0,
    "tpr_tree_base_wrench_batch": 10, "tpr_tree_base_wrench_terms_batch": 13, "tpr_joint_sections_bytes": 0,
    "tpr_tree_joint_wrench_batch": 10, "tpr_tree_joint_wrench_terms_batch": 13, "tpr_tree_momentum_batch": 14,
}


def test_public_signatures():
    assert sorted(SIGNATURES) == sorted(batch.__all__)
    for name, text in SIGNATURES.items():
        assert str(inspect.signature(getattr(batch, name))) == text, name
    classes = {cls.__name__: cls for cls in (algorithm.BatchTOPPRA, solverwrapper.hipSeidelWrapper, solverwrapper.hipDenseSeidelWrapper,
                                             solverwrapper.hipSampledSeidelWrapper, solverwrapper.hipRobustWrapper)}
    for cls in classes.values():
        public = ["__init__"] + [n for n, v in inspect.getmembers(cls) if not n.startswith("_") and callable(v)]
        assert sorted("%s.%s" % (cls.__name__, n) for n in public) == sorted(k for k in CLASS_SIGNATURES if k.startswith(cls.__name__ + "."))
    for name, text in CLASS_SIGNATURES.items():
        cls, method = name.split(".")
        assert str(inspect.signature(getattr(classes[cls], method))) == text, name


def test_load_declares_every_export():
    if not os.path.exists(_capi.LIB_PATH):
        pytest.skip("libtoppra_hip.so is not built")
    import ctypes as C
    lib = _capi.load()
    assert sorted(ARGTYPES) == sorted(_capi.EXPORTS)
    other = {"tpr_init": C.c_int, "tpr_device_count": C.c_int, "tpr_last_error": C.c_char_p, "tpr_version": C.c_char_p}
    for name in _capi.EXPORTS:
        entry = getattr(lib, name)
        assert entry.restype is other.get(name, C.c_int), name
        assert (None if entry.argtypes is None else len(entry.argtypes)) == ARGTYPES[name], name
        if name not in other:
            assert isinstance(entry.argtypes, (list, tuple)), name

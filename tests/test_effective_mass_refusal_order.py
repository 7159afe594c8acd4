"""Which refusal wins when two arguments of tpr_tree_effective_mass_batch (include/toppra_hip_contact.h) are bad at once, through
ctypes; every case is refused, nothing is launched, and the buffers handed over are 64 doubles long.  The order is behaviour, as
tests/test_momentum_refusal_order.py pins it for the entry's sibling: B / N; then what tpr_tree_momentum_batch refuses of the links
and the parent table, in its order -- the links as a chain, the parent table, the fork count --; then the points (NULL, the
count, a link outside the robot, an offset that is not finite); then a direction that is not finite; then a NULL q; a NULL qs
where it is needed; all outputs NULL; xbound without limit.

The first half needs no GPU: it is what the entry decides before it looks for a device."""
import ctypes

import numpy as np
import pytest

from tests.rigid_support import BADARG, BUF as _BUF, UNSUPPORTED, c_model as _model, parent_table as _parent

NAME = "tpr_tree_effective_mass_batch"
_KEEP = []


def _points(count=2, links=(0, 2), offsets=None):
    from toppra_amd import _capi
    pts = _capi.tpr_chain_points(count=count)
    for k, link in enumerate(links):
        pts.link[k] = link
    for k, off in enumerate(offsets or ()):
        pts.offset[k][:] = off
    return pts


def _direction(values):
    u = np.ascontiguousarray(values, dtype=np.float64)
    _KEEP.append(u)
    return u


def _call(model, parent, points, direction=None, B=1, N=1, q=True, qs=True, limit=True, outputs=(True, True, True)):
    """(code, message) of one call: ``model`` / ``parent`` / ``points`` / ``direction`` may be None (NULL); ``q``, ``qs``, ``limit``
    False pass NULL, ``outputs`` says which of speed2, mobility, xbound are given."""
    from toppra_amd import contact
    lib = contact.load()
    p = _BUF.ctypes.data
    rc = lib.tpr_tree_effective_mass_batch(None if model is None else ctypes.byref(model), None if parent is None else parent.ctypes.data,
                                           None if points is None else ctypes.byref(points),
                                           None if direction is None else direction.ctypes.data, B, N, p if q else None,
                                           p if qs else None, p if limit else None, *[p if given else None for given in outputs], 0, None)
    return rc, lib.tpr_last_error()


# ---- without a GPU: what is decided before the links are looked at (check_chain looks for a device first) ------------------------

@pytest.mark.parametrize("B, N", [(-1, 1), (1, -1)])
def test_a_negative_b_or_n_is_refused_before_everything_else(B, N):
    rc, msg = _call(None, None, None, B=B, N=N, q=False, outputs=(False, False, False))
    assert rc == BADARG and b"B >= 0, N >= 0" in msg and NAME.encode() in msg, msg


def test_valid_early_arguments_reach_the_device_check():
    from toppra_amd import _capi
    sc, model = _model()
    if _capi.device_count() == 0:  # (with a device the call would be valid and run)
        rc, msg = _call(model, _parent(), _points())
        assert rc < 0 and b"tpr_init" in msg, msg
        # ... and so does a call whose later arguments are all bad: the device check comes with the links, before them
        rc, msg = _call(model, _parent(), None, _direction([[np.nan] * 3] * 2), q=False, outputs=(False, False, False))
        assert rc < 0 and b"tpr_init" in msg, msg


# ---- with a GPU: what the checks after B / N decide; every call is refused ------------------------------------------------------

@pytest.mark.gpu
def test_the_links_are_refused_before_the_parent_table_and_the_rest(gpu):
    rc, msg = _call(None, None, None, q=False)
    assert rc == BADARG and b"null chain" in msg and NAME.encode() in msg, msg
    sc, model = _model(dof=33)
    rc, msg = _call(model, None, None, outputs=(False, False, False))
    assert rc == BADARG and b"the chain's dof must be in [1, TPR_MAX_DOF]" in msg, msg
    sc, model = _model(joint_type=[0, 7, 0])
    rc, msg = _call(model, None, _points())
    assert rc == BADARG and b"unknown joint type" in msg, msg


@pytest.mark.gpu
def test_the_parent_table_and_the_fork_count_before_the_points(gpu):
    sc, model = _model()
    rc, msg = _call(model, None, None)
    assert rc == BADARG and b"null parent array" in msg, msg
    rc, msg = _call(model, _parent(table=[-1, 0, 2]), _points(count=0), q=False)
    assert rc == BADARG and b"the parent of link 2 is 2, outside -1 .. 1" in msg, msg
    sc, model = _model(d=11)
    five = _parent(table=[-1, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4])
    rc, msg = _call(model, five, None, outputs=(False, False, False))
    assert rc == UNSUPPORTED and b"the tree has 5 forks, more than TPR_TREE_MAX_FORKS = 4" in msg, msg


@pytest.mark.gpu
def test_the_points_before_the_direction_and_the_arrays(gpu):
    sc, model = _model()
    parent = _parent()
    bad_dir = _direction([[1.0, 0.0, np.nan], [0.0, 1.0, 0.0]])
    rc, msg = _call(model, parent, None, bad_dir, q=False)
    assert rc == BADARG and b"null control points" in msg and NAME.encode() in msg, msg
    for count in (0, 17, -1):
        rc, msg = _call(model, parent, _points(count=count), bad_dir, q=False)
        assert rc == BADARG and b"the point count must be in [1, TPR_CHAIN_MAX_POINTS]" in msg, msg
    for links in ((0, 3), (-1, 0)):
        rc, msg = _call(model, parent, _points(links=links), bad_dir, outputs=(False, False, False))
        assert rc == BADARG and b"a control point's link is outside the chain" in msg, msg
    rc, msg = _call(model, parent, _points(offsets=[(0.0, 0.0, 0.0), (0.0, np.inf, 0.0)]), bad_dir, q=False)
    assert rc == BADARG and b"every control point's offset must be finite" in msg, msg
    # an entry past the count is not looked at: neither a link nor a direction
    rc, msg = _call(model, parent, _points(count=1, links=(0, 9)), _direction([[1.0, 0.0, 0.0], [np.nan, 0.0, 0.0]]), q=False)
    assert rc == BADARG and b"q is required" in msg, msg


@pytest.mark.gpu
def test_the_direction_before_the_arrays(gpu):
    sc, model = _model()
    parent = _parent()
    for bad in ([[1.0, 0.0, np.nan], [0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0], [np.inf, 1.0, 0.0]]):
        rc, msg = _call(model, parent, _points(), _direction(bad), q=False, outputs=(False, False, False))
        assert rc == BADARG and b"every direction must be finite" in msg, msg


@pytest.mark.gpu
def test_the_arrays_in_their_order(gpu):
    sc, model = _model()
    parent, pts = _parent(), _points()
    unit = _direction([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    rc, msg = _call(model, parent, pts, q=False, qs=False, outputs=(False, False, False))
    assert rc == BADARG and b"q is required" in msg, msg
    # qs: needed in the velocity mode, and for speed2 or xbound in the direction mode
    for direction, outputs in ((None, (False, True, False)), (unit, (True, False, False)), (unit, (False, True, True)), (None, (False, False, False))):
        rc, msg = _call(model, parent, pts, direction, qs=False, limit=False, outputs=outputs)
        assert rc == BADARG and b"qs is required" in msg, (msg, outputs)
    rc, msg = _call(model, parent, pts, limit=False, outputs=(False, False, False))
    assert rc == BADARG and b"one of speed2, mobility, xbound is required" in msg, msg
    rc, msg = _call(model, parent, pts, unit, qs=False, limit=False, outputs=(False, False, False))
    assert rc == BADARG and b"one of speed2, mobility, xbound is required" in msg, msg
    for outputs in ((False, False, True), (True, True, True)):
        rc, msg = _call(model, parent, pts, limit=False, outputs=outputs)
        assert rc == BADARG and b"xbound needs limit" in msg, msg


@pytest.mark.gpu
def test_an_empty_batch_passes_every_check(gpu):
    """... and launches nothing: at 32 dof with 16 points, and the mobility alone along directions without qs."""
    sc, model = _model(d=32)
    pts = _points(count=16, links=tuple(range(0, 32, 2)))
    rc, msg = _call(model, _parent(32), pts, B=0)
    assert rc == 0, msg
    rc, msg = _call(model, _parent(32), pts, _direction(np.tile([0.0, 0.0, 1.0], (16, 1))), B=0, qs=False, limit=False, outputs=(False, True, False))
    assert rc == 0, msg

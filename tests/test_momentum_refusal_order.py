"""Which refusal wins when two arguments of tpr_tree_momentum_batch are bad at once, through ctypes; every case is refused, nothing
is launched, and the buffers handed over are 64 doubles long.  The order is behaviour, as tests/test_rigid_refusal_order.py pins it
for the entry's siblings: B / N; then what tpr_tree_base_wrench_batch refuses, in its order -- the links as a chain, the parent
table, the fork count, the mount --; then the link mask; then a NULL q or qs; then all outputs NULL; then xbound without limit.

The first half needs no GPU: it is what the entry decides before it looks for a device."""
import ctypes

import numpy as np
import pytest

from tests import base_wrench_cases as bw, base_wrench_ref as bwr
from tests.rigid_support import BADARG, BUF as _BUF, UNSUPPORTED, c_model as _model, parent_table as _parent

NAME = "tpr_tree_momentum_batch"


def _call(model, parent, mount=None, mask=0b111, B=1, N=1, q=True, qs=True, limit=True, outputs=(True, True, True)):
    """(code, message) of one call: ``model`` / ``parent`` / ``mount`` may be None (NULL); ``q``, ``qs``, ``limit`` False pass NULL,
    ``outputs`` says which of momentum, energy2, xbound are given."""
    from toppra_amd import _capi
    lib = _capi.load()
    p = _BUF.ctypes.data
    rc = lib.tpr_tree_momentum_batch(None if model is None else ctypes.byref(model), None if parent is None else parent.ctypes.data,
                                     None if mount is None else ctypes.byref(mount), mask, B, N, p if q else None, p if qs else None,
                                     p if limit else None, *[p if given else None for given in outputs], 0, None)
    return rc, lib.tpr_last_error()


# ---- without a GPU: what is decided before the links are looked at (check_chain looks for a device first) ------------------------

@pytest.mark.parametrize("B, N", [(-1, 1), (1, -1)])
def test_a_negative_b_or_n_is_refused_before_everything_else(B, N):
    rc, msg = _call(None, None, mask=0, B=B, N=N, q=False, outputs=(False, False, False))
    assert rc == BADARG and b"B >= 0, N >= 0" in msg and NAME.encode() in msg, msg


def test_valid_early_arguments_reach_the_device_check():
    from toppra_amd import _capi
    sc, model = _model()
    if _capi.device_count() == 0:  # (with a device the call would be valid and run)
        for mount in (None, bwr.mount_of(bw.MOUNT).c_struct()):
            rc, msg = _call(model, _parent(), mount)
            assert rc < 0 and b"tpr_init" in msg, msg
        # ... and so does a call whose later arguments are all bad: the device check comes with the links, before them
        rc, msg = _call(model, _parent(), mask=0, q=False, outputs=(False, False, False))
        assert rc < 0 and b"tpr_init" in msg, msg


# ---- with a GPU: what the checks after B / N decide; every call is refused ------------------------------------------------------

@pytest.mark.gpu
def test_the_links_are_refused_before_the_parent_table_and_the_rest(gpu):
    rc, msg = _call(None, None, mask=0, q=False)
    assert rc == BADARG and b"null chain" in msg and NAME.encode() in msg, msg
    sc, model = _model(dof=33)
    rc, msg = _call(model, None, mask=0, outputs=(False, False, False))
    assert rc == BADARG and b"the chain's dof must be in [1, TPR_MAX_DOF]" in msg, msg
    sc, model = _model(joint_type=[0, 7, 0])
    rc, msg = _call(model, None)
    assert rc == BADARG and b"unknown joint type" in msg, msg


@pytest.mark.gpu
def test_the_parent_table_and_the_fork_count_before_the_mount(gpu):
    bad_mount = bwr.mount_of(bw.MOUNT).c_struct()
    bad_mount.origin[1] = np.nan
    sc, model = _model()
    rc, msg = _call(model, None, bad_mount)
    assert rc == BADARG and b"null parent array" in msg, msg
    rc, msg = _call(model, _parent(table=[-1, 0, 2]), bad_mount, q=False)
    assert rc == BADARG and b"the parent of link 2 is 2, outside -1 .. 1" in msg, msg
    sc, model = _model(d=11)
    five = _parent(table=[-1, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4])
    rc, msg = _call(model, five, bad_mount, mask=0, outputs=(False, False, False))
    assert rc == UNSUPPORTED and b"the tree has 5 forks, more than TPR_TREE_MAX_FORKS = 4" in msg, msg


@pytest.mark.gpu
def test_the_mount_before_the_mask_and_the_mask_before_the_arrays(gpu):
    sc, model = _model()
    parent = _parent()
    mount = bwr.mount_of(bw.MOUNT).c_struct()
    mount.origin[1] = np.nan
    rc, msg = _call(model, parent, mount, mask=0, q=False)
    assert rc == BADARG and b"every entry of the mount must be finite" in msg, msg
    mount = bwr.mount_of(bw.MOUNT).c_struct()
    mount.rot[0] = 1.5
    rc, msg = _call(model, parent, mount, mask=0b1000)
    assert rc == BADARG and b"the mount's rot must be orthonormal" in msg, msg
    good = bwr.mount_of(bw.MOUNT).c_struct()
    for mount in (None, good):
        rc, msg = _call(model, parent, mount, mask=0, q=False)
        assert rc == BADARG and b"the link set is empty" in msg and NAME.encode() in msg, msg
        for mask in (0b1000, 0b1001, 1 << 31):
            rc, msg = _call(model, parent, mount, mask=mask, qs=False, outputs=(False, False, False))
            assert rc == BADARG and b"the link set names a link outside the robot" in msg, msg


@pytest.mark.gpu
def test_the_arrays_in_their_order(gpu):
    sc, model = _model()
    parent = _parent()
    for q, qs in ((False, True), (True, False)):
        rc, msg = _call(model, parent, q=q, qs=qs, outputs=(False, False, False))
        assert rc == BADARG and b"q, qs are required" in msg, msg
    rc, msg = _call(model, parent, limit=False, outputs=(False, False, False))
    assert rc == BADARG and b"one of momentum, energy2, xbound is required" in msg, msg
    for outputs in ((False, False, True), (True, True, True)):
        rc, msg = _call(model, parent, limit=False, outputs=outputs)
        assert rc == BADARG and b"xbound needs limit" in msg, msg


@pytest.mark.gpu
def test_a_mask_of_all_32_links_is_accepted_at_32_dof(gpu):
    """Bit 31 is a link of a 32-dof robot: an empty batch passes every check and launches nothing."""
    sc, model = _model(d=32)
    rc, msg = _call(model, _parent(32), mask=0xFFFFFFFF, B=0)
    assert rc == 0, msg
    rc, msg = _call(model, _parent(32), mask=1 << 31, B=0, limit=False, outputs=(False, True, False))
    assert rc == 0, msg

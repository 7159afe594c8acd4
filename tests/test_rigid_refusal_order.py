"""Which refusal wins when two arguments of a rigid-body entry are bad at once.  Every ``tpr_chain_*_batch`` /
``tpr_tree_*_batch`` entry of include/toppra_hip.h, through ctypes; every case is refused, nothing is launched, and the buffers
handed over are 64 doubles long.  The order is behaviour:

* the three control-point entries check the point set first (it needs no device), then B / N, then their pointers, then the
  chain -- so a chain of 33 dof AND null outputs is answered with "... required", where every other entry names the dof;
* the payload entries check the chain, then the payload, then their pointers;
* the tree entries check the links as a chain, then the parent table, then the fork count, then their pointers;
* the others check B / N, then the chain, then their pointers.

The first half needs no GPU: it is what an entry decides before it looks for a device."""
import ctypes

import numpy as np
import pytest

from tests.rigid_support import BADARG, BUF as _BUF, UNSUPPORTED, c_model as _model, parent_table

# name: (what follows the chain, the size arguments, inputs, outputs, the refusal of a null q, the refusal of null outputs)
ENTRIES = {
    "tpr_chain_inverse_dynamics_batch": (None, "npoints", 3, 1, b"q, qd, qdd, tau are required", b"q, qd, qdd, tau are required"),
    "tpr_chain_torque_terms_batch": (None, "BN", 3, 3, b"q, qs, qss, w0, wa, wb are required", b"q, qs, qss, w0, wa, wb are required"),
    "tpr_chain_tool_velocity_batch": (None, "BN", 4, 2, b"q, qs are required", b"one of vSv, xbound is required"),
    "tpr_chain_tool_acceleration_batch": (None, "npoints", 3, 1, b"q, qd, qdd, acc are required", b"q, qd, qdd, acc are required"),
    "tpr_chain_tool_acceleration_terms_batch": (None, "BN", 3, 2, b"q, qs, qss, wa, wb are required", b"q, qs, qss, wa, wb are required"),
    "tpr_chain_tool_wrench_batch": ("payload", "npoints", 3, 1, b"q, qd, qdd, wrench are required", b"q, qd, qdd, wrench are required"),
    "tpr_chain_tool_wrench_terms_batch": ("payload", "BN", 3, 3, b"q, qs, qss, w0, wa, wb are required", b"q, qs, qss, w0, wa, wb are required"),
    "tpr_chain_points_speed_batch": ("points", "BN", 3, 2, b"q, qs are required", b"one of speed2, xbound is required"),
    "tpr_chain_points_acceleration_batch": ("points", "npoints", 3, 1, b"q, qd, qdd, acc are required", b"q, qd, qdd, acc are required"),
    "tpr_chain_points_acceleration_terms_batch": ("points", "BN", 3, 2, b"q, qs, qss, wa, wb are required", b"q, qs, qss, wa, wb are required"),
    "tpr_tree_inverse_dynamics_batch": ("parent", "npoints", 3, 1, b"q, qd, qdd, tau are required", b"q, qd, qdd, tau are required"),
    "tpr_tree_torque_terms_batch": ("parent", "BN", 3, 3, b"q, qs, qss, w0, wa, wb are required", b"q, qs, qss, w0, wa, wb are required"),
}
NAMES = sorted(ENTRIES)
POINT_ENTRIES = [n for n in NAMES if ENTRIES[n][0] == "points"]
PAYLOAD_ENTRIES = [n for n in NAMES if ENTRIES[n][0] == "payload"]
TREE_ENTRIES = [n for n in NAMES if ENTRIES[n][0] == "parent"]
BN_FIRST_ENTRIES = [n for n in NAMES if ENTRIES[n][1] == "BN" and ENTRIES[n][0] != "points"]


def _extra(kind, sc, parent=None):
    """A valid second argument of an entry of ``kind`` on the chain ``sc``."""
    from toppra_amd.chain import ControlPoints, Payload
    if kind == "payload":
        return Payload(1.5, com=(0.0, 0.1, 0.0)).c_struct(sc)
    if kind == "points":
        return ControlPoints([0, sc.dof - 1], np.ones((2, 3))).c_struct(sc)
    if kind == "parent":
        return parent_table(sc.dof, parent)
    return None


def _call(name, model, extra, size=1, q=True, outputs=True):
    """(code, message) of one call of ``name``: ``model`` / ``extra`` may be None (NULL); ``size`` is B (with N = 1) or half of
    npoints; ``q`` False passes NULL for q, ``outputs`` False NULL for every output."""
    from toppra_amd import _capi
    lib = _capi.load()
    kind, sized, n_in, n_out = ENTRIES[name][:4]
    p = _BUF.ctypes.data
    args = [None if model is None else ctypes.byref(model)]
    if kind == "parent":
        args.append(None if extra is None else extra.ctypes.data)
    elif kind is not None:
        args.append(None if extra is None else ctypes.byref(extra))
    args += [size, 1] if sized == "BN" else [2 * size]
    args += [p if q else None] + [p] * (n_in - 1) + [p if outputs else None] * n_out + [0, None]
    rc = getattr(lib, name)(*args)
    return rc, lib.tpr_last_error()


# ---- without a GPU: what is decided before check_chain looks for a device ---------------------------------------------------

@pytest.mark.parametrize("name", POINT_ENTRIES)
def test_control_point_entries_refuse_in_their_order(name):
    sc, model = _model()
    good = _extra("points", sc)
    bad = _extra("points", sc)
    bad.count = 0
    # a bad point set and a negative B (a negative point count): the point set
    rc, msg = _call(name, model, bad, size=-1)
    assert rc == BADARG and b"the point count must be in [1, TPR_CHAIN_MAX_POINTS]" in msg, msg
    # a negative B and a null q: B / N -- the entry that takes npoints has no B to refuse (a negative count is check_chain's)
    rc, msg = _call(name, model, good, size=-1, q=False)
    assert rc == BADARG and (b"B >= 0, N >= 0" if ENTRIES[name][1] == "BN" else ENTRIES[name][4]) in msg, msg
    # a null q, and tpr_init() may not have been called: the pointers
    rc, msg = _call(name, model, good, q=False)
    assert rc == BADARG and ENTRIES[name][4] in msg, msg


@pytest.mark.parametrize("name", BN_FIRST_ENTRIES)
def test_a_negative_b_is_refused_before_a_null_chain(name):
    rc, msg = _call(name, None, None, size=-1)
    assert rc == BADARG and b"B >= 0, N >= 0" in msg and name.encode() in msg, msg


@pytest.mark.parametrize("name", NAMES)
def test_valid_early_arguments_reach_the_device_check(name):
    from toppra_amd import _capi
    sc, model = _model()
    extra = _extra(ENTRIES[name][0], sc)
    if _capi.device_count() == 0:  # (with a device the call would be valid and run)
        rc, msg = _call(name, model, extra)
        assert rc < 0 and b"tpr_init" in msg, msg


# ---- with a GPU: what check_chain and the checks after it decide; every call is refused -------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_a_null_chain_is_refused_before_a_null_q(gpu, name):
    sc, _ = _model()
    rc, msg = _call(name, None, _extra(ENTRIES[name][0], sc), q=False)
    assert rc == BADARG and b"null chain" in msg and name.encode() in msg, msg


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_a_dof_of_33_and_null_outputs(gpu, name):
    """The dof wins -- but for the control-point entries, which look at their pointers before they look at the chain."""
    sc, model = _model(dof=33)
    rc, msg = _call(name, model, _extra(ENTRIES[name][0], sc), outputs=False)
    want = ENTRIES[name][5] if name in POINT_ENTRIES else b"the chain's dof must be in [1, TPR_MAX_DOF]"
    assert rc == BADARG and want in msg and name.encode() in msg, msg


@pytest.mark.gpu
@pytest.mark.parametrize("name", PAYLOAD_ENTRIES)
def test_payload_entries_refuse_in_their_order(gpu, name):
    sc, model = _model()
    body = _extra("payload", sc)
    body.com[1] = np.nan
    rc, msg = _call(name, model, body, q=False)
    assert rc == BADARG and b"every entry of the payload must be finite" in msg, msg
    sc, model = _model(joint_type=[0, 7, 0])
    rc, msg = _call(name, model, None)
    assert rc == BADARG and b"unknown joint type" in msg, msg


@pytest.mark.gpu
@pytest.mark.parametrize("name", TREE_ENTRIES)
def test_tree_entries_refuse_in_their_order(gpu, name):
    sc, model = _model()
    rc, msg = _call(name, model, _extra("parent", sc, parent=[-1, 0, 2]), q=False)
    assert rc == BADARG and b"the parent of link 2 is 2, outside -1 .. 1" in msg, msg
    sc, model = _model(d=11)
    five = _extra("parent", sc, parent=[-1, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4])
    rc, msg = _call(name, model, five, outputs=False)
    assert rc == UNSUPPORTED and b"the tree has 5 forks, more than TPR_TREE_MAX_FORKS = 4" in msg, msg

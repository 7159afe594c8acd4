"""The batched second-order / torque constraints without a GPU: argument validation (everything is refused before a launch),
the new C-ABI entries in the header and the library, the row kernel's resources, and the numpy restatement the GPU tests
compare with (tests/second_order_ref.py) against the reference-generated fixtures."""
import os
import re
import sys

import numpy as np
import pytest

from tests import second_order_ref as ref
from tests.helpers import dense_fixtures, golden
from toppra_amd import _capi, batch
from toppra_amd.algorithm import BatchTOPPRA
from toppra_amd.constraint import BatchJointTorqueConstraint, BatchSecondOrderConstraint, DiscretizationType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tpr_path_eval_batch", "tpr_second_order_rows_batch", "tpr_second_order_block_bytes")


def _problem(B=3, d=4, N=10):
    data = batch.make_synthetic_batch(B, d, N, seed=5)
    return data, (data["coef"], data["breaks"], data["grid"], data["vlim"], data["alim"])


def _tau(q, qd, qdd):
    return qdd + q * qd


def test_defaults_are_the_reference_s():
    t = BatchJointTorqueConstraint(_tau, np.ones((4, 2)), np.zeros(4))
    s = BatchSecondOrderConstraint(_tau, np.ones((3, 4)), np.ones(3))
    j = BatchSecondOrderConstraint.joint_torque_constraint(_tau, np.ones((4, 2)), np.zeros(4))
    assert t.get_discretization_type() == DiscretizationType.Collocation
    assert s.get_discretization_type() == j.get_discretization_type() == DiscretizationType.Interpolation
    assert (t.rows_per_stage(4), s.rows_per_stage(4), j.rows_per_stage(4)) == (8, 6, 16)
    assert "custom_term" in BatchSecondOrderConstraint.__doc__


def test_row_limit_is_refused_at_construction():
    """2 + 4 d + 2 * (2 * 2 d) = 122 at d = 10 passes; one more constraint names the count."""
    data, args = _problem(d=10)
    lim = np.stack([-np.ones((3, 10)), np.ones((3, 10))], -1)
    two = [BatchSecondOrderConstraint.joint_torque_constraint(_tau, lim, np.zeros(10)) for _ in range(2)]
    BatchTOPPRA(*args, constraints=two)
    with pytest.raises(NotImplementedError, match="142"):
        BatchTOPPRA(*args, constraints=two + [BatchJointTorqueConstraint(_tau, lim, np.zeros(10))])
    with pytest.raises(NotImplementedError, match="%d" % _capi.SO_MAX_BLOCKS):
        BatchTOPPRA(data["coef"], data["breaks"], data["grid"], None, None,
                    constraints=[BatchSecondOrderConstraint(_tau, np.ones((1, 10)), np.ones(1)) for _ in range(9)])
    # the array-level call refuses the same count, before it asks for a device
    w = np.zeros((3, 11, 10))
    blk = dict(w0=w, wa=w, wb=w, F=None, g=np.ones(20), friction=None, interpolation=True)
    with pytest.raises(NotImplementedError, match="162"):
        batch.second_order_rows_batch(*args, [blk] * 3)


def test_limit_shapes():
    data, args = _problem()
    with pytest.raises(ValueError):
        BatchJointTorqueConstraint(_tau, np.ones((4, 3)), np.zeros(4))
    with pytest.raises(ValueError):
        BatchJointTorqueConstraint(_tau, np.ones((4, 2)), np.zeros(5))
    with pytest.raises(ValueError):
        BatchSecondOrderConstraint.joint_torque_constraint(_tau, np.ones(4), np.zeros(4))
    with pytest.raises(ValueError):
        BatchSecondOrderConstraint(_tau, np.ones(4), np.ones(4))
    with pytest.raises(ValueError):
        BatchSecondOrderConstraint(_tau, np.ones((3, 4)), np.ones(5))
    with pytest.raises(ValueError, match="dof"):
        BatchTOPPRA(*args, constraints=[BatchJointTorqueConstraint(_tau, np.ones((5, 2)), np.zeros(5))])
    with pytest.raises(ValueError, match="per trajectory"):
        BatchTOPPRA(*args, constraints=[BatchJointTorqueConstraint(_tau, np.ones((7, 4, 2)), np.zeros(4))])
    with pytest.raises(ValueError, match="leading shape"):
        BatchTOPPRA(*args, constraints=[BatchSecondOrderConstraint(_tau, np.ones((2, 3, 4)), np.ones(3))])
    with pytest.raises(ValueError, match="friction"):
        BatchTOPPRA(*args, constraints=[BatchSecondOrderConstraint(_tau, np.ones((3, 4)), np.ones(3), friction=np.zeros(6))])
    with pytest.raises(NotImplementedError):
        BatchTOPPRA(*args, constraints=[object()])
    assert BatchTOPPRA(*args).constraints == []  # nothing changes without the argument


def test_callback_contract():
    """Three calls with [B, N+1, d] arrays; a wrong output shape is a ValueError before the row launch."""
    B, N, d = 3, 10, 4
    q = np.random.default_rng(0).standard_normal((B, N + 1, d))
    calls = []

    def tau(q_, qd, qdd):
        calls.append((q_.shape, bool(np.any(qd)), bool(np.any(qdd))))
        return qdd + q_ * qd

    blk = BatchJointTorqueConstraint(tau, np.ones((d, 2)), np.zeros(d)).block(q, q + 1, q + 2)
    assert calls == [((B, N + 1, d), False, False), ((B, N + 1, d), False, True), ((B, N + 1, d), True, True)]
    assert blk["F"] is None and blk["g"].shape == (2 * d,) and blk["friction"].shape == (B, d) and not blk["interpolation"]
    for bad in (lambda q_, qd, qdd: qdd[0], lambda q_, qd, qdd: qdd[:, 1:], lambda q_, qd, qdd: qdd[:, :, :3]):
        with pytest.raises(ValueError):
            BatchJointTorqueConstraint(bad, np.ones((d, 2)), np.zeros(d)).block(q, q, q)
    with pytest.raises(ValueError, match="columns"):
        BatchSecondOrderConstraint(lambda q_, qd, qdd: qdd[:, :, :3], np.ones((5, 4)), np.ones(5)).block(q, q, q)
    with pytest.raises(ValueError, match="callback"):
        BatchSecondOrderConstraint(tau, lambda q_: np.ones((5, 4)), np.ones(5)).block(q, q, q)
    with pytest.raises(ValueError, match="p == d"):
        BatchSecondOrderConstraint(lambda q_, qd, qdd: qdd[:, :, :3], np.ones((5, 3)), np.ones(5), friction=np.zeros(d)).block(q, q, q)
    # array-level shape checks
    data, args = _problem(B, d, N)
    w = np.zeros((B, N + 1, d))
    for wrong in (dict(w0=w[:, :-1]), dict(g=np.ones(7)), dict(F=np.ones((5, 3)), g=np.ones(5)), dict(friction=np.zeros((B, d + 1)))):
        blk = dict(w0=w, wa=w, wb=w, F=None, g=np.ones(2 * d), friction=None, interpolation=True)
        blk.update(wrong)
        with pytest.raises(ValueError):
            batch.second_order_rows_batch(*args, [blk])


def test_header_declares_and_library_exports_the_new_entries():
    from toppra_amd import build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "toppra_hip.h")).read()
    lib = _capi.load()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr) and name in _capi.EXPORTS and hasattr(lib, name), name
    for cite in ("linear_second_order.py:142-173", "joint_torque.py", "linear_constraint.py:84-192", "cy_seidel_solverwrapper.pyx:455-520"):
        assert cite in hdr, cite
    body = hdr[hdr.index("typedef struct tpr_second_order_block {"):hdr.index("} tpr_second_order_block;")]
    order = [body.index(n) for n in ("p, m, flags, reserved", "*w0, *wa, *wb", "*F, *g", "*friction")]
    assert order == sorted(order)
    import ctypes
    assert ctypes.sizeof(_capi.tpr_second_order_block) == 4 * 4 + 6 * 8
    # ... and the C side agrees (the library's own sizeof; _capi.load() refuses a mismatch)
    assert lib.tpr_second_order_block_bytes() == ctypes.sizeof(_capi.tpr_second_order_block)
    for flag, name in ((_capi.SO_INTERPOLATION, "TPR_SO_INTERPOLATION"), (_capi.SO_F_SHARED, "TPR_SO_F_SHARED"),
                       (_capi.SO_F_PER_TRAJ, "TPR_SO_F_PER_TRAJ"), (_capi.SO_F_PER_POINT, "TPR_SO_F_PER_POINT"),
                       (_capi.SO_G_PER_TRAJ, "TPR_SO_G_PER_TRAJ"), (_capi.SO_G_PER_POINT, "TPR_SO_G_PER_POINT"),
                       (_capi.SO_MAX_BLOCKS, "TPR_SO_MAX_BLOCKS")):
        assert re.search(r"#define %s %d\b" % (name, flag), hdr), name
    # no device: the entries refuse to compute
    if _capi.device_count() == 0:
        data, args = _problem()
        with pytest.raises(_capi.ToppraHipError):
            batch.path_eval_batch(*args[:3])


def test_row_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as kr
    from toppra_amd import build
    build.build()
    ks = {n: r for n, r in kr.kernels().items() if "second_order_rows_kernel" in n or "path_eval_kernel" in n}
    assert len(ks) == 2, sorted(ks)
    for name, r in ks.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)  # four waves per SIMD and more


@pytest.mark.parametrize("name", dense_fixtures() + ["dense_reuse_d5_N60"])
def test_the_restatement_reproduces_the_reference_s_rows(name):
    """tests/second_order_ref.py, the yardstick of the GPU tests at sizes no fixture covers, on the five reference-generated
    fixtures: a, b, c, low, high bit for bit."""
    fx = golden(name)
    kinds, interp = str(fx["kinds"]).split(","), bool(int(fx["scheme"]))
    coef, breaks = batch.spline_coefficients(fx["knots"], fx["way"])
    vlim = np.stack([-fx["vmax"], fx["vmax"]], -1) if "vel" in kinds else None
    alim = np.stack([-fx["amax"], fx["amax"]], -1) if "acc" in kinds else None
    q, qs, qss = ref.path_samples(coef, breaks, fx["grid"])
    model = ref.batched_torque_model(fx["mass"], fx["grav"], fx["cori"])
    z = np.zeros_like(q)
    blocks = [dict(w0=model(q, z, z), wa=model(q, z, qs), wb=model(q, qs, qss), F=None, g=np.concatenate((fx["taumax"], fx["taumax"]), -1),
                   friction=fx["fric"], interpolation=interp) for k in kinds if k in ("torque", "second")]
    out = ref.dense_problem(coef, breaks, fx["grid"], vlim, alim, interp, blocks)
    for k in ("a", "b", "c", "low", "high"):
        assert np.array_equal(out[k], fx[k]), k

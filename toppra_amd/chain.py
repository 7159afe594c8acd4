"""A serial rigid-body chain evaluated on the GPU: the robot model behind a batch's torque and tool-speed limits.

The reference's Python side leaves the robot to the caller (``JointTorqueConstraint`` takes an ``inv_dyn`` callback); its C++
twin evaluates a pinocchio model (constraint/joint_torque/pinocchio.hpp, constraint/cartesian_velocity_norm/pinocchio.hpp).
:class:`SerialChain` is that piece here: one model for the whole batch, evaluated by the chain kernels at every gridpoint
of every trajectory (include/toppra_hip.h: ``tpr_chain``).
"""
import numpy as np

from . import _capi
from . import batch as _batch

REVOLUTE, PRISMATIC = "revolute", "prismatic"
_JOINT_CODES = {REVOLUTE: _capi.JOINT_REVOLUTE, "r": _capi.JOINT_REVOLUTE, _capi.JOINT_REVOLUTE: _capi.JOINT_REVOLUTE,
                PRISMATIC: _capi.JOINT_PRISMATIC, "p": _capi.JOINT_PRISMATIC, _capi.JOINT_PRISMATIC: _capi.JOINT_PRISMATIC}


class SerialChain(object):
    """A fixed-base serial chain of 1 .. 32 revolute / prismatic joints.

    Links are i = 0 .. d-1; the parent of link i is link i-1, the parent of link 0 the fixed base (the world frame).

    Parameters
    ----------
    joint_types : d entries, "revolute" / "prismatic" (or "r" / "p", or 0 / 1).
    axes : [d, 3] unit vectors in the joint frames: a revolute joint rotates by q_i about its axis (Rodrigues' formula), a
        prismatic one translates by q_i * axis.  The link frame is the joint frame after that motion.
    rotations : [d, 3, 3], translations : [d, 3] -- joint i in its parent's frame: the columns of the rotation are the joint
        frame's axes in parent coordinates, the translation is its origin there.
    masses : [d] (>= 0), coms : [d, 3] centres of mass in the link frames, inertias : [d, 6] = xx, yy, zz, xy, xz, yz about
        the centre of mass in link-frame axes (or [d, 3, 3] symmetric).
    gravity : gravitational acceleration in the world frame (applied as a base acceleration of -gravity).
    tool : a point in the last link's frame (:meth:`tool_velocity_norm`, :meth:`tool_acceleration`).

    Not modelled: rotor inertia, viscous damping, branched trees, floating bases; dry friction stays with the constraints
    (``fs_coef`` / ``friction``).  The model is uploaded to a device once per object, on first use there.
    """

    def __init__(self, joint_types, axes, rotations, translations, masses, coms, inertias, gravity=(0.0, 0.0, -9.81),
                 tool=(0.0, 0.0, 0.0)):
        try:
            codes = [_JOINT_CODES[t.lower() if isinstance(t, str) else int(t)] for t in joint_types]
        except (KeyError, TypeError, ValueError):
            raise ValueError("joint_types must hold 'revolute' / 'prismatic' (or 'r' / 'p', 0 / 1), got %r" % (joint_types,))
        d = len(codes)
        if not 1 <= d <= _capi.MAX_DOF:
            raise ValueError("a chain has 1..%d joints, got %d" % (_capi.MAX_DOF, d))
        arr = {"axis": axes, "rot": rotations, "trans": translations, "mass": masses, "com": coms, "inertia": inertias,
               "gravity": gravity, "tool": tool}
        for name in arr:
            try:
                arr[name] = np.array(arr[name], dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("%s is not an array of numbers" % name)
        if arr["inertia"].shape == (d, 3, 3):
            full = arr["inertia"]
            if not np.array_equal(full, np.swapaxes(full, 1, 2)):
                raise ValueError("inertia matrices must be symmetric")
            arr["inertia"] = np.stack([full[:, 0, 0], full[:, 1, 1], full[:, 2, 2], full[:, 0, 1], full[:, 0, 2], full[:, 1, 2]], -1)
        want = {"axis": (d, 3), "rot": (d, 3, 3), "trans": (d, 3), "mass": (d,), "com": (d, 3), "inertia": (d, 6),
                "gravity": (3,), "tool": (3,)}
        for name, shape in want.items():
            if arr[name].shape != shape:
                raise ValueError("%s must have shape %s for %d joints, got %s" % (name, list(shape), d, list(arr[name].shape)))
            if not np.all(np.isfinite(arr[name])):
                raise ValueError("%s holds a value that is not finite" % name)
        if np.any(np.abs(np.sqrt((arr["axis"] ** 2).sum(-1)) - 1.0) > 1e-12):
            raise ValueError("axes must be unit vectors (to 1e-12)")
        rot = arr["rot"]
        if np.any(np.abs(np.swapaxes(rot, 1, 2) @ rot - np.eye(3)) > 1e-12) or np.any(np.abs(np.linalg.det(rot) - 1.0) > 1e-12):
            raise ValueError("rotations must be orthonormal with determinant +1 (to 1e-12)")
        if np.any(arr["mass"] < 0):
            raise ValueError("masses must be >= 0")
        self.dof = d
        self.joint_types = [PRISMATIC if c == _capi.JOINT_PRISMATIC else REVOLUTE for c in codes]
        self._codes = np.array(codes, dtype=np.int32)
        # one packed buffer: a single upload per device, the struct's pointers are offsets into it
        self._offsets, parts, at = {}, [], 0
        for name, _ in _capi.CHAIN_ARRAYS:
            self._offsets[name] = at
            parts.append(arr[name].ravel())
            at += parts[-1].size
        self._host = np.ascontiguousarray(np.concatenate(parts))
        for name in arr:
            view = self._host[self._offsets[name]:self._offsets[name] + arr[name].size].reshape(arr[name].shape)
            view.flags.writeable = False
            setattr(self, {"axis": "axes", "rot": "rotations", "trans": "translations", "mass": "masses", "com": "coms",
                           "inertia": "inertias"}.get(name, name), view)
        self._device = {}  # torch device -> the packed buffer there

    def __repr__(self):
        return "SerialChain(%d dof: %s)" % (self.dof, "".join("P" if t == PRISMATIC else "R" for t in self.joint_types))

    def c_struct(self, like):
        """(tpr_chain, what it points to) for a call whose arrays are of the kind of ``like``: host pointers for numpy, the
        model's copy on like's device otherwise (made on first use).  The joint types are a host array in both cases."""
        if _capi.is_torch_cuda(like):
            buf = self._device.get(like.device)
            if buf is None:
                import torch
                buf = self._device[like.device] = torch.from_numpy(self._host).to(like.device)
            base = buf.data_ptr()
        else:
            buf, base = self._host, self._host.ctypes.data
        model = _capi.tpr_chain(d=self.dof, flags=0, joint_type=self._codes.ctypes.data)
        for name, _ in _capi.CHAIN_ARRAYS:
            setattr(model, name, base + 8 * self._offsets[name])
        return model, (buf, self._codes)

    def inverse_dynamics(self, q, qd, qdd):
        """Joint torques / forces tau(q, qd, qdd) by recursive Newton-Euler: arrays [..., d] in, [..., d] out (numpy in ->
        numpy out, torch-ROCm tensors in -> a tensor out on the current stream).  A valid ``inv_dyn`` callback of the
        torque constraints."""
        return _batch.chain_inverse_dynamics_batch(self, q, qd, qdd)

    def torque_terms(self, q, qs, qss):
        """(tau(q, 0, 0), tau(q, 0, qs), tau(q, qs, qss)) in one launch: the three evaluations a torque constraint needs."""
        return _batch.chain_torque_terms_batch(self, q, qs, qss)

    def tool_velocity_norm(self, q, qs, S=None):
        """v' S v of the tool point for qd = qs, shape [...]: [v; w] are its linear and angular velocity in world axes, ``S``
        [6, 6] (None: the linear part only, i.e. the squared tool speed per unit of path velocity)."""
        return _batch.chain_tool_bound_batch(self, q, qs, None, S)

    def tool_acceleration(self, q, qd, qdd):
        """The tool point's acceleration [..., 6] = [linear; angular] in world axes: the classical acceleration of the point
        (the second time derivative of its world position) and the last link's angular acceleration.  Kinematics only: gravity
        does not enter.  A valid batched ``inv_dyn`` of :class:`toppra_amd.constraint.BatchSecondOrderConstraint` (p = 6)."""
        return _batch.chain_tool_acceleration_batch(self, q, qd, qdd)

    def tool_acceleration_terms(self, q, qs, qss):
        """(acc(q, 0, qs), acc(q, qs, qss)) in one launch: the evaluations a limit on the tool acceleration needs; acc(q, 0, 0)
        is an exact zero."""
        return _batch.chain_tool_acceleration_terms_batch(self, q, qs, qss)

"""A serial rigid-body chain, or a branched tree of links, evaluated on the GPU: the robot model behind a batch's torque and
tool-speed limits.

The reference's Python side leaves the robot to the caller (``JointTorqueConstraint`` takes an ``inv_dyn`` callback); its C++
twin evaluates a pinocchio model (constraint/joint_torque/pinocchio.hpp, constraint/cartesian_velocity_norm/pinocchio.hpp).
:class:`SerialChain` is that piece here: one model for the whole batch, evaluated by the chain kernels at every gridpoint
of every trajectory (include/toppra_hip.h: ``tpr_chain``).  :class:`KinematicTree` is the same model with a parent table: two
arms on a torso, an arm beside a pan-tilt head, several robots on one base (``tpr_tree_*``).
"""
import numpy as np

from . import _capi
from . import batch as _batch
from . import contact as _contact

REVOLUTE, PRISMATIC = "revolute", "prismatic"
_JOINT_CODES = {REVOLUTE: _capi.JOINT_REVOLUTE, "r": _capi.JOINT_REVOLUTE, _capi.JOINT_REVOLUTE: _capi.JOINT_REVOLUTE,
                PRISMATIC: _capi.JOINT_PRISMATIC, "p": _capi.JOINT_PRISMATIC, _capi.JOINT_PRISMATIC: _capi.JOINT_PRISMATIC}


def _inertia6(value, name):
    """An inertia given as [6] = xx, yy, zz, xy, xz, yz or as a symmetric [3, 3], as [6]."""
    value = np.array(value, dtype=np.float64)
    if value.shape == (3, 3):
        if not np.array_equal(value, value.T):
            raise ValueError("%s must be symmetric" % name)
        value = np.array([value[0, 0], value[1, 1], value[2, 2], value[0, 1], value[0, 2], value[1, 2]])
    return value


def _inertia33(I):
    return np.array([[I[0], I[3], I[4]], [I[3], I[1], I[5]], [I[4], I[5], I[2]]])


def _arrays(values, want, infix="", words=None, convert=None, fold=None):
    """``values`` (name -> what was given) as finite float64 arrays of the shapes ``want`` (name -> shape): {name: array}, a
    ValueError that names the argument otherwise.  Every value is converted before any shape is looked at, then each is checked
    for its shape and its content in the order of ``want``.  ``infix`` goes after the wanted shape in the message and ``words``
    (name -> text) in that shape's place; ``convert`` (name -> f(value, name)) stands in for ``np.array`` and its "symmetric"
    refusal passes through; ``fold(arrays)`` runs between the two passes."""
    arr = dict(values)
    for name in arr:
        special = (convert or {}).get(name)
        try:
            arr[name] = np.array(arr[name], dtype=np.float64) if special is None else special(arr[name], name)
        except (TypeError, ValueError) as exc:
            if "symmetric" in str(exc):
                raise
            raise ValueError("%s is not an array of numbers" % name)
    if fold is not None:
        fold(arr)
    for name, shape in want.items():
        if name not in arr:
            continue
        if arr[name].shape != tuple(shape):
            raise ValueError("%s must have shape %s%s, got %s" % (name, (words or {}).get(name, list(shape)), infix, list(arr[name].shape)))
        if not np.all(np.isfinite(arr[name])):
            raise ValueError("%s holds a value that is not finite" % name)
    return arr


def _need_rotation(rot, name):
    """ValueError unless ``rot`` -- [3, 3], or a stack [K, 3, 3] -- is orthonormal with determinant +1 (to 1e-12)."""
    if np.any(np.abs(np.swapaxes(rot, -1, -2) @ rot - np.eye(3)) > 1e-12) or np.any(np.abs(np.linalg.det(rot) - 1.0) > 1e-12):
        raise ValueError("%s must be orthonormal with determinant +1 (to 1e-12)" % name)


def _with_payload_on(masses, coms, inertias, link, payload):
    """Copies of (masses, coms, inertias) with ``payload`` (a :class:`Payload` fixed in the frame of ``link``) merged into that
    link's mass, centre of mass and inertia (parallel-axis theorem)."""
    masses, coms, inertias = masses.copy(), coms.copy(), inertias.copy()
    ml, cl, mp, cp = masses[link], coms[link].copy(), payload.mass, payload.com
    total = ml + mp
    if mp > 0:
        cm = (ml * cl + mp * cp) / total
        merged = np.zeros((3, 3))
        for m, c, I in ((ml, cl, inertias[link]), (mp, cp, payload.inertia)):
            r = c - cm
            merged += _inertia33(I) + m * (np.dot(r, r) * np.eye(3) - np.outer(r, r))
        masses[link], coms[link], inertias[link] = total, cm, _inertia6(merged, "inertia")
    else:  # nothing moves the centre of mass
        inertias[link] = inertias[link] + payload.inertia
    return masses, coms, inertias


class Payload(object):
    """A carried object: a rigid body fixed to a chain's last link, and the contact frame its wrench is reported in.

    Parameters
    ----------
    mass : >= 0.
    com : [3] the centre of mass in the last link's frame.
    inertia : [6] = xx, yy, zz, xy, xz, yz about ``com`` in link-frame axes (the chain's convention), or [3, 3] symmetric;
        None = zeros (a point mass).
    frame_rotation : [3, 3], columns = the contact frame's axes in last-link coordinates (orthonormal, determinant +1, to
        1e-12); None = identity.
    frame_origin : [3] the contact frame's origin in the last link's frame; None = the chain's ``tool`` at use.
    """

    def __init__(self, mass, com=(0.0, 0.0, 0.0), inertia=None, frame_rotation=None, frame_origin=None):
        arr = {"mass": mass, "com": com, "inertia": np.zeros(6) if inertia is None else inertia,
               "frame_rotation": np.eye(3) if frame_rotation is None else frame_rotation}
        if frame_origin is not None:
            arr["frame_origin"] = frame_origin
        arr = _arrays(arr, {"mass": (), "com": (3,), "inertia": (6,), "frame_rotation": (3, 3), "frame_origin": (3,)},
                      convert={"inertia": _inertia6})
        if arr["mass"] < 0:
            raise ValueError("mass must be >= 0")
        _need_rotation(arr["frame_rotation"], "frame_rotation")
        self.mass = float(arr["mass"])
        self.com, self.inertia, self.frame_rotation = arr["com"], arr["inertia"], arr["frame_rotation"]
        self.frame_origin = arr.get("frame_origin")
        for value in (self.com, self.inertia, self.frame_rotation, self.frame_origin):
            if value is not None:
                value.flags.writeable = False

    def __repr__(self):
        return "Payload(mass=%g)" % self.mass

    def origin(self, chain):
        """The contact frame's origin in the last link's frame: ``frame_origin``, or ``chain``'s tool point."""
        return np.asarray(chain.tool if self.frame_origin is None else self.frame_origin, dtype=np.float64)

    def c_struct(self, chain):
        """The tpr_payload of a call on ``chain`` (a host struct, passed to the kernels by value)."""
        body = _capi.tpr_payload(mass=self.mass)
        body.com[:] = self.com.tolist()
        body.inertia[:] = self.inertia.tolist()
        body.rot[:] = self.frame_rotation.ravel().tolist()
        body.origin[:] = self.origin(chain).tolist()
        return body


class Mount(object):
    """What a robot is bolted to or stands on: the frame its base reaction is reported in, and an optional rigid platform.

    Parameters
    ----------
    rotation : [3, 3], columns = the mount frame's axes in base coordinates (orthonormal, determinant +1, to 1e-12); None =
        identity.
    origin : [3] the mount frame's origin in base coordinates: the point the moment is taken about.
    mass : >= 0, com : [3] -- a rigid platform fixed to the base (the cart or column whose weight keeps a mobile manipulator
        upright): its mass and its centre of mass in base coordinates.  It adds ``-mass * gravity`` at ``com`` to every
        evaluation.

    The default is the base frame itself without a platform.
    """

    def __init__(self, rotation=None, origin=(0.0, 0.0, 0.0), mass=0.0, com=(0.0, 0.0, 0.0)):
        arr = _arrays({"rotation": np.eye(3) if rotation is None else rotation, "origin": origin, "mass": mass, "com": com},
                      {"rotation": (3, 3), "origin": (3,), "mass": (), "com": (3,)})
        if arr["mass"] < 0:
            raise ValueError("mass must be >= 0")
        _need_rotation(arr["rotation"], "rotation")
        self.mass = float(arr["mass"])
        self.rotation, self.origin, self.com = arr["rotation"], arr["origin"], arr["com"]
        for value in (self.rotation, self.origin, self.com):
            value.flags.writeable = False

    def __repr__(self):
        return "Mount(origin=%s, mass=%g)" % (self.origin.tolist(), self.mass)

    def c_struct(self, robot=None):
        """The tpr_mount of a call (a host struct, passed to the kernels by value); the same for every robot."""
        frame = _capi.tpr_mount(mass=self.mass)
        frame.rot[:] = self.rotation.ravel().tolist()
        frame.origin[:] = self.origin.tolist()
        frame.com[:] = self.com.tolist()
        return frame


class _LinkSet(object):
    """What :class:`ControlPoints` and :class:`JointSections` share: K entries, each fixed to a link of a robot that is named only
    where the set is used -- the index checks of the constructor, the length, the resolution of -1 and read-only storage.  A
    subclass names its index argument (``_index``, also the attribute), its cap, and its words: the letter of its count, what it
    is a set of, and its refusal of a link outside the robot."""
    _index = _cap = _letter = _holds = _sits = None

    def _indices(self, given):
        """``given`` as the integer array [K] of the set, 1 <= K <= the cap (the range waits for :meth:`_store`)."""
        try:
            raw = np.array(given)
        except (TypeError, ValueError):
            raise ValueError("%s is not an array of integers" % self._index)
        if raw.ndim != 1 or not 1 <= raw.shape[0] <= self._cap:
            raise ValueError("a %s: %s must have shape [%s], got %s"
                             % (self._holds % self._cap, self._index, self._letter, list(raw.shape)))
        if raw.dtype.kind not in "iu":
            raise ValueError("%s must hold integers (link indices 0 .. d-1, or -1 for the last link), got %r" % (self._index, given))
        return raw

    def _store(self, raw, **payload):
        """Keeps the indices (-1 .. MAX_DOF-1, as int32) and the checked per-entry arrays ``payload``, all read-only."""
        if np.any(raw.astype(np.int64) < -1) or np.any(raw.astype(np.int64) >= _capi.MAX_DOF):
            raise ValueError("%s must lie in -1 .. %d, got %r" % (self._index, _capi.MAX_DOF - 1, raw.tolist()))
        self.count = int(raw.shape[0])
        for name, value in dict(payload, **{self._index: raw.astype(np.int32)}).items():
            value.flags.writeable = False
            setattr(self, name, value)

    def __len__(self):
        return self.count

    def _on(self, robot):
        links = getattr(self, self._index)
        links = np.where(links < 0, robot.dof - 1, links).astype(np.int32)
        if np.any(links >= robot.dof):
            raise ValueError(self._sits % (int(links.max()), robot.dof - 1))
        return links


class ControlPoints(_LinkSet):
    """Points fixed to ANY links of a chain -- an elbow, a camera bracket, a cable carrier: what the whole-arm speed and
    acceleration limits are set on.

    Parameters
    ----------
    links : [P] integers, the link (0 .. d-1) in whose frame each point is fixed; -1 = the chain's last link.  Several points
        may sit on one link.
    offsets : [P, 3] the points in their links' frames.

    P is 1 .. 16 (several sets may be used side by side).  The given order is the order of every output.  The links are checked
    against a chain where the set is used with one (:meth:`c_struct`).
    """
    _index, _cap, _letter = "links", _capi.CHAIN_MAX_POINTS, "P"
    _holds, _sits = "control-point set holds 1..%d points", "a control point sits on link %d, the chain has links 0..%d"

    def __init__(self, links, offsets):
        raw = self._indices(links)
        P = raw.shape[0]
        self._store(raw, **_arrays({"offsets": offsets}, {"offsets": (P, 3)}, words={"offsets": "[P, 3] = [%d, 3]" % P}))

    def __repr__(self):
        return "ControlPoints(%d points on links %s)" % (self.count, self.links.tolist())

    def on(self, chain):
        """The link of every point on ``chain`` ([P], -1 resolved to its last link); ValueError for a link outside it."""
        return self._on(chain)

    def c_struct(self, chain):
        """The tpr_chain_points of a call on ``chain`` (a host struct, passed to the kernels by value)."""
        pts = _capi.tpr_chain_points(count=self.count)
        pts.link[:self.count] = self.on(chain).tolist()
        for p in range(self.count):
            pts.offset[p][:] = self.offsets[p].tolist()
        return pts


class JointSections(_LinkSet):
    """Cuts across joints of a robot -- a gearbox's output bearing, a linear guide's carriage, a slender link's flange: where the
    joint-load limits are set (:class:`toppra_amd.constraint.BatchJointLoadConstraint`).

    Parameters
    ----------
    joints : [S] integers, the joint / link (0 .. d-1) each section cuts; -1 = the robot's last link.  Several sections may sit on
        one joint.
    origins : [S, 3] the point the moment is taken about, in the frame of the joint's link; None = the link's origin.
    rotations : [S, 3, 3], columns = the section frame's axes in link coordinates (orthonormal, determinant +1, to 1e-12);
        None = the link's axes.

    A section reports the wrench the parent side exerts ON its link through the joint -- the force and its moment about the
    section's origin, in the section's axes; the frame moves with the link.  S is 1 .. 8 (several sets may be used side by side).
    The given order is the order of every output.  The links are checked against a robot where the set is used with one
    (:meth:`on`, :meth:`c_struct`).  :meth:`on_axes` builds sections along joint axes.
    """
    _index, _cap, _letter = "joints", _capi.JOINT_MAX_SECTIONS, "S"
    _holds, _sits = "section set holds 1..%d sections", "a section sits on joint %d, the robot has joints 0..%d"

    def __init__(self, joints, origins=None, rotations=None):
        raw = self._indices(joints)
        S = int(raw.shape[0])
        arr = _arrays({"origins": np.zeros((S, 3)) if origins is None else origins,
                       "rotations": np.broadcast_to(np.eye(3), (S, 3, 3)) if rotations is None else rotations},
                      {"origins": (S, 3), "rotations": (S, 3, 3)})
        _need_rotation(arr["rotations"], "rotations")
        self._store(raw, **arr)

    def __repr__(self):
        return "JointSections(%d sections on joints %s)" % (self.count, self.joints.tolist())

    @classmethod
    def on_axes(cls, robot, joints, offsets=0.0):
        """Sections whose z-axis is each joint's axis and whose origin is ``axis * offset`` -- a bearing's centre along the axis
        (``offsets``: a scalar or [S]).  x and y are a fixed perpendicular pair: with e the coordinate axis of the smallest
        |axis_k| (the lowest index on ties), x = normalize(e - (e . a) a), y = a x x."""
        try:
            raw = np.array(joints)
            off = np.array(offsets, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("joints is not an array of integers, or offsets not one of numbers")
        if raw.ndim != 1 or raw.dtype.kind not in "iu" or raw.shape[0] < 1:
            raise ValueError("joints must be an integer array [S], got %r" % (joints,))
        if off.shape not in ((), (raw.shape[0],)) or not np.all(np.isfinite(off)):
            raise ValueError("offsets must be a finite scalar or have shape [S] = [%d], got %s" % (raw.shape[0], list(off.shape)))
        links = np.where(raw < 0, robot.dof - 1, raw)
        if np.any(links < 0) or np.any(links >= robot.dof):
            raise ValueError("a section sits on joint %d, the robot has joints 0..%d" % (int(links.max()), robot.dof - 1))
        off = np.broadcast_to(off, raw.shape)
        rot, org = np.empty((len(links), 3, 3)), np.empty((len(links), 3))
        for k, i in enumerate(links.tolist()):
            a = np.asarray(robot.axes[i], dtype=np.float64)
            e = np.zeros(3)
            e[int(np.argmin(np.abs(a)))] = 1.0
            x = e - np.dot(e, a) * a
            x = x / np.sqrt(np.dot(x, x))
            rot[k] = np.stack([x, np.cross(a, x), a], -1)
            org[k] = a * off[k]
        return cls(raw, origins=org, rotations=rot)

    def on(self, robot):
        """The link of every section on ``robot`` ([S], -1 resolved to its last link); ValueError for a link outside it."""
        return self._on(robot)

    def c_struct(self, robot):
        """The tpr_joint_sections of a call on ``robot`` (a host struct, passed to the kernels by value)."""
        sec = _capi.tpr_joint_sections(count=self.count)
        sec.link[:self.count] = self.on(robot).tolist()
        for k in range(self.count):
            sec.rot[k][:] = self.rotations[k].ravel().tolist()
            sec.origin[k][:] = self.origins[k].tolist()
        return sec


class _Robot(object):
    """What :class:`SerialChain` and :class:`KinematicTree` share: the evaluations that walk any robot as a tree -- base reaction,
    momentum, joint loads -- and the joint torques, which each class takes from the entries of its own family (``_family``)."""
    _family = None  # "chain" / "tree": the prefix of toppra_amd.batch's torque functions

    def as_tree(self, like):
        """(tpr_chain of the links, the host parent array [d] int32, what they point to): how the robot presents itself to the
        tree-walking entries, for a call whose arrays are of the kind of ``like`` (see :meth:`SerialChain.c_struct`).  A tree's
        ``c_struct`` is that; a chain adds its parent table -1, 0, 1, ..."""
        return self.c_struct(like)

    def inverse_dynamics(self, q, qd, qdd):
        """Joint torques / forces tau(q, qd, qdd) by recursive Newton-Euler: arrays [..., d] in, [..., d] out (numpy in ->
        numpy out, torch-ROCm tensors in -> a tensor out on the current stream).  A valid ``inv_dyn`` callback of the
        torque constraints."""
        return getattr(_batch, self._family + "_inverse_dynamics_batch")(self, q, qd, qdd)

    def torque_terms(self, q, qs, qss):
        """(tau(q, 0, 0), tau(q, 0, qs), tau(q, qs, qss)) in one launch: the three evaluations a torque constraint needs."""
        return getattr(_batch, self._family + "_torque_terms_batch")(self, q, qs, qss)

    def base_wrench(self, q, qd, qdd, mount=None):
        """The base reaction [..., 6] = [force; moment]: the wrench the mount exerts ON the robot, summed over every link,
        gravity included -- at rest the force holds up the weight.  ``mount`` (a :class:`Mount`, None = the base frame, no
        platform) gives the frame: the moment is about its origin, both parts are in its axes.  With the mount bound
        (``lambda q, qd, qdd: robot.base_wrench(q, qd, qdd, mount)``) a valid batched ``inv_dyn`` of
        :class:`toppra_amd.constraint.BatchSecondOrderConstraint` (p = 6)."""
        return _batch.base_wrench_batch(self, q, qd, qdd, mount)

    def base_wrench_terms(self, q, qs, qss, mount=None):
        """(w(q, 0, 0), w(q, 0, qs), w(q, qs, qss)) of :meth:`base_wrench` in one launch: the evaluations a limit on the base
        reaction needs; the first is the static reaction, which gravity keeps from being zero."""
        return _batch.base_wrench_terms_batch(self, q, qs, qss, mount)

    def momentum(self, q, qd, mount=None, links=None):
        """The momentum [..., 6] = [linear; angular] the robot carries at velocity ``qd``: the sum over the links of ``links`` (an
        iterable of link numbers, -1 = the last; None = every link) of each link's linear momentum and of its angular momentum
        about the origin of ``mount``'s frame (a :class:`Mount`, None = the base frame), both in that frame's axes -- kg m / s
        and kg m^2 / s.  The mount's platform does not move and plays no part."""
        return _batch.momentum_batch(self, q, qd, mount, links)[0]

    def kinetic_energy(self, q, qd, links=None):
        """The kinetic energy [...] = 1/2 qd' M(q) qd of the links of ``links`` (as in :meth:`momentum`; None = the whole
        robot), in J: what the structure can transfer on contact, whatever the contact point and direction -- the upper envelope of
        :meth:`contact_energy`, which is the energy at given points."""
        return 0.5 * _batch.momentum_batch(self, q, qd, None, links)[1]

    def effective_mass(self, q, qd, points, directions=None):
        """The effective (reflected) mass [..., P] of the robot at the points of ``points`` (a :class:`ControlPoints`), in kg: what
        a contact there has to stop, m_R with 1 / m_R = u' J M(q)^-1 J' u.  ``directions`` None: u is the direction of each point's
        velocity at ``qd`` -- speed2 / mobility of :func:`toppra_amd.contact.effective_mass_batch`, NaN (0 / 0) where the point
        stands still, which has no direction.  ``directions`` [P, 3] (unit vectors in the points' link axes): 1 / mobility along
        them; ``qd`` is not read then and may be None."""
        speed2, mobility, _ = _contact.effective_mass_batch(self, q, qd, points, directions=directions)
        with np.errstate(divide="ignore", invalid="ignore"):  # (a standstill: 0 / 0, documented; tensors are not numpy's to warn about)
            return 1.0 / mobility if directions is not None else speed2 / mobility

    def contact_energy(self, q, qd, points, body_mass=None):
        """The energy [..., P] in J that a contact at each point of ``points`` can transfer at velocity ``qd``: 1/2 mu v^2 with v the
        point's speed, mu = (1 / m_body + 1 / m_R)^-1 the reduced mass of the body part (``body_mass`` in kg: a scalar or [P];
        None or inf = a clamped body part, 1 / m = 0) and of the robot's effective mass m_R along the point's velocity
        (:meth:`effective_mass`); 0 where the point stands still.  What ISO/TS 15066 power and force limiting caps per body
        region; :meth:`kinetic_energy` is its upper envelope."""
        speed2, mobility, _ = _contact.effective_mass_batch(self, q, qd, points)
        inv = _contact.inverse_body_mass(body_mass, int(speed2.shape[-1]))
        if not isinstance(speed2, np.ndarray):
            import torch
            inv = torch.as_tensor(inv, device=speed2.device)
            return torch.where(speed2 == 0, torch.zeros_like(speed2), 0.5 * speed2 / (inv + mobility / speed2))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(speed2 == 0, 0.0, 0.5 * speed2 / (inv + mobility / speed2))

    def joint_wrenches(self, q, qd, qdd, sections):
        """The wrench across the joints of ``sections`` (a :class:`JointSections`), [..., S, 6] in the set's order: per section
        [force; moment about its origin] in its axes -- what the parent side exerts ON the section's link through its joint,
        gravity included (at rest the force is the support of the weight of everything that hangs on the joint).  With the
        sections bound and the result flattened to [..., 6 S], a valid batched ``inv_dyn`` of
        :class:`toppra_amd.constraint.BatchSecondOrderConstraint`."""
        return _batch.joint_wrench_batch(self, q, qd, qdd, sections)

    def joint_wrench_terms(self, q, qs, qss, sections):
        """(w(q, 0, 0), w(q, 0, qs), w(q, qs, qss)) of :meth:`joint_wrenches` in one launch: the evaluations a limit on joint
        loads needs; the first is the static load, which gravity keeps from being zero."""
        return _batch.joint_wrench_terms_batch(self, q, qs, qss, sections)


class SerialChain(_Robot):
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

    Not modelled: rotor inertia, viscous damping, floating bases (branched robots: :class:`KinematicTree`); dry friction stays
    with the constraints (``fs_coef`` / ``friction``).  The model is uploaded to a device once per object, on first use there.
    """

    _family = "chain"

    def __init__(self, joint_types, axes, rotations, translations, masses, coms, inertias, gravity=(0.0, 0.0, -9.81),
                 tool=(0.0, 0.0, 0.0)):
        try:
            codes = [_JOINT_CODES[t.lower() if isinstance(t, str) else int(t)] for t in joint_types]
        except (KeyError, TypeError, ValueError):
            raise ValueError("joint_types must hold 'revolute' / 'prismatic' (or 'r' / 'p', 0 / 1), got %r" % (joint_types,))
        d = len(codes)
        if not 1 <= d <= _capi.MAX_DOF:
            raise ValueError("a chain has 1..%d joints, got %d" % (_capi.MAX_DOF, d))

        def fold(arr):  # inertias given as [d, 3, 3]
            full = arr["inertia"]
            if full.shape == (d, 3, 3):
                if not np.array_equal(full, np.swapaxes(full, 1, 2)):
                    raise ValueError("inertia matrices must be symmetric")
                arr["inertia"] = np.stack([full[:, 0, 0], full[:, 1, 1], full[:, 2, 2], full[:, 0, 1], full[:, 0, 2], full[:, 1, 2]], -1)

        arr = _arrays({"axis": axes, "rot": rotations, "trans": translations, "mass": masses, "com": coms, "inertia": inertias,
                       "gravity": gravity, "tool": tool},
                      {"axis": (d, 3), "rot": (d, 3, 3), "trans": (d, 3), "mass": (d,), "com": (d, 3), "inertia": (d, 6),
                       "gravity": (3,), "tool": (3,)}, infix=" for %d joints" % d, fold=fold)
        if np.any(np.abs(np.sqrt((arr["axis"] ** 2).sum(-1)) - 1.0) > 1e-12):
            raise ValueError("axes must be unit vectors (to 1e-12)")
        _need_rotation(arr["rot"], "rotations")
        if np.any(arr["mass"] < 0):
            raise ValueError("masses must be >= 0")
        self.dof = d
        self.joint_types = [PRISMATIC if c == _capi.JOINT_PRISMATIC else REVOLUTE for c in codes]
        self._codes = np.array(codes, dtype=np.int32)
        self._parents = (np.arange(d) - 1).astype(np.int32)  # the chain as a tree: -1, 0, 1, ...
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

    def as_tree(self, like):
        model, keep = self.c_struct(like)
        return model, self._parents, (keep, self._parents)

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

    def tool_wrench(self, q, qd, qdd, payload):
        """The wrench [..., 6] = [force; moment] the last link transmits to ``payload`` (a :class:`Payload`): the force on the
        body and its moment about the contact frame's origin, both in contact-frame axes.  Gravity is included: at rest the
        force is the support of the body's weight.  With the payload bound (``lambda q, qd, qdd: chain.tool_wrench(q, qd, qdd,
        payload)``) a valid batched ``inv_dyn`` of :class:`toppra_amd.constraint.BatchSecondOrderConstraint` (p = 6)."""
        return _batch.chain_tool_wrench_batch(self, q, qd, qdd, payload)

    def tool_wrench_terms(self, q, qs, qss, payload):
        """(wrench(q, 0, 0), wrench(q, 0, qs), wrench(q, qs, qss)) in one launch: the evaluations a limit on the wrench at the
        tool needs; the first is the static wrench, which gravity keeps from being zero."""
        return _batch.chain_tool_wrench_terms_batch(self, q, qs, qss, payload)

    def point_speeds(self, q, qs, points):
        """The squared speed of every point of ``points`` (a :class:`ControlPoints`) for qd = qs, shape [..., P]: per unit of path
        velocity, in the points' order.  A point (k, r) gives the bits of :meth:`tool_velocity_norm` on the chain cut after link k
        with tool = r."""
        return _batch.chain_points_speed_batch(self, q, qs, points)

    def point_accelerations(self, q, qd, qdd, points):
        """The linear acceleration of every point of ``points`` in world axes, [..., P, 3]: the classical acceleration of each
        point, as the first three of :meth:`tool_acceleration` are for the tool.  Kinematics only: gravity does not enter."""
        return _batch.chain_points_acceleration_batch(self, q, qd, qdd, points)

    def point_acceleration_terms(self, q, qs, qss, points):
        """(acc(q, 0, qs), acc(q, qs, qss)) of :meth:`point_accelerations` in one launch, [..., P, 3] each: the evaluations a
        limit on the points' accelerations needs; acc(q, 0, 0) is an exact zero."""
        return _batch.chain_points_acceleration_terms_batch(self, q, qs, qss, points)

    def with_payload(self, payload):
        """A new chain whose last link carries ``payload``: its mass, centre of mass and inertia merged into the last link's
        (parallel-axis theorem).  Host only; the contact frame plays no part.  Torque limits on the result load the joints
        with the carried object: ``BatchJointTorqueConstraint(arm.with_payload(obj), ...)``."""
        masses, coms, inertias = _with_payload_on(self.masses, self.coms, self.inertias, self.dof - 1, payload)
        return SerialChain(self.joint_types, self.axes, self.rotations, self.translations, masses, coms, inertias,
                           gravity=self.gravity, tool=self.tool)


class KinematicTree(_Robot):
    """A fixed-base tree of 1 .. 32 revolute / prismatic joints: a branched robot -- two arms on a torso or a lifting column, an
    arm beside a pan-tilt head, an arm with an articulated gripper -- or several robots on one base planned as one path.

    Parameters
    ----------
    parents : [d] integers.  ``parents[i]`` is the link that joint i attaches link i to, -1 = the fixed base (the world frame).
        The numbering is topological: ``-1 <= parents[i] < i``.  Several links may have parent -1 (a forest).
    joint_types, axes, rotations, translations, masses, coms, inertias, gravity : as for :class:`SerialChain`, per link;
        ``rotations[i]``, ``translations[i]`` place joint i in the frame of ``parents[i]``.

    There is no ``tool``: a tree has no single tip (:meth:`chain_to` gives the serial chain to any link, for the tool and
    control-point limits).  A FORK is a link j that is the parent of some link i != j + 1; a tree may have at most 4
    (``TPR_TREE_MAX_FORKS``).  ``parents = [-1, 0, 1, ...]`` is the serial chain and gives :class:`SerialChain`'s torques bit for
    bit.  Not modelled: floating bases, closed loops, rotor inertia, viscous damping.
    """

    _family = "tree"

    def __init__(self, parents, joint_types, axes, rotations, translations, masses, coms, inertias, gravity=(0.0, 0.0, -9.81)):
        try:
            raw = np.array(parents)
        except (TypeError, ValueError):
            raise ValueError("parents is not an array of integers")
        if raw.ndim != 1 or raw.dtype.kind not in "iu":
            raise ValueError("parents must be an integer array [d] (the parent link of every link, -1 = the base), got %r" % (parents,))
        d = int(raw.shape[0])
        if not 1 <= d <= _capi.MAX_DOF:
            raise ValueError("a tree has 1..%d joints, got %d" % (_capi.MAX_DOF, d))
        try:
            count = len(joint_types)
        except TypeError:
            raise ValueError("joint_types must hold one entry per link")
        if count != d:
            raise ValueError("parents has %d entries, joint_types %d: one per link each" % (d, count))
        raw = raw.astype(np.int64)
        for i in range(d):
            if not -1 <= raw[i] < i:
                raise ValueError("the parent of link %d is %d, outside -1 .. %d: links are numbered after their parents"
                                 % (i, int(raw[i]), i - 1))
        forks = sorted(set(int(raw[i]) for i in range(d) if raw[i] >= 0 and raw[i] != i - 1))
        if len(forks) > _capi.TREE_MAX_FORKS:
            raise NotImplementedError("the tree has %d forks (links %s), the kernels keep banks for %d"
                                      % (len(forks), forks, _capi.TREE_MAX_FORKS))
        # the links are a chain's: validated, packed and uploaded as one (its tool is not read)
        self._links = SerialChain(joint_types, axes, rotations, translations, masses, coms, inertias, gravity=gravity)
        self.dof = d
        self.parents = raw.astype(np.int32)
        self.parents.flags.writeable = False
        self.forks = forks
        for name in ("joint_types", "axes", "rotations", "translations", "masses", "coms", "inertias", "gravity"):
            setattr(self, name, getattr(self._links, name))

    def __repr__(self):
        leaves = self.dof - len(set(int(p) for p in self.parents if p >= 0))
        return "KinematicTree(%d dof, %d forks, %d leaves: %s)" % (
            self.dof, len(self.forks), leaves, "".join("P" if t == PRISMATIC else "R" for t in self.joint_types))

    @classmethod
    def from_chain(cls, chain):
        """The tree that is ``chain`` (its tool is dropped): parents -1, 0, 1, ..."""
        return cls(np.arange(chain.dof) - 1, chain.joint_types, chain.axes, chain.rotations, chain.translations, chain.masses,
                   chain.coms, chain.inertias, gravity=chain.gravity)

    def c_struct(self, like):
        """(tpr_chain of the links, the host parent array, what they point to) for a call whose arrays are of the kind of
        ``like`` (see :meth:`SerialChain.c_struct`).  The parent table is a host array in both cases."""
        model, keep = self._links.c_struct(like)
        return model, self.parents, (keep, self.parents)

    def inverse_dynamics(self, q, qd, qdd):
        """Joint torques / forces tau(q, qd, qdd) by recursive Newton-Euler over the tree: arrays [..., d] in, [..., d] out
        (numpy in -> numpy out, torch-ROCm tensors in -> a tensor out on the current stream).  A valid ``inv_dyn`` callback of
        the torque constraints."""
        return super(KinematicTree, self).inverse_dynamics(q, qd, qdd)

    def path_to(self, link):
        """The links from the base to ``link``, in order: the joints that move it."""
        link = int(link)
        if not 0 <= link < self.dof:
            raise ValueError("link %d is outside the tree's links 0..%d" % (link, self.dof - 1))
        path = []
        while link >= 0:
            path.append(link)
            link = int(self.parents[link])
        return np.array(path[::-1], dtype=np.int64)

    def chain_to(self, link, tool=(0.0, 0.0, 0.0)):
        """(SerialChain, joints): the serial chain from the base to ``link`` with ``tool`` in that link's frame, and the indices
        of its joints in the tree.  The tool and control-point entries of :class:`SerialChain` then evaluate on
        ``q[..., joints]``; their bounds enter a batch through ``BatchBoundConstraint``."""
        joints = self.path_to(link)
        chain = SerialChain([self.joint_types[i] for i in joints], self.axes[joints], self.rotations[joints], self.translations[joints],
                            self.masses[joints], self.coms[joints], self.inertias[joints], gravity=self.gravity, tool=tool)
        return chain, joints

    def with_payload(self, payload, link):
        """A new tree whose link ``link`` carries ``payload`` (a :class:`Payload` fixed in that link's frame): its mass, centre
        of mass and inertia merged into the link's, as :meth:`SerialChain.with_payload` does for a chain's last link."""
        link = int(link)
        if not 0 <= link < self.dof:
            raise ValueError("link %d is outside the tree's links 0..%d" % (link, self.dof - 1))
        masses, coms, inertias = _with_payload_on(self.masses, self.coms, self.inertias, link, payload)
        return KinematicTree(self.parents, self.joint_types, self.axes, self.rotations, self.translations, masses, coms, inertias,
                             gravity=self.gravity)

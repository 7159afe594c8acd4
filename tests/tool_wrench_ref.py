"""Plain numpy reference for the wrench a serial chain's last link transmits to a carried body (include/toppra_hip.h:
tpr_chain_tool_wrench_batch), written in WORLD coordinates from the forward recursion of tests/chain_ref.py (``forward`` with the
chain's own gravity: the base accelerates by -gravity).  With R, w, wd, a the last link's rotation, angular velocity, angular acceleration and origin acceleration in the world, and the payload (mass m, centre of mass c, inertia
I about c, contact frame Rc at p, all in the last link's frame):

    cw = R c,  Fw = m (a + wd x cw + w x (w x cw)),  Nw = R I R' wd + w x (R I R' w)
    f = Rc' R' Fw,   n = Rc' R' (Nw + (R (c - p)) x Fw)

the force on the body and its moment about the contact frame's origin, in contact-frame axes.  Like ``chain_ref.rnea`` it takes
``dtype`` (np.longdouble as well) and ``absolute=True`` (every product and sum in absolute value: the metric's magnitude).

A payload is a dict: mass, com [3], inertia [6] = xx, yy, zz, xy, xz, yz, rot [3, 3], origin [3].
"""
import numpy as np

from tests import chain_ref
from tests.chain_ref import _add, _cross, _mtv, _mv, _scale


def tool_wrench(chain, payload, q, qd, qdd, dtype=np.float64, absolute=False):
    """wrench(q, qd, qdd) [..., 6] = [f; n] in contact-frame axes; arrays [..., d]."""
    links, ar = chain_ref.forward(chain, q, qd, qdd, dtype, absolute)
    L = links[-1]
    R, w, wd = L["R"], L["w"], L["wd"]
    com, origin = ar.vec(payload["com"]), ar.vec(payload["origin"])
    cw = _mv(R, com)
    ac = _add(_add(L["a"], _cross(wd, cw)), _cross(w, _cross(w, cw)))
    Fw = _scale(ac, ar.scalar(payload["mass"]))
    inertia = ar.inertia(R, payload["inertia"])
    Nw = _add(inertia(wd), _cross(w, inertia(w)))
    arm = _mv(R, [com[j] - origin[j] for j in range(3)])
    nw = _add(Nw, _cross(arm, Fw))
    Rc = ar.mat(payload["rot"])
    return ar.stack(_mtv(Rc, _mtv(R, Fw)) + _mtv(Rc, _mtv(R, nw)))


def payload_of(p, chain):
    """The toppra_amd.chain.Payload of a payload dict."""
    from toppra_amd.chain import Payload
    return Payload(p["mass"], com=p["com"], inertia=p["inertia"], frame_rotation=p["rot"], frame_origin=p["origin"])


def extended_chain(chain, payload, axis, prismatic):
    """The independent route: ``chain`` with a (d+1)-th joint at the contact frame (rot, origin) whose link IS the payload --
    centre of mass rot' (com - origin), inertia rotated into the contact frame.  Held at q = qd = qdd = 0, the last entry of
    its inverse dynamics is axis . n (revolute) or axis . f (prismatic) of the wrench."""
    Rc, I = np.asarray(payload["rot"]), np.asarray(payload["inertia"])
    full = np.array([[I[0], I[3], I[4]], [I[3], I[1], I[5]], [I[4], I[5], I[2]]])
    rotated = Rc.T @ full @ Rc
    rotated = 0.5 * (rotated + rotated.T)
    ext = {k: np.array(v) for k, v in chain.items()}
    ext["joint_type"] = np.append(chain["joint_type"], 1 if prismatic else 0).astype(np.int32)
    ext["axis"] = np.vstack([chain["axis"], np.asarray(axis, dtype=np.float64)[None]])
    ext["rot"] = np.concatenate([chain["rot"], Rc[None]])
    ext["trans"] = np.vstack([chain["trans"], np.asarray(payload["origin"])[None]])
    ext["mass"] = np.append(chain["mass"], payload["mass"])
    ext["com"] = np.vstack([chain["com"], (Rc.T @ (np.asarray(payload["com"]) - np.asarray(payload["origin"])))[None]])
    ext["inertia"] = np.vstack([chain["inertia"], np.array([rotated[0, 0], rotated[1, 1], rotated[2, 2], rotated[0, 1],
                                                            rotated[0, 2], rotated[1, 2]])[None]])
    return ext

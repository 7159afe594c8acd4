"""Plain numpy reference for the tool point's acceleration of the serial chain (include/toppra_hip.h:
tpr_chain_tool_acceleration_batch), in WORLD coordinates: the forward recursion of tests/chain_ref.py (``forward``) with the
gravity parameter set to zero -- the base is at rest, this is kinematics -- plus the tool offset:

    lin = a_d + wd_d x t + w_d x (w_d x t),   ang = wd_d,   t = R_d tool

with a_d, w_d, wd_d the last link's origin acceleration, angular velocity and angular acceleration in the world.  ``lin`` is the
classical acceleration of the point: the second time derivative of its world position.  Like ``chain_ref.rnea`` it takes
``dtype`` (np.longdouble as well) and ``absolute=True`` (every product and sum in absolute value: the metric's magnitude).
"""
import numpy as np

from tests import chain_ref
from tests.chain_ref import _add, _cross, _mv


def tool_acceleration(chain, q, qd, qdd, dtype=np.float64, absolute=False):
    """acc(q, qd, qdd) [..., 6] = [lin; ang] in world axes; arrays [..., d]."""
    links, ar = chain_ref.forward(dict(chain, gravity=np.zeros(3)), q, qd, qdd, dtype, absolute)
    L = links[-1]
    tool = _mv(L["R"], ar.vec(chain["tool"]))
    lin = _add(_add(L["a"], _cross(L["wd"], tool)), _cross(L["w"], _cross(L["w"], tool)))
    return ar.stack(lin + L["wd"])

"""``SimplePath``: a geometric path through positions and, optionally, first derivatives at given path positions.

A host-side interface mirror like ``SplineInterpolator``: constructor, ``__call__``, ``dof``, ``path_interval`` and ``waypoints``
as the reference's class of this name has them, and one scipy ``BPoly.from_derivatives`` per joint, so that the samples
``path(gridpoints, order)`` handed to the solver are the reference's for the same scipy.
"""
import numpy as np
from scipy.interpolate import BPoly

from .interpolator import AbstractGeometricPath


class SimplePath(AbstractGeometricPath):
    """Hermite path: values ``y`` [n] or [n, dof] and first derivatives ``yd`` (shape of ``y``) at the positions ``x`` [n].
    Without ``yd`` an interior derivative is the central difference of its two neighbours and both ends are at rest."""

    def __init__(self, x, y, yd=None):
        self._knots = np.asarray(x)
        values = np.asarray(y).astype(float)
        self._values = values[:, None] if values.ndim == 1 else values
        if yd is None:
            slopes = np.zeros_like(self._values)
            if len(slopes) > 2:
                span = self._knots[2:] - self._knots[:-2]
                slopes[1:-1] = (self._values[2:] - self._values[:-2]) / span[:, None]
        else:
            slopes = np.asarray(yd).astype(float).reshape(self._values.shape)
        # one Bernstein-basis polynomial per joint, derivatives of every order cached on first use
        self._orders = {0: [BPoly.from_derivatives(self._knots, np.column_stack((self._values[:, j], slopes[:, j])))
                            for j in range(self._values.shape[1])]}

    def _polynomials(self, order):
        if order not in self._orders:
            self._orders[order] = [poly.derivative(order) for poly in self._orders[0]]
        return self._orders[order]

    def __call__(self, xi, order=0):
        """[len(xi), dof] ([dof] for a scalar): the path (order 0) or its ``order``-th derivative at ``xi``."""
        return np.array([poly(xi) for poly in self._polynomials(order)]).T

    @property
    def dof(self):
        return self._values.shape[1]

    @property
    def path_interval(self):
        return np.array([self._knots[0], self._knots[-1]], dtype=float)

    @property
    def waypoints(self):
        return self._values

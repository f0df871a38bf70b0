"""Boundary conditions of the ADER-DG solver at the faces of the domain (AderDgSolver(boundary=...)).

A boundary is a dict {(axis, side): condition}, side 0 = low and 1 = high face; a face it does not name stays periodic.  Every condition
prescribes the ghost trace stage B reads beyond the face, as the halo exchange does between blocks (include/exahype_hip.h
exa_dg_boundary_ghost):

  Outflow()          the cell's own outward trace: the Rusanov flux becomes F(q_in)
  Wall(sign=None)    state s * q_in and flux -s * F_in; a mirror image of the domain across the face for term sets with F_d(S q) = -S F_d(q),
                     S = diag(s).  sign=None: only for the built-in Euler sets (the normal momentum, variable 1 + axis, changes sign)
  Dirichlet(state)   a prescribed state: an array [n_vars] (constant), or a callable f(x, t) -> [n, n_vars] on device tensors, x: [n, 3]; the
                     ghost is then the time average over the step's Gauss time levels of f and of its normal flux

This module needs neither torch nor a GPU: validate_boundary() is what the solver calls on its argument.
"""
import numpy as np

from ._lib import PDE_EULER, PDE_EULER_REF2D

BC_OUTFLOW, BC_WALL, BC_DIRICHLET = 1, 2, 3      # include/exahype_hip.h EXA_BC_*


class Outflow:
    kind = BC_OUTFLOW

    def __repr__(self):
        return "Outflow()"


class Wall:
    kind = BC_WALL

    def __init__(self, sign=None):
        self.sign = None if sign is None else np.asarray(sign, dtype=np.float64).reshape(-1)

    def __repr__(self):
        return "Wall(sign=%s)" % (None if self.sign is None else list(self.sign))


class Dirichlet:
    kind = BC_DIRICHLET

    def __init__(self, state):
        self.state = state if callable(state) else np.asarray(state, dtype=np.float64)

    @property
    def constant(self):
        return not callable(self.state)

    def __repr__(self):
        return "Dirichlet(%s)" % (getattr(self.state, "__name__", "f") if callable(self.state) else list(self.state))


def euler_wall_sign(pde, n_vars, axis):
    """The reflection of the built-in Euler sets at a face normal to `axis`: -1 on the normal momentum, +1 elsewhere."""
    if pde not in (PDE_EULER, PDE_EULER_REF2D):
        return None
    s = np.ones(n_vars)
    s[1 + axis] = -1.0
    return s


def validate_boundary(boundary, dim, n_vars, pde):
    """Check a boundary dict and resolve it: returns {(axis, side): condition} with every Wall's sign filled in (a new Wall), {} for None.
    Raises ValueError on an axis outside the domain, a side other than 0 / 1, a condition of another type, a constant Dirichlet state or a
    wall sign whose length is not n_vars, a non-finite state, a sign entry other than +-1, and a Wall without sign for a term set other
    than the built-in Euler sets."""
    if boundary is None:
        return {}
    if not isinstance(boundary, dict):
        raise ValueError("boundary: a dict {(axis, side): Outflow() | Wall(...) | Dirichlet(...)}, got %r" % type(boundary).__name__)
    out = {}
    for key, bc in boundary.items():
        if not (isinstance(key, tuple) and len(key) == 2 and all(isinstance(k, (int, np.integer)) for k in key)):
            raise ValueError("boundary: key %r is not (axis, side)" % (key,))
        axis, side = int(key[0]), int(key[1])
        if not 0 <= axis < dim:
            raise ValueError("boundary: axis %d outside a %d-D domain" % (axis, dim))
        if side not in (0, 1):
            raise ValueError("boundary: side %d of axis %d (0 = low, 1 = high)" % (side, axis))
        if isinstance(bc, Outflow):
            out[(axis, side)] = bc
        elif isinstance(bc, Wall):
            s = bc.sign
            if s is None:
                s = euler_wall_sign(pde, n_vars, axis)
                if s is None:
                    raise ValueError("boundary: Wall() at (%d, %d) needs sign= for pde %d (the default reflection is the built-in Euler sets')"
                                     % (axis, side, pde))
            if s.shape != (n_vars,):
                raise ValueError("boundary: Wall sign at (%d, %d) has %d entries, the term set %d variables" % (axis, side, s.size, n_vars))
            if not np.all(np.abs(s) == 1.0):
                raise ValueError("boundary: Wall sign at (%d, %d) must hold +1 / -1 only, got %s" % (axis, side, list(s)))
            out[(axis, side)] = Wall(s)
        elif isinstance(bc, Dirichlet):
            if bc.constant:
                if bc.state.shape != (n_vars,):
                    raise ValueError("boundary: Dirichlet state at (%d, %d) has shape %s, expected (%d,)" % (axis, side, bc.state.shape, n_vars))
                if not np.all(np.isfinite(bc.state)):
                    raise ValueError("boundary: Dirichlet state at (%d, %d) is not finite" % (axis, side))
            out[(axis, side)] = bc
        else:
            raise ValueError("boundary: %r at (%d, %d) is not Outflow(), Wall(...) or Dirichlet(...)" % (bc, axis, side))
    return out


def coefficients(bc, n_vars):
    """The host factors exa_dg_boundary_ghost takes: 2 n_vars (state, flux) factors for Outflow / Wall, the state for a constant Dirichlet,
    None for a Dirichlet function."""
    if isinstance(bc, Outflow):
        return np.ones(2 * n_vars)
    if isinstance(bc, Wall):
        return np.concatenate([bc.sign, -bc.sign])
    return np.array(bc.state, dtype=np.float64) if bc.constant else None

"""Boundary conditions at the faces of the domain: AderDgSolver(boundary=...), the SubcellLimiter that follows it, and FVPatchGrid(boundary=...).

A boundary is a dict {(axis, side): condition}, side 0 = low and 1 = high face; a face it does not name stays periodic.

ADER-DG: every condition prescribes the ghost trace stage B reads beyond the face, as the halo exchange does between blocks
(include/exahype_hip.h exa_dg_boundary_ghost):

  Outflow()          the cell's own outward trace: the Rusanov flux becomes F(q_in)
  Wall(sign=None)    state s * q_in and flux -s * F_in; a mirror image of the domain across the face for term sets with F_d(S q) = -S F_d(q),
                     S = diag(s).  sign=None: only for the built-in Euler sets (the normal momentum, variable 1 + axis, changes sign)
  Dirichlet(state)   a prescribed state: an array [n_vars] (constant), or a callable f(x, t) -> [n, n_vars] on device tensors, x: [n, 3]; the
                     ghost is then the time average over the step's Gauss time levels of f and of its normal flux.  A constant state is
                     its own average; its flux is averaged over the levels too where the term set's flux sees x or t

FV patch grid: every condition prescribes the volumes of the halo layers beyond the face (include/exahype_hip.h exa_fv_grid_step_device_bc;
fv_faces() below turns the dict into the kinds and the per-face data of that call):

  Outflow()          the patch's own interior volume at the same distance inside the face (a mirror with every sign +1): the Rusanov flux at the
                     face becomes F(q_in)
  Wall(sign=None)    that mirror volume times s on the evolved variables, +1 on the auxiliary ones (sign=None as above)
  Dirichlet(state)   a constant state [n_real + n_aux] in every volume beyond the face -- as a bare array means.  One state per face: a callable
                     is refused (position- or time-dependent FV ghosts are not supported)

This module needs neither torch nor a GPU: validate_boundary() / fv_faces() are what the solvers call on their argument.
"""
import numpy as np

from ._lib import FV_FACE_MIRROR, FV_FACE_PERIODIC, FV_FACE_STATE, PDE_EULER, PDE_EULER_REF2D

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


def fv_faces(boundary, dim, n_real, n_aux, pde):
    """FVPatchGrid's boundary dict, resolved for exa_fv_grid_step_device_bc: (kinds [2 dim], data [2 dim][V], conditions), V = n_real + n_aux.
    Face axis * 2 + side is FV_FACE_PERIODIC (not named), FV_FACE_STATE with its state as data (Dirichlet(constant) or a bare array,
    broadcast to [V] as FVPatchGrid always did) or FV_FACE_MIRROR with its signs as data (Outflow: all +1; Wall: its sign on the n_real evolved
    variables -- resolved by validate_boundary with n_real variables -- and +1 on the auxiliary ones).  conditions: {(axis, side): Outflow() |
    Wall(sign [n_real]) | Dirichlet(state [V])}, what fill_halos_boundary takes.  Raises ValueError like validate_boundary, and on a callable
    Dirichlet, a state that does not broadcast to [V] and a state that is not finite."""
    V = n_real + n_aux
    if not isinstance(boundary, dict):
        raise ValueError("boundary: a dict {(axis, side): Outflow() | Wall(...) | Dirichlet(state) | state}, got %r" % type(boundary).__name__)
    checked, states = {}, {}
    for key, bc in boundary.items():
        if isinstance(bc, (Outflow, Wall)):
            checked[key] = bc
            continue
        if isinstance(bc, Dirichlet):
            if not bc.constant:
                raise ValueError("boundary: Dirichlet(function) at %r -- the FV grid takes one constant state per face" % (key,))
            state = bc.state
        else:
            try:
                state = np.asarray(bc, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError("boundary: %r at %r is not Outflow(), Wall(...), Dirichlet(state) or a state" % (bc, key)) from None
        try:
            state = np.array(np.broadcast_to(state, (V,)))
        except ValueError:
            raise ValueError("boundary: the state at %r has shape %s, expected (%d,)" % (key, np.shape(state), V)) from None
        if not np.all(np.isfinite(state)):
            raise ValueError("boundary: the state at %r is not finite" % (key,))
        checked[key] = Dirichlet(state[:n_real])
        states[key] = state
    resolved = validate_boundary(checked, dim, n_real, pde)          # (keys, wall signs)
    states = {(int(k[0]), int(k[1])): v for k, v in states.items()}
    kinds, data, conditions = [FV_FACE_PERIODIC] * (2 * dim), np.zeros((2 * dim, V)), {}
    for (a, side), bc in resolved.items():
        f = a * 2 + side
        if isinstance(bc, Dirichlet):
            kinds[f], data[f] = FV_FACE_STATE, states[(a, side)]
            conditions[(a, side)] = Dirichlet(states[(a, side)])
        else:
            kinds[f], data[f] = FV_FACE_MIRROR, 1.0
            if isinstance(bc, Wall):
                data[f, :n_real] = bc.sign
            conditions[(a, side)] = bc
    return kinds, data, conditions

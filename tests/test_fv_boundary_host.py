"""FVPatchGrid boundary conditions, the part that needs no GPU: the validation of the boundary dict (exahype_amd/boundary.py fv_faces), the
reference restatement the GPU tests compare against (tests/fv_boundary_ref.py) and the torch / numpy halo fill of the two-pass form
(solvers.fill_halos_boundary)."""
import os
import re

import numpy as np
import pytest

from exahype_amd import Dirichlet, Outflow, Wall
from exahype_amd._lib import PDE_ADVECTION, PDE_EULER
from exahype_amd.boundary import fv_faces
from oracle import fv_reference as R
from tests import fv_boundary_ref as B
from tests import fv_cases as K

LD = R.LD


def test_faces_resolved():
    kinds, data, cond = fv_faces({(0, 0): Wall(), (0, 1): Outflow(), (1, 1): Dirichlet(np.arange(7.0)), (2, 0): np.full(7, 2.0)}, 3, 5, 2, PDE_EULER)
    assert kinds == [B.MIRROR, B.MIRROR, B.PERIODIC, B.STATE, B.STATE, B.PERIODIC]
    assert np.array_equal(data[0], [1, -1, 1, 1, 1, 1, 1]) and np.array_equal(data[1], np.ones(7))
    assert np.array_equal(data[3], np.arange(7.0)) and np.array_equal(data[4], np.full(7, 2.0)) and not data[2].any() and not data[5].any()
    assert sorted(cond) == [(0, 0), (0, 1), (1, 1), (2, 0)] and np.array_equal(cond[(0, 0)].sign, [1, -1, 1, 1, 1])
    assert np.array_equal(fv_faces({(1, 0): Wall()}, 2, 5, 0, PDE_EULER)[1][2], [1, 1, -1, 1, 1])
    assert fv_faces({}, 2, 5, 5, PDE_EULER)[0] == [B.PERIODIC] * 4


@pytest.mark.parametrize("bad, dim, n_real, n_aux, pde, msg", [
    ({(0, 0): Dirichlet(lambda x, t: x)}, 2, 5, 0, PDE_EULER, "constant state per face"),
    ({(0, 0): Wall(sign=[1, -1, 1])}, 2, 5, 0, PDE_EULER, "3 entries"),
    ({(0, 0): Wall(sign=[1, -1, 1, 1, 1, 1, 1])}, 2, 5, 2, PDE_EULER, "7 entries"),
    ({(0, 0): Wall()}, 2, 5, 0, PDE_ADVECTION, "needs sign="),
    ({(2, 0): Outflow()}, 2, 5, 0, PDE_EULER, "axis 2"),
    ({(-1, 0): np.ones(5)}, 2, 5, 0, PDE_EULER, "axis -1"),
    ({(0, 2): Outflow()}, 2, 5, 0, PDE_EULER, "side 2"),
    ({0: Outflow()}, 2, 5, 0, PDE_EULER, "not (axis, side)"),
    ({(0, 0): np.ones(4)}, 2, 5, 0, PDE_EULER, "expected (5,)"),
    ({(0, 0): Dirichlet([1.0, 0, 0, 0, np.nan])}, 2, 5, 0, PDE_EULER, "not finite"),
    ({(0, 0): "wall"}, 2, 5, 0, PDE_EULER, "is not Outflow"),
    ({(0, 0): Wall(sign=[1, -2, 1, 1, 1])}, 2, 5, 0, PDE_EULER, "+1 / -1"),
    (np.ones(5), 2, 5, 0, PDE_EULER, "a dict"),
])
def test_validation(bad, dim, n_real, n_aux, pde, msg):
    with pytest.raises(ValueError) as e:
        fv_faces(bad, dim, n_real, n_aux, pde)
    assert msg in str(e.value), str(e.value)


def _states(dim, grid, P, V, seed, family="benign"):
    return K.state(family, int(np.prod(grid)), dim, P, 0, V, seed).reshape(tuple(grid) + (P,) * dim + (V,))


@pytest.mark.parametrize("dim, grid, P, V", [(2, (3, 2), 4, 7), (3, (2, 1, 2), 3, 5)])
def test_restatement_is_grid_update_for_the_old_kinds(dim, grid, P, V):
    U = _states(dim, grid, P, V, 5)
    dt, h = K.cfl_step(U, dim, R.PDE_EULER)
    want = R.grid_update(U, dt, h, dim, 5, R.PDE_EULER)
    got = B.grid_update(U, dt, h, dim, 5, R.PDE_EULER, [B.PERIODIC] * (2 * dim), np.zeros((2 * dim, V)))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    bnd = {(a, s): K.state("benign", 1, dim, 1, 0, V, 40 + 2 * a + s).reshape(V) for a in range(dim) for s in range(2)}
    want = R.grid_update(U, dt, h, dim, 5, R.PDE_EULER, boundary=bnd)
    kinds, data = B.faces_of(bnd, dim, 5, V - 5, R.PDE_EULER)
    assert kinds == [B.STATE] * (2 * dim)
    got = B.grid_update(U, dt, h, dim, 5, R.PDE_EULER, kinds, data)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("dim, grid, P", [(2, (2, 3), 4), (3, (2, 1, 2), 3)])
def test_closed_box_conserves_mass_and_energy(dim, grid, P):
    """every face a wall: the face fluxes of density and energy vanish in exact arithmetic (the mirror state has the same density, pressure and
    speed of sound and the opposite normal velocity), so the sums move by the long-double rounding of the step only"""
    U = _states(dim, grid, P, 5, 9, "riemann")
    kinds, data = B.faces_of({(a, s): Wall() for a in range(dim) for s in range(2)}, dim, 5, 0, R.PDE_EULER)
    dt, h = K.cfl_step(U, dim, R.PDE_EULER)
    for _ in range(3):
        new = B.grid_update(U, dt, h, dim, 5, R.PDE_EULER, kinds, data, track=False).new
        for v in (0, 4):
            before, after, mag = np.sum(U[..., v].astype(LD)), np.sum(new[..., v]), np.sum(np.abs(new[..., v]))
            assert abs(after - before) <= 16 * LD(2) ** -64 * mag, (v, float(after - before), float(mag))
        U = new.astype(np.float64)
    # the momentum normal to a wall is NOT conserved (the wall pushes back): the check above is not vacuous
    assert abs(np.sum(new[..., 1]) - np.sum(_states(dim, grid, P, 5, 9, "riemann")[..., 1].astype(LD))) > 1e-6


@pytest.mark.parametrize("dim, grid, P", [(2, (2, 2), 4), (3, (1, 2, 2), 3)])
def test_constant_state_is_a_fixed_point_under_outflow(dim, grid, P):
    q = np.array([1.3, 0.4, -0.2, 0.1, 2.9])
    U = np.broadcast_to(q, tuple(grid) + (P,) * dim + (5,)).copy()
    kinds, data = B.faces_of({(a, s): Outflow() for a in range(dim) for s in range(2)}, dim, 5, 0, R.PDE_EULER)
    new = B.grid_update(U, 0.01, 0.1, dim, 5, R.PDE_EULER, kinds, data, track=False).new
    assert np.array_equal(new, U.astype(LD))


@pytest.mark.parametrize("dim, grid, P, H", [(2, (1, 3), 4, 1), (2, (2, 2), 4, 2), (3, (2, 1, 2), 3, 1)])
def test_fill_halos_boundary_is_the_padded_global_array(dim, grid, P, H):
    """the two-pass form's halo fill (numpy here, torch on the device) puts into the stencil's halo entries what the restatement pads with: every
    face kind, a grid extent of 1 with a different kind either side"""
    from exahype_amd.solvers import fill_halos_boundary
    V = 7
    U = _states(dim, grid, P, V, 3)
    cond = {(0, 0): Wall(), (0, 1): Outflow(), (1, 0): Dirichlet(np.arange(1.0, V + 1)), (1, 1): Wall(sign=[1, 1, -1, -1, 1])}
    kinds, data, resolved = fv_faces(cond, dim, 5, V - 5, PDE_EULER)
    S = P + 2 * H
    Q = np.zeros(tuple(grid) + (S,) * dim + (V,))
    Q[(slice(None),) * dim + (slice(H, H + P),) * dim] = U
    fill_halos_boundary(Q, grid, dim, P, H, resolved)
    assert np.array_equal(Q[(slice(None),) * dim + (slice(H, H + P),) * dim], U)
    A = B.padded(R.assemble(U, dim), dim, kinds, data)             # one layer: the layer next to the faces
    cut = Q[(slice(None),) * dim + (slice(H - 1, H + P + 1),) * dim]
    for idx in np.ndindex(*grid):
        for a in range(dim):
            for side in range(2):
                sel = [slice(1, P + 1)] * dim
                sel[a] = 0 if side == 0 else P + 1
                glob = [slice(1 + idx[b] * P, 1 + (idx[b] + 1) * P) for b in range(dim)]
                glob[a] = idx[a] * P if side == 0 else (idx[a] + 1) * P + 1
                assert np.array_equal(cut[idx][tuple(sel)], A[tuple(glob)]), (idx, a, side)
    if H == 2:                                                      # the second layer: the mirror reaches one volume deeper
        q = Q[(0,) * dim]
        lo = [slice(H, H + P)] * dim
        lo[0] = 0
        inner = [slice(H, H + P)] * dim
        inner[0] = 2 * H - 1
        assert np.array_equal(q[tuple(lo)], q[tuple(inner)] * data[0])


def test_new_entry_declared_and_bound():
    from exahype_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "exahype_hip.h")).read()
    assert re.search(r"\bint\s+exa_fv_grid_step_device_bc\s*\(", header)
    for k, v in (("PERIODIC", 0), ("STATE", 1), ("MIRROR", 2)):
        assert re.search(r"#define\s+EXA_FV_FACE_%s\s+%d\b" % (k, v), header) and getattr(_lib, "FV_FACE_" + k) == v
    assert len(_lib.SIGNATURES["exa_fv_grid_step_device_bc"][1]) == len(_lib.SIGNATURES["exa_fv_grid_step_device"][1]) + 1
    assert hasattr(_lib.load(), "exa_fv_grid_step_device_bc")

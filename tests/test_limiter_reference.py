"""The long-double reference of the limiter glue (oracle/limiter_reference.py), without a GPU:

1. the committed operator file is what mpmath gives, digit for digit; the reference operators satisfy R P = I, mean preservation, and
   constants stay constants;
2. the fp64 numpy oracle's P and R (oracle/limiter_numpy.py) lie within 8 * 2^-53 * cond(K) of them;
3. the bound tests/test_limiter_kernels.py holds the kernels to is sound: a correct fp64 tensor product (numpy) stays inside it, element by
   element, on every input of the GPU case table;
4. and it is sharp: every mutant of the reference (a halo from the wrong side, axis, layer or neighbour, an edge entry continued from a
   halo, an operator row off by one, a face buffer transposed) leaves it by a factor of 100 at least on every input of that table.
"""
import json

import numpy as np
import pytest

from oracle import limiter_reference as L
from oracle.dg_operators import operators
from oracle.limiter_numpy import apply_all_axes, projection_matrix, reconstruction_matrix
from tests import limiter_cases as K

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def test_operator_file_is_what_mpmath_gives():
    with open(L.OPERATORS_FILE) as f:
        assert json.load(f) == L.operators_file_content()
    ops = L.load_operators_file()
    assert sorted(ops) == list(L.ORDERS)
    for N in L.ORDERS:
        h = L.limiter_operators_hp(N)
        assert h["P"].dtype == LD and h["R"].dtype == LD and h["P"].shape == (2 * N - 1, N) and h["R"].shape == (N, 2 * N - 1)
        assert all(np.array_equal(ops[N][k], h[k]) for k in ("P", "R", "w")) and ops[N]["condK"] == h["condK"]


@pytest.mark.parametrize("N", L.ORDERS)
def test_reference_operator_identities(N):
    h = L.limiter_operators_hp(N)
    P, R, w, Ns = h["P"], h["R"], h["w"], 2 * N - 1
    tol = 16 * Ns * EPS_LD * float(np.max(np.abs(R) @ np.abs(P)))            # entries rounded to long double, sums of N_s products
    assert float(np.max(np.abs(R @ P - np.eye(N)))) < tol                      # exact on degree <= p data
    assert float(np.max(np.abs(w @ R - LD(1) / Ns))) < tol                     # the reconstruction preserves the mean of ANY data
    assert float(np.max(np.abs(P.sum(axis=1) - 1))) < tol                      # constants stay constants
    assert float(np.max(np.abs(P.mean(axis=0) - w))) < tol                     # the projection preserves the cell mean
    assert 15 < h["condK"] < 200                                              # nothing ill-posed


@pytest.mark.parametrize("N", L.ORDERS)
def test_numpy_oracle_operators_vs_reference(N):
    h, o = L.limiter_operators_hp(N), operators(N)
    P = projection_matrix(o["xi"], 2 * N - 1)
    R = reconstruction_matrix(P, o["w"])
    tol = L.operator_tolerance(h["condK"])
    eP, eR = float(np.max(np.abs(P - h["P"]))), float(np.max(np.abs(R - h["R"])))
    print("N %d: |P - P_hp| %.2e, |R - R_hp| %.2e, tolerance %.2e" % (N, eP, eR, tol))
    assert eP <= tol and eR <= tol


@pytest.mark.parametrize("dim,N", K.KERNEL_CASES)
def test_fp64_tensor_products_stay_inside_the_rounding_bound(dim, N):
    """What the GPU tests hold the kernels to holds for numpy's fp64 products of the same operator (rounded to fp64, as the device's is)."""
    h = L.limiter_operators_hp(N)
    P, R = h["P"].astype(np.float64), h["R"].astype(np.float64)
    worst = [0.0, 0.0]
    for i, (nc, kind, u) in enumerate(K.inputs(dim, N)):
        ref = L.project_grid(u, P)
        bound = L.rounding_factor(dim, N) * L.project_grid(np.abs(u), np.abs(P))
        worst[0] = max(worst[0], K.worst_ratio(apply_all_axes(P, u, dim, dim), ref, bound))
        for p in K.random_patches(dim, N, 5, 2, seed=7 * N + dim + i):
            core = p[(slice(1, -1),) * dim]
            worst[1] = max(worst[1], K.worst_ratio(apply_all_axes(R, core, dim, 0), L.reference_reconstruct(p, R), K.reconstruction_bound(p, R)))
    print("dim %d N %d: projection %.2f, reconstruction %.2f of the bound" % (dim, N, worst[0], worst[1]))
    assert max(worst) <= 1.0, worst


# ---- deliberate mistakes, built from the pieces of the reference ---------------------------------------------------------------------------
def _halo_mutant(kind):
    """Patch whose face halos come from a wrongly chosen neighbour cell or subcell layer."""
    def patch(u, cell, P, proj):
        dim, nc, Ns = (u.ndim - 1) // 2, u.shape[:(u.ndim - 1) // 2], P.shape[0]
        cc = np.unravel_index(cell, nc)
        out = L.reference_patch(u, cell, P, proj=proj)
        for a in range(dim):
            for side in (0, 1):
                nb, step, row = list(cc), (1 if side else -1), (0 if side else Ns - 1)
                an = (a + 1) % dim if kind == "wrong_axis" else a                         # the neighbour along another axis
                if kind == "neighbour_swapped":
                    step = -step                                                          # the neighbour on the other side
                nb[an] = min(max(nb[an] + step, 0), nc[an] - 1) if kind == "no_wrap" else (nb[an] + step) % nc[an]
                if kind == "layer_swapped":
                    row = Ns - 1 - row                                                    # the neighbour's far layer
                if kind == "halo_row_shift":
                    row += 1 if side else -1                                              # operator row off by one
                out[L.face_slice(dim, Ns, a, side)] = np.take(proj[tuple(nb)], row, axis=a)
        return out
    return patch


def _interior_row_shift(u, cell, P, proj):
    """One row of P replaced by its neighbour in the cell's own projection (interior, edges and corners)."""
    dim, Ns = (u.ndim - 1) // 2, P.shape[0]
    ref = L.reference_patch(u, cell, P, proj=proj)
    Pm = np.array(P, dtype=LD)
    Pm[Ns // 2] = Pm[Ns // 2 - 1]
    own = apply_all_axes(Pm, u[np.unravel_index(cell, u.shape[:dim])].astype(LD), dim, 0)
    out = np.pad(own, [(1, 1)] * dim + [(0, 0)], mode="edge")
    for a in range(dim):
        for side in (0, 1):
            out[L.face_slice(dim, Ns, a, side)] = ref[L.face_slice(dim, Ns, a, side)]
    return out


def _edge_from_neighbour(u, cell, P, proj):
    """Edge and corner entries continue a face halo (neighbour data) instead of the interior."""
    dim, Ns = (u.ndim - 1) // 2, P.shape[0]
    out = L.reference_patch(u, cell, P, proj=proj)
    idx = np.indices((Ns + 2,) * dim)
    halo = (idx == 0) | (idx == Ns + 1)
    first = np.argmax(halo, axis=0)                                                       # this halo coordinate stays, the others are clamped
    src = np.clip(idx, 1, Ns)
    for a in range(dim):
        src[a] = np.where(first == a, idx[a], src[a])
    edge = halo.sum(axis=0) >= 2
    out[edge] = out[tuple(src)][edge]
    return out


MUTANTS_PATCH = dict({k: _halo_mutant(k) for k in ("layer_swapped", "neighbour_swapped", "wrong_axis", "halo_row_shift", "no_wrap")},
                     interior_row_shift=_interior_row_shift, edge_from_neighbour=_edge_from_neighbour)


def _transposed(u, d, side, P):
    Ns, nv = P.shape[0], u.shape[-1]
    return np.swapaxes(L.reference_face_layers(u, d, side, P).reshape(-1, Ns, Ns, nv), 1, 2).reshape(-1, Ns * Ns, nv)


MUTANTS_FACE = dict(
    side_swapped=lambda u, d, side, P: L.boundary_cell_layers(u, d, 0 if side else u.shape[d] - 1, P.shape[0] - 1 if side else 0, P),
    layer_swapped=lambda u, d, side, P: L.boundary_cell_layers(u, d, u.shape[d] - 1 if side else 0, 0 if side else P.shape[0] - 1, P),
    row_shift=lambda u, d, side, P: L.boundary_cell_layers(u, d, u.shape[d] - 1 if side else 0, P.shape[0] - 2 if side else 1, P),
    transposed=_transposed)                                                               # (3-D: the two transverse subcell axes exchanged)


@pytest.mark.parametrize("dim,N", K.KERNEL_CASES)
def test_every_mutant_leaves_the_bound(dim, N):
    P = L.limiter_operators_hp(N)["P"].astype(np.float64)
    faces = K.ghost_faces(dim)
    for nv in (5, 1, 2):
        for nc, kind, u in K.inputs(dim, N, nv):
            proj, absproj = L.project_grid(u, P), L.project_grid(np.abs(u), np.abs(P))
            ncell = int(np.prod(nc))
            seen = dict.fromkeys(MUTANTS_PATCH, 0.0)
            for cell in range(ncell):
                ref, bound = L.reference_patch(u, cell, P, proj=proj), K.projection_bound(u, cell, P, absproj=absproj)
                for m, mutant in MUTANTS_PATCH.items():
                    seen[m] = max(seen[m], K.worst_ratio(mutant(u, cell, P, proj), ref, bound))
            assert min(seen.values()) >= 100, (nv, nc, kind, seen)
            if nv != 5:
                continue
            # the ghost-layer test: a buffer on the wrong face, or applied to cells that are not at the block face, is as visible
            gh = K.ghost_buffers(dim, N, nc, nv, faces)
            swapped = {(a, 1 - side): g for (a, side), g in gh.items()}
            r = max(K.worst_ratio(L.reference_patch(u, c, P, swapped, proj=proj), L.reference_patch(u, c, P, gh, proj=proj),
                                  K.projection_bound(u, c, P, gh, absproj=absproj)) for c in range(ncell))
            assert r >= 100, (nc, kind, "ghost faces swapped", r)
            for d in range(dim):
                for side in (0, 1):
                    ref, bound = L.reference_face_layers(u, d, side, P), K.face_bound(u, d, side, P)
                    for m, mutant in MUTANTS_FACE.items():
                        if m == "transposed" and dim == 2:
                            continue                              # (one transverse axis: nothing to transpose)
                        if m == "side_swapped" and nc[d] == 1:
                            continue                              # (one cell along d: both block faces belong to it)
                        r = K.worst_ratio(mutant(u, d, side, P), ref, bound)
                        assert r >= 100, (nc, kind, d, side, m, r)

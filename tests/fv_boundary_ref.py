"""The reference restatement of a FV patch grid step with boundary conditions (FVPatchGrid(boundary={...}), exa_fv_grid_step_device_bc), shared by
tests/test_fv_boundary_host.py and tests/test_fv_boundary_gpu.py.

As oracle/fv_reference.py grid_update: the halo-less patches are assembled into ONE global array (`assemble`), the array is padded by one layer in
long double, and the reference's block update runs on it.  The pad of a domain face follows the face's kind (include/exahype_hip.h EXA_FV_FACE_*):
the wrap (periodic), the face's state, or the sign times the array's own first / last layer (mirror).  A product with +-1 is exact, so the bound
E of the block update is the bound of the step, as for the periodic grid.  Edge and corner pads are not read by the 2 dim + 1-point stencil.
"""
import numpy as np

from oracle import fv_reference as R

PERIODIC, STATE, MIRROR = 0, 1, 2
LD = R.LD


def padded(G, dim, kinds, data):
    """G [n0, .., V] (long double) -> [n0 + 2, .., V]: wrap, then every face that is not periodic by its kind (axes in order)"""
    A = np.pad(G, [(1, 1)] * dim + [(0, 0)], mode="wrap")
    for a in range(dim):
        for side in range(2):
            f = a * 2 + side
            if kinds[f] == PERIODIC:
                continue
            idx, src = [slice(None)] * (dim + 1), [slice(None)] * (dim + 1)
            idx[a] = 0 if side == 0 else A.shape[a] - 1
            src[a] = 1 if side == 0 else A.shape[a] - 2
            row = np.asarray(data[f], dtype=np.float64).astype(A.dtype)
            if kinds[f] == STATE:
                A[tuple(idx)] = row
            else:
                assert kinds[f] == MIRROR and np.all(np.abs(row) == 1)
                A[tuple(idx)] = row * A[tuple(src)]
    return A


def faces_of(boundary, dim, n_real, n_aux, pde):
    """(kinds, data) of a FVPatchGrid boundary argument: None, a dict of states for all faces, or a dict of conditions"""
    from exahype_amd.boundary import Dirichlet, Outflow, Wall, fv_faces
    V = n_real + n_aux
    if boundary is None:
        return [PERIODIC] * (2 * dim), np.zeros((2 * dim, V))
    if not any(isinstance(b, (Outflow, Wall, Dirichlet)) for b in boundary.values()) and len(boundary) == 2 * dim:
        return [STATE] * (2 * dim), np.stack([np.broadcast_to(np.asarray(boundary[(a, s)], dtype=np.float64), (V,)) for a in range(dim) for s in range(2)])
    kinds, data, _ = fv_faces(boundary, dim, n_real, n_aux, 1 if pde == R.PDE_EULER else 2)
    return kinds, data


def grid_update(U, dt, h, dim, n_real, pde, kinds, data, prim=R.IEEE, track=True):
    """R.grid_update with a kind per domain face -> Result(new [as U, long double], M, E [g.., P.., n_real])"""
    U = np.asarray(U)
    grid, P = U.shape[:dim], U.shape[dim]
    G = R.assemble(U, dim).astype(LD)
    A = padded(G, dim, kinds, data)
    new_i, M, E = R._update_block(A[None], dt, h, dim, n_real, pde, prim, None, track)
    Gn = G.copy()
    Gn[..., :n_real] = new_i[0]
    return R.Result(R.cut_patches(Gn, dim, grid, P), R.cut_patches(M[0], dim, grid, P), R.cut_patches(E[0], dim, grid, P))


def user_grid_update(U, dt, h, dim, terms, kinds, data, centres=None, t=0.0, prim=R.IEEE, track=True):
    """R.user_grid_update (a generated term set) with a kind per domain face"""
    U = np.asarray(U)
    grid, P, m = U.shape[:dim], U.shape[dim], terms.m
    n = int(np.prod(grid))
    G = R.assemble(U, dim).astype(LD)
    A = padded(G, dim, kinds, data)
    glob = lambda x: R.assemble(x.reshape(grid + (P,) * dim + (1,)), dim)[None, ..., 0]     # noqa: E731
    X = [R._V(glob(x.v), glob(x.e) if track else None) for x in R.volume_centres(centres, n, dim, P, h, LD, track)]
    new_i, M, E = R._update_block_user(A[None], X, t, dt, h, dim, m, terms, prim, None, track)
    Gn = G.copy()
    Gn[..., :m] = new_i[0]
    return R.Result(R.cut_patches(Gn, dim, grid, P), R.cut_patches(M[0], dim, grid, P), R.cut_patches(E[0], dim, grid, P))


def lam_reference(U, kinds, data, dim, pde, prim):
    """tests/test_fv_kernels_hp.py _lam_reference with the STATE faces' states only: a mirror ghost has its interior twin's eigenvalue"""
    states = U.reshape(-1, U.shape[-1])
    st = [f for f in range(2 * dim) if kinds[f] == STATE]
    if st:
        states = np.concatenate([states, np.asarray(data)[st]])
    lam, e = [np.concatenate(x) for x in zip(*[R.max_eigenvalue(states, d, pde, prim) for d in range(dim)])]
    top = int(np.argmax(lam))
    can_win = lam + R.U53 * e >= lam[top] - R.U53 * e[top]
    return lam[top], np.max(e[can_win])

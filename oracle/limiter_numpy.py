"""ORACLE (test infrastructure only -- never imported by the product path).

FV subcell limiter glue of BASELINE configs[4]: projection of a DG cell onto
N_s = 2p+1 equal subcells per axis, constrained least-squares reconstruction, and the limited step
(troubled cells take the FV Rusanov patch update of their projected data instead of the DG result).

Reference anchor: none -- /root/reference holds no limiter; "parity unpinned".  The FV
patch update used inside IS the reference's kernel shape (`Unit test/test.cpp`, corrected form).
Pinned by the identities in tests/test_limiter.py (R P = I on degree <= p data, mean preservation).
P and R are pinned to the mpmath operators of oracle/limiter_reference.py (tests/test_limiter_reference.py).
"""
import numpy as np

from .dg_operators import gauss_legendre_01, lagrange_eval


def projection_matrix(xi, Ns):
    """P[s][i] = N_s * int_{s/N_s}^{(s+1)/N_s} phi_i  (Gauss-Legendre on every subinterval: exact)."""
    N = len(xi)
    g, gw = gauss_legendre_01(N)
    P = np.zeros((Ns, N))
    for s in range(Ns):
        for k in range(N):
            x = (s + g[k]) / Ns
            P[s] += gw[k] * lagrange_eval(xi, x)
    return P


def reconstruction_matrix(P, w):
    """R = argmin ||P u - v||^2  s.t.  w.u = mean(v)   (KKT system), as a matrix N x N_s."""
    Ns, N = P.shape
    K = np.zeros((N + 1, N + 1))
    K[:N, :N] = 2 * P.T @ P
    K[:N, N] = w
    K[N, :N] = w
    rhs = np.zeros((N + 1, Ns))
    rhs[:N] = 2 * P.T
    rhs[N] = 1.0 / Ns
    return np.linalg.solve(K, rhs)[:N]


def apply_all_axes(M, a, dim, first_axis):
    for d in range(dim):
        a = np.moveaxis(np.tensordot(M, a, axes=([1], [first_axis + d])), 0, first_axis + d)
    return a


def build_patch(proj, idx, bcs=None):
    """patch [(Ns + 2).., V] of cell idx from the projected state proj [grid.., Ns.., V]: interior, face halos = the adjacent subcell layer of the
    face neighbours (periodic; at a domain face with a condition the cell's own adjacent layer, times the sign for a wall), edges / corners =
    nearest interior value (never read).  bcs: {(axis, side): ("outflow",) | ("wall", sign[V])}; a face not named is periodic."""
    dim = (proj.ndim - 1) // 2
    Ns = proj.shape[dim]
    S = Ns + 2
    bcs = bcs or {}
    patch = np.pad(proj[idx], [(1, 1)] * dim + [(0, 0)], mode="edge")
    for a in range(dim):
        for side, off in ((0, -1), (1, +1)):
            sl = [slice(1, -1)] * dim
            sl[a] = 0 if side == 0 else S - 1
            bc = bcs.get((a, side))
            if bc is not None and idx[a] == (0 if side == 0 else proj.shape[a] - 1):
                layer = np.take(proj[idx], 0 if side == 0 else Ns - 1, axis=a)
                if bc[0] == "wall":
                    layer = layer * np.asarray(bc[1])
                elif bc[0] != "outflow":
                    raise ValueError(bc[0])
            else:
                nb = list(idx)
                nb[a] = (nb[a] + off) % proj.shape[a]
                layer = np.take(proj[tuple(nb)], Ns - 1 if side == 0 else 0, axis=a)
            patch[tuple(sl)] = layer
    return patch


def replace_troubled(u, cand, mask, dt, dx, ops, fv, bcs=None):
    """cand with the cells of mask[grid..] replaced: u (own + face neighbours' boundary layers, build_patch) projected onto subcells, one
    update fv(patch[S.., m], dt, h) -> patch with h = dx / N_s, reconstructed."""
    dim = (u.ndim - 1) // 2
    Ns = 2 * ops["N"] - 1
    P = projection_matrix(ops["xi"], Ns)
    R = reconstruction_matrix(P, ops["w"])
    out = cand.copy()
    if not mask.any():
        return out
    proj = apply_all_axes(P, u, dim, dim)                                  # [grid.., Ns.., m]
    core = (slice(1, -1),) * dim
    for idx in zip(*np.nonzero(mask)):
        patch = fv(build_patch(proj, idx, bcs), dt, dx[0] / Ns)
        out[idx] = apply_all_axes(R, patch[core], dim, 0)
    return out


def limited_step(u, mask, dt, dx, ops, pde, fv_update, n_it=None):
    """One step of the limited scheme on a periodic grid.
    u[grid.., nodes.., m]; mask[grid..] bool (troubled); fv_update(patch[S..,m], dt, h) -> patch (in place semantics).
    Untroubled cells: ADER-DG step.  Troubled cells: replace_troubled from u^n."""
    from . import aderdg_numpy as A
    dim = (u.ndim - 1) // 2
    if max(dx[:dim]) - min(dx[:dim]) > 1e-12 * max(dx[:dim]):         # one volume size per patch update: as solvers.SubcellLimiter, refuse what would be silently wrong
        raise ValueError("limited_step: the FV patch update takes one volume size, dx = %s" % (list(dx),))
    return replace_troubled(u, A.step(u, dt, dx, ops, pde, n_it), np.asarray(mask), dt, dx, ops, fv_update)

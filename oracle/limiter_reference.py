"""ORACLE (test infrastructure only -- never imported by the product path).

Long-double reference of the FV subcell limiter glue (exahype_amd/csrc/limiter.hip; include/exahype_hip.h "FV subcell limiter glue"):
the operators P, R from closed forms in mpmath, and the three things the kernels produce -- the FV patch with halo of one cell, the
face layers of a block face, the reconstruction -- as plain tensor products in np.longdouble.

Reference anchor: none -- the reference project holds no limiter.  Pinned by the identities of
tests/test_limiter_reference.py, which also pins the fp64 oracle (oracle/limiter_numpy.py) to it.

mpmath is needed only by limiter_operators_hp / write_operators_file.  GPU tests read the committed
tests/golden/limiter_operators_hp.json through load_operators_file instead (plain json + np.longdouble).

The reference rests on np.longdouble carrying more digits than fp64 (64-bit significand on x86-64): checked at import.
"""
import json
import os

import numpy as np

from .limiter_numpy import apply_all_axes

LD = np.longdouble
DIGITS = 40                                     # significant decimal digits per entry in the operator file
OPERATORS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "limiter_operators_hp.json")
ORDERS = tuple(range(2, 9))                     # the N limiter.hip is instantiated for (EXA_LIM_CASES)

assert np.finfo(LD).eps < 2.0 ** -60, "np.longdouble is no wider than fp64 here: the reference would round like the code it judges"

_HP_STRINGS = {}
_HP_CACHE = {}


def _operator_strings(N, dps=60):
    """P, R and cond_2(K) of order N as decimal strings of DIGITS digits (computed at `dps` digits).

    P[s][i] = N_s * int_{s/N_s}^{(s+1)/N_s} phi_i: phi_i multiplied out into monomial coefficients, integrated term by term.
    R: the KKT system of oracle.limiter_numpy.reconstruction_matrix, [2 P^T P, w; w^T, 0] [R; lambda] = [2 P^T; 1/N_s], by mpmath's LU."""
    if N in _HP_STRINGS:
        return _HP_STRINGS[N]
    import mpmath
    from .dg_operators import gauss_legendre_mp
    Ns = 2 * N - 1
    with mpmath.workdps(dps):
        mp = mpmath.mpf
        xs, ws = gauss_legendre_mp(N, dps)
        P = mpmath.matrix(Ns, N)
        for i in range(N):
            c = [mp(1)]                                            # coefficients of phi_i, lowest degree first
            for k in range(N):
                if k == i:
                    continue
                d = xs[i] - xs[k]
                c = [((c[j - 1] if j > 0 else 0) - xs[k] * (c[j] if j < len(c) else 0)) / d for j in range(len(c) + 1)]
            prim = lambda x: sum(c[j] * x ** (j + 1) / (j + 1) for j in range(N))
            for s in range(Ns):
                P[s, i] = Ns * (prim(mp(s + 1) / Ns) - prim(mp(s) / Ns))
        K = mpmath.matrix(N + 1, N + 1)
        rhs = mpmath.matrix(N + 1, Ns)
        PtP = P.T * P
        for i in range(N):
            for j in range(N):
                K[i, j] = 2 * PtP[i, j]
            K[i, N] = K[N, i] = ws[i]
            for s in range(Ns):
                rhs[i, s] = 2 * P[s, i]
        for s in range(Ns):
            rhs[N, s] = mp(1) / Ns
        X = mpmath.matrix(N + 1, Ns)
        for s in range(Ns):
            X[:, s] = mpmath.lu_solve(K, rhs[:, s])
        sv = mpmath.svd_r(K, compute_uv=False)
        cond = max(sv) / min(sv)
        f = lambda v: mpmath.nstr(v, DIGITS, strip_zeros=False)
        out = dict(P=[[f(P[s, i]) for i in range(N)] for s in range(Ns)], R=[[f(X[i, s]) for s in range(Ns)] for i in range(N)],
                   w=[f(v) for v in ws], condK=f(cond))
    _HP_STRINGS[N] = out
    return out


def _from_strings(N, d):
    arr = lambda a: np.array([[LD(v) for v in row] for row in a], dtype=LD)           # decimal string -> correctly rounded long double
    return dict(N=N, Ns=2 * N - 1, P=arr(d["P"]), R=arr(d["R"]), w=np.array([LD(v) for v in d["w"]], dtype=LD), condK=float(d["condK"]))


def limiter_operators_hp(N):
    """dict(N, Ns, P[2N-1][N], R[N][2N-1], w[N], condK) in np.longdouble (condK: float, the 2-norm condition number of the KKT matrix),
    built in mpmath; cached per N."""
    if N not in _HP_CACHE:
        _HP_CACHE[N] = _from_strings(N, _operator_strings(N))
    return _HP_CACHE[N]


def operators_file_content():
    return dict(digits=DIGITS, orders={str(N): _operator_strings(N) for N in ORDERS})


def write_operators_file(path=OPERATORS_FILE):
    """(Re)write tests/golden/limiter_operators_hp.json: python -c "from oracle.limiter_reference import *; write_operators_file()"."""
    with open(path, "w") as f:
        json.dump(operators_file_content(), f, indent=0, sort_keys=True)
        f.write("\n")


def load_operators_file(path=OPERATORS_FILE):
    """{N: dict as limiter_operators_hp(N)} from the committed file -- no mpmath."""
    with open(path) as f:
        d = json.load(f)
    return {int(N): _from_strings(int(N), v) for N, v in d["orders"].items()}


def operator_tolerance(condK):
    """What an fp64 construction of P and R is held to, entry by entry (entries are O(1)): 8 ulp(1)/2 times the condition number of the KKT
    system it solves."""
    return 8 * 2.0 ** -53 * condK


# ---- what the kernels compute -----------------------------------------------------------------------------------------------------------

def _grid(u, P):
    u = np.asarray(u)
    dim = (u.ndim - 1) // 2
    assert u.ndim == 2 * dim + 1 and all(n == P.shape[1] for n in u.shape[dim:2 * dim]), (u.shape, P.shape)
    return dim, u.shape[:dim]


def project_grid(u, P):
    """(P x .. x P) u for every cell: u[grid.., N.., nv] -> [grid.., N_s.., nv] in long double."""
    dim, _ = _grid(u, P)
    return apply_all_axes(np.asarray(P, dtype=LD), np.asarray(u, dtype=LD), dim, dim)


def transverse_index(cc, nc, a):
    """Index of a cell in the [transverse cell] axis of a face buffer of direction a: row-major over the axes != a."""
    tc = 0
    for b in range(len(nc)):
        if b != a:
            tc = tc * nc[b] + cc[b]
    return tc


def face_slice(dim, Ns, a, side):
    """Index of the face halo (a, side) of a patch [(N_s+2)..][nv]: halo layer along a, interior along the other axes."""
    sl = [slice(1, -1)] * dim
    sl[a] = Ns + 1 if side else 0
    return tuple(sl)


def reference_patch(u, cell, P, ghosts=None, proj=None):
    """The FV patch [(N_s+2)..][nv] (long double) exa_dg_project_patches(_ghost) builds for `cell` (flat row-major index or index tuple) of
    the block u[grid.., N.., nv]: interior = projected cell; face halo (a, side) = the subcell layer of the projected face neighbour that
    touches the face, periodic in the block -- or, where ghosts[(a, side)] ([transverse cell][N_s^(dim-1)][nv]) is given and the cell lies at
    that block face, the cell's entry of it; edge and corner entries = nearest interior value.
    proj: project_grid(u, P) if the caller has it already."""
    dim, nc = _grid(u, P)
    Ns = P.shape[0]
    cc = tuple(int(c) for c in (np.unravel_index(cell, nc) if np.ndim(cell) == 0 else cell))
    if proj is None:
        proj = project_grid(u, P)
    own = proj[cc]
    nv = own.shape[-1]
    patch = np.pad(own, [(1, 1)] * dim + [(0, 0)], mode="edge")  # every halo entry: nearest interior value; the faces follow
    for a in range(dim):
        for side in (0, 1):
            g = None if ghosts is None else ghosts.get((a, side))
            if g is not None and cc[a] == (nc[a] - 1 if side else 0):
                layer = np.asarray(g, dtype=LD).reshape(-1, Ns ** (dim - 1), nv)[transverse_index(cc, nc, a)].reshape((Ns,) * (dim - 1) + (nv,))
            else:
                nb = list(cc)
                nb[a] = (nb[a] + (1 if side else -1)) % nc[a]
                layer = np.take(proj[tuple(nb)], 0 if side else Ns - 1, axis=a)
            patch[face_slice(dim, Ns, a, side)] = layer
    return patch


def boundary_cell_layers(u, d, at, row, P):
    """Subcell layer `row` along axis d of the projections of the cells with index `at` along d: [transverse cell][N_s^(dim-1)][nv],
    transverse cells and transverse subcells row-major over the axes != d."""
    dim, _ = _grid(u, P)
    cells = np.take(np.asarray(u, dtype=LD), at, axis=d)         # [transverse grid.., N.., nv]
    proj = apply_all_axes(np.asarray(P, dtype=LD), cells, dim, dim - 1)
    layer = np.take(proj, row, axis=dim - 1 + d)                 # [transverse grid.., transverse N_s.., nv]
    return layer.reshape(-1, P.shape[0] ** (dim - 1), np.shape(u)[-1])


def reference_face_layers(u, d, side, P):
    """exa_lim_face_layers: out[transverse cell][N_s^(dim-1)][nv] (long double), for every cell of the block's boundary layer at face
    (d, side) its projected subcell layer next to that face (subcell 0 at side 0, N_s - 1 at side 1)."""
    _, nc = _grid(u, P)
    return boundary_cell_layers(u, d, nc[d] - 1 if side else 0, P.shape[0] - 1 if side else 0, P)


def reference_reconstruct(patch, R):
    """exa_dg_reconstruct_patches for one patch [(N_s+2)..][nv]: (R x .. x R) applied to the interior -> [N..][nv] (long double)."""
    dim = np.ndim(patch) - 1
    return apply_all_axes(np.asarray(R, dtype=LD), np.asarray(patch, dtype=LD)[(slice(1, -1),) * dim], dim, 0)


def rounding_factor(dim, C):
    """An fp64 tensor product of `dim` passes with contraction length C lies within rounding_factor * B of the exact one, element by element,
    B = (|M| x .. x |M|) |input|: every pass is a sum of C products, (C + 1) roundings of relative size 2^-53 at most per term."""
    return dim * (C + 1) * 2.0 ** -53

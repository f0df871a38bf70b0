"""Long-double restatement of the second-order MUSCL-Hancock patch update (EXA_FV_MUSCL_HANCOCK) -- TEST INFRASTRUCTURE ONLY.

Written from the five statements of the scheme in vectorised numpy, not from exahype_amd/csrc/exa_fv_muscl.hpp.  On a patch array
Q[patch][S..][V] (S = P + 2 H, H >= 2), evolved variables v < n_real, r = dt / h:

  1. slopes       s_e(c) = minmod(Q_c - Q_{c-e}, Q_{c+e} - Q_c) for every axis e; minmod(a, b) is the one of smaller magnitude if both are > 0 or
                  both are < 0, else 0 (decided by the signs, a NaN difference gives 0).  Auxiliary variables are not reconstructed.
  2. predictor    delta_c = -(r/2) sum_e [f_e(Q_c + s_e/2) - f_e(Q_c - s_e/2)]
  3. face states  w_c^{+-d} = (Q_c +- s_d(c)/2) + delta_c
  4. face flux    F*_{c+1/2,d} = (f_d(w_L) + f_d(w_R))/2 - max(l_d(w_L), l_d(w_R))/2 (w_R - w_L),  w_L = w_c^{+d}, w_R = w_{c+e_d}^{-d}
  5. update       Q_c <- Q_c - r sum_d (F*_{c+1/2,d} - F*_{c-1/2,d}) for the evolved variables of the interior volumes; halo layers and auxiliary
                  variables are returned untouched.

update() returns Result(new, M, E) as oracle/fv_reference.py does: the new state in long double, the magnitude M (the update with every
product and sum over absolute values: |Q_c| + |r| sum_faces (1/2 (|F|_L + |F|_R) + 1/2 s (|w_R| + |w_L|))) and the rounding bound E of an fp64
evaluation in units of 2^-53.  E follows the rules of oracle/fv_reference.py (its _V, _add, _mul, _exact, _max, _terms, _sum_any_order and
UserTerms are imported, the module is untouched): every fp64 operation adds |result| to the bound its operands carry, a factor 1/2 or a sign
adds nothing, dt / h carries its own rounding, the term sets use IEEE division and square root.  Two rules are added:

  minmod     carries max(e_a, e_b): it is the median of (a, b, 0), and the median is 1-Lipschitz in the max norm -- whichever branch the fp64
             evaluation takes, its result is within max(e_a, e_b) of the exact one.
  axis sums  the sums over the axes (in delta and in the update) are counted with the association-free rule (_sum_any_order: every partial
             sum is at most sum |a_i|), so a kernel may add the axes in any order.

The count, statement by statement: a difference Q_c - Q_{c-e} 1; Q_c +- s/2 1 more; the flux's own count on top; f(+) - f(-) 1; the axis sum; the
product with -(r/2) (r's rounding and the product's); (Q_c +- s/2) + delta 1; the Rusanov flux as in oracle/fv_reference.py (sum of the two
fluxes 1, w_R - w_L 1, product with max/2 1, difference 1); F*_+ - F*_- 1; the axis sum; the product with r and the last subtraction.  Nothing here
is taken from what a kernel gives.  A result is accepted when |got - new| <= 2^-53 E for every evolved interior value.

grid_update() applies the same statements to ONE global array whose two ghost layers come from the product's own numpy halo fill of a
1 x 1 (x 1) "grid" holding the whole domain (periodic wrap, prescribed states, Outflow / Wall / Dirichlet faces in the order
fill_halos_boundary defines).

MUTANTS, each a single change: forward_slope (slope = forward difference, no minmod), slope_not_halved, delta_zero, delta_full_r (r in place of
r/2), delta_normal_only (the face states of axis d take the predictor of axis d alone), swap_w (w^- in place of w^+ as the left state of
every face), halo2_from_halo1 (the second halo layer read from the first), edge_from_face (an edge entry replaced by the nearest face-halo
entry), aux_reconstructed (the auxiliary variables get slopes and a predictor too).
"""
import collections

import numpy as np

from oracle import fv_reference as R
from oracle.fv_reference import UserTerms, _V, _add, _exact, _max, _mul, _sum_any_order, _terms  # noqa: F401

LD = np.longdouble
U53 = R.U53
MUTANTS = ("forward_slope", "slope_not_halved", "delta_zero", "delta_full_r", "delta_normal_only", "swap_w", "halo2_from_halo1",
           "edge_from_face", "aux_reconstructed")
Result = collections.namedtuple("Result", "new M E")


def mutant_exemption(mutant, dim, pde, n_aux=0):
    """None when the mutant applies to such a row, else the reason it cannot."""
    if mutant == "aux_reconstructed":
        return ("the flux and eigenvalue of every term set here read the evolved variables alone (the kernels hand them no auxiliary value), so "
                "face states whose auxiliary part was reconstructed give the same evolved values; what it would break -- auxiliary values "
                "written -- is the bit-equality check of the auxiliary variables, not the bound")
    return None


def _take(x, have, lo, hi):
    """x covers the window minus `have` layers on every side of every spatial axis (axes 1 .. dim of x); -> the part that leaves lo[a] / hi[a]
    layers of the WINDOW out on the low / high side of axis a"""
    idx = [slice(None)] * x.ndim
    for a in range(len(lo)):
        n = x.shape[1 + a]
        idx[1 + a] = slice(lo[a] - have, n - (hi[a] - have))
    return x[tuple(idx)]


def _takev(x, have, lo, hi):
    return _V(_take(x.v, have, lo, hi), None if x.e is None else _take(x.e, have, lo, hi))


def _minmod(a, b, forward=False):
    if forward:
        return b
    with np.errstate(invalid="ignore"):
        pos, neg = (a.v > 0) & (b.v > 0), (a.v < 0) & (b.v < 0)
        v = np.where(pos, np.minimum(a.v, b.v), np.where(neg, np.maximum(a.v, b.v), 0))
    return _V(v.astype(a.v.dtype), None if a.e is None else np.maximum(a.e, b.e))


def _eval(q, dim, pde, terms, prim):
    """flux F[d][v], eigenvalue lam[d] (_V) and |F|[d][v] of the states q (list of _V) for a built-in term set or UserTerms"""
    if terms is None:
        return _terms(q, dim, pde, prim, None)
    T = q[0].v.dtype.type
    z = _V(np.zeros_like(q[0].v), None if q[0].e is None else np.zeros_like(q[0].v))
    F, lam, Fabs = [], [], []
    for d in range(dim):
        f = terms.flux(q, [z, z, z], _V(np.full_like(q[0].v, T(0)), z.e), d, prim)
        F.append([x[0] for x in f])
        Fabs.append([x[1] for x in f])
        lam.append(terms.eig(q, [z, z, z], _V(np.full_like(q[0].v, T(0)), z.e), d, prim))
    return F, lam, Fabs


def _mutate_input(A, dim, mutant):
    """the mutants that change what is read: A is the window [n, (n_a + 4).., V]"""
    if mutant == "halo2_from_halo1":
        A = A.copy()
        for a in range(dim):
            lo, hi, l1, h1 = ([slice(None)] * A.ndim for _ in range(4))
            n = A.shape[1 + a]
            lo[1 + a], l1[1 + a], hi[1 + a], h1[1 + a] = 0, 1, n - 1, n - 2
            A[tuple(lo)] = A[tuple(l1)]
            A[tuple(hi)] = A[tuple(h1)]
    elif mutant == "edge_from_face":
        B = A.copy()
        for a in range(dim):
            for b in range(a + 1, dim):
                for sa in (0, 1):
                    for sb in (0, 1):
                        dst, src = [slice(None)] * A.ndim, [slice(None)] * A.ndim
                        na, nb = A.shape[1 + a], A.shape[1 + b]
                        dst[1 + a] = 1 if sa == 0 else na - 2
                        dst[1 + b] = 1 if sb == 0 else nb - 2
                        src[1 + a] = 2 if sa == 0 else na - 3          # the nearest interior coordinate along a: a face-halo entry of axis b
                        src[1 + b] = dst[1 + b]
                        B[tuple(dst)] = A[tuple(src)]
        A = B
    return A


def update_block(A, dt, h, dim, m, pde=R.PDE_EULER, terms=None, prim=R.IEEE, mutant=None, track=True):
    """A [n, n_0 + 4, .., n_{dim-1} + 4, V] (long double: the reference; fp64 with track=False: an fp64 evaluation of the same statements): the
    update of every volume that has two neighbours on either side along every axis -> (new [n, n_0, .., m], M, E)."""
    assert mutant is None or mutant in MUTANTS, mutant
    A = _mutate_input(A, dim, mutant)
    T = A.dtype.type
    nvar = A.shape[-1] if mutant == "aux_reconstructed" else m
    q = [_V(np.ascontiguousarray(A[..., v]), np.zeros(A.shape[:-1], dtype=A.dtype) if track else None) for v in range(nvar)]
    one, two = [1] * dim, [2] * dim
    r = T(dt) / T(h)
    rV = lambda like, c: _V(np.full_like(like.v, c * r), None if not track else np.full_like(like.v, abs(c * r)))     # noqa: E731  (c r: r's one rounding)
    half = 1.0 if mutant == "slope_not_halved" else 0.5
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # 1. slopes on the window minus one layer (its corners are computed and never used)
        q1 = [_takev(x, 0, one, one) for x in q]
        s = []
        for e in range(dim):
            lo, hi = list(one), list(one)
            lo[e], hi[e] = 0, 2
            qm = [_takev(x, 0, lo, hi) for x in q]
            lo[e], hi[e] = 2, 0
            qp = [_takev(x, 0, lo, hi) for x in q]
            s.append([_minmod(_add(q1[v], qm[v], -1), _add(qp[v], q1[v], -1), forward=mutant == "forward_slope") for v in range(nvar)])
        # 2. predictor: per axis the flux difference of the two extrapolated states, then the sum over the axes
        diff = []
        for e in range(dim):
            wp = [_add(q1[v], _exact(s[e][v], half)) for v in range(nvar)]
            wm = [_add(q1[v], _exact(s[e][v], half), -1) for v in range(nvar)]
            Fp, Fm = _eval(wp[:m], dim, pde, terms, prim)[0][e], _eval(wm[:m], dim, pde, terms, prim)[0][e]
            diff.append([_add(Fp[v], Fm[v], -1) for v in range(m)])

        def delta(axes):
            if mutant == "delta_zero":
                return [_V(np.zeros_like(q1[0].v), None if not track else np.zeros_like(q1[0].v)) for _ in range(m)]
            c = -1.0 if mutant == "delta_full_r" else -0.5
            out = []
            for v in range(m):
                ts = [diff[e][v] for e in axes]
                out.append(_mul(rV(q1[0], c), ts[0] if len(ts) == 1 else _sum_any_order(ts)))
            return out
        dl_all = delta(range(dim))
        # 3. - 5.
        qc = [_takev(x, 0, two, two) for x in q[:m]]
        terms_d, mag = [], [0] * m
        for d in range(dim):
            dl = delta([d]) if mutant == "delta_normal_only" else dl_all
            lo, hi = list(two), list(two)
            lo[d], hi[d] = 1, 1                                       # the interior and one more volume on either side along d
            qe = [_takev(q1[v], 1, lo, hi) for v in range(m)]
            se = [_takev(s[d][v], 1, lo, hi) for v in range(m)]
            de = [_takev(dl[v], 1, lo, hi) for v in range(m)]
            wplus = [_add(_add(qe[v], _exact(se[v], half)), de[v]) for v in range(m)]
            wminus = [_add(_add(qe[v], _exact(se[v], half), -1), de[v]) for v in range(m)]

            def along(x, a, b):                                      # volumes a .. n - b of the extended range along d
                idx = [slice(None)] * x.v.ndim
                idx[1 + d] = slice(a, x.v.shape[1 + d] - b)
                return _V(x.v[tuple(idx)], None if x.e is None else x.e[tuple(idx)])
            wL = [along(x, 0, 1) for x in (wminus if mutant == "swap_w" else wplus)]
            wR = [along(x, 1, 0) for x in wminus]
            FL, lL, FLa = _eval(wL, dim, pde, terms, prim)
            FR, lR, FRa = _eval(wR, dim, pde, terms, prim)
            lam = _max(lL[d], lR[d])
            face = [_add(_exact(_add(FL[d][v], FR[d][v]), 0.5), _mul(_exact(lam, 0.5), _add(wR[v], wL[v], -1)), -1) for v in range(m)]
            terms_d.append([_add(along(face[v], 1, 0), along(face[v], 0, 1), -1) for v in range(m)])
            if track:
                for v in range(m):
                    fm = 0.5 * (FLa[d][v] + FRa[d][v]) + 0.5 * lam.v * (np.abs(wR[v].v) + np.abs(wL[v].v))
                    idx_p, idx_m = [slice(None)] * fm.ndim, [slice(None)] * fm.ndim
                    idx_p[1 + d], idx_m[1 + d] = slice(1, None), slice(0, -1)
                    mag[v] = mag[v] + fm[tuple(idx_p)] + fm[tuple(idx_m)]
        new, M, E = [], [], []
        for v in range(m):
            ts = [terms_d[d][v] for d in range(dim)]
            out = _add(qc[v], _mul(rV(qc[v], 1.0), _sum_any_order(ts)), -1)
            new.append(out.v)
            M.append(np.abs(qc[v].v) + abs(r) * mag[v] if track else np.zeros_like(out.v))
            E.append(out.e if track else np.zeros_like(out.v))
    return np.stack(new, -1), np.stack(M, -1), np.stack(E, -1)


def interior(dim, P, H):
    return R.interior(dim, P, H)


def update(Q, dt, h, dim, P, H, n_real, n_aux=0, pde=R.PDE_EULER, terms=None, prim=R.IEEE, mutant=None, track=True, dtype=LD):
    """Q [n_patches, S.., n_real + n_aux] (S = P + 2 H, H >= 2) -> Result(new [as Q], M, E [n_patches, P.., n_real]).  dtype=np.float64 with
    track=False evaluates the same statements in fp64."""
    Q = np.asarray(Q)
    S = P + 2 * H
    assert H >= 2 and Q.shape[1:] == (S,) * dim + (n_real + n_aux,), Q.shape
    A = Q[(slice(None),) + (slice(H - 2, H + P + 2),) * dim].astype(dtype)
    new_i, M, E = update_block(A, dt, h, dim, n_real, pde, terms, prim, mutant, track)
    new = Q.astype(dtype)
    new[interior(dim, P, H) + (slice(0, n_real),)] = new_i
    return Result(new, M, E)


def global_with_ghosts(G, dim, boundary=None, conditions=None):
    """The global array G [N_0, .., V] with two ghost layers: the product's own halo fill (numpy) of a 1 x 1 (x 1) grid whose one patch is the
    whole domain -- periodic wrap, prescribed states (boundary: one state or {(axis, side): state}) or boundary conditions (conditions:
    {(axis, side): Outflow | Wall | Dirichlet | state}).  Only cubic domains have a patch form; others are padded axis by axis the same way."""
    from exahype_amd.boundary import Dirichlet, Outflow, Wall
    A = np.pad(np.asarray(G), [(2, 2)] * dim + [(0, 0)])
    V = A.shape[-1]
    for a in range(dim):
        n = A.shape[a]
        at = lambda layers: tuple(layers if x == a else slice(None) for x in range(A.ndim))      # noqa: E731
        A[at(slice(0, 2))] = A[at(slice(n - 4, n - 2))]
        A[at(slice(n - 2, n))] = A[at(slice(2, 4))]
        for side in range(2):
            bc = None
            if conditions is not None:
                bc = conditions.get((a, side))
            elif boundary is not None:
                bc = boundary[(a, side)] if isinstance(boundary, dict) else boundary
            if bc is None:
                continue
            halo = slice(0, 2) if side == 0 else slice(n - 2, n)
            inner = slice(2, 4) if side == 0 else slice(n - 4, n - 2)
            if isinstance(bc, (Outflow, Wall)):
                sign = np.ones(V)
                if isinstance(bc, Wall):
                    sign[:len(bc.sign)] = bc.sign
                A[at(halo)] = np.flip(A[at(inner)], axis=a) * sign
            else:
                A[at(halo)] = np.asarray(bc.state if isinstance(bc, Dirichlet) else bc, dtype=np.float64)
    return A


def grid_update(U, dt, h, dim, n_real, pde=R.PDE_EULER, terms=None, boundary=None, conditions=None, prim=R.IEEE, track=True, dtype=LD):
    """One step of a Cartesian grid of halo-less patches U [g.., P.., V] as ONE array -> Result(new [as U], M, E [g.., P.., n_real])."""
    U = np.asarray(U)
    grid, P = U.shape[:dim], U.shape[dim]
    G = R.assemble(U, dim)
    A = global_with_ghosts(G, dim, boundary, conditions).astype(dtype)
    new_i, M, E = update_block(A[None], dt, h, dim, n_real, pde, terms, prim, None, track)
    Gn = G.astype(dtype)
    Gn[..., :n_real] = new_i[0]
    return Result(R.cut_patches(Gn, dim, grid, P), R.cut_patches(M[0], dim, grid, P), R.cut_patches(E[0], dim, grid, P))


def ratio(got, res, sel=None):
    return R.ratio(got, res, sel)


def outside_stencil(dim, P, H):
    """boolean [S..]: the entries of a patch that no interior update reads -- everything but the interior, the two layers next to it along ONE
    axis (interior along the others) and the edge entries (layer 1 along exactly two axes, interior along the third)"""
    S = P + 2 * H
    co = np.indices((S,) * dim)
    dist = [np.where(co[a] < H, H - co[a], np.where(co[a] >= H + P, co[a] - (H + P) + 1, 0)) for a in range(dim)]      # layers outside the interior
    nz = sum((d > 0).astype(int) for d in dist)
    dmax = np.maximum.reduce(dist)
    read = (nz == 0) | ((nz == 1) & (dmax <= 2)) | ((nz == 2) & (dmax == 1))
    return ~read


# ---- the same statements in plain fp64 numpy: the form tests/test_fv_muscl_reference.py holds to the bound, and the runs behind
# ---- tests/golden/fv_muscl_runs.json
ADV64 = (1.0, 0.5, -0.75)
GM1_64 = np.float64(1.4) - np.float64(1.0)


def flux64(q, d, pde):
    """f_d of the states q [..., m] in fp64, in the order of the device's flux_rt"""
    if pde == R.PDE_ADVECTION:
        return ADV64[d] * q
    irho = 1.0 / q[..., 0]
    p = GM1_64 * (q[..., 4] - 0.5 * irho * (q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3]))
    coeff = irho * q[..., d + 1]
    F = np.zeros_like(q)
    F[..., :4] = coeff[..., None] * q[..., :4]
    F[..., 4] = coeff * q[..., 4] + coeff * p
    F[..., d + 1] += p
    return F


def eig64(q, d, pde):
    if pde == R.PDE_ADVECTION:
        return np.full(q.shape[:-1], abs(ADV64[d]))
    irho = 1.0 / np.abs(q[..., 0])
    p = GM1_64 * (q[..., 4] - 0.5 * irho * (q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3]))
    c = np.sqrt(np.float64(1.4) * np.abs(p) * irho)
    un = q[..., d + 1] * irho
    return np.maximum(np.abs(un - c), np.abs(un + c))


def _sh(x, a, k):
    """the value at c + k e_a (cyclic: what wraps around lies in the outer layers, which are cut away)"""
    return np.roll(x, -k, axis=1 + a)


def fp64_block(A, dt, h, dim, m, pde, scheme="muscl"):
    """the update of update_block() in plain fp64 on the whole window (rolls), cut to the volumes it is valid for -> new [n, n_0, .., m].
    scheme="rusanov": the first-order update of the same volumes, for the comparison runs."""
    q = np.ascontiguousarray(np.asarray(A)[..., :m], dtype=np.float64)
    r = np.float64(dt) / np.float64(h)
    cut = (slice(None),) + (slice(2, -2),) * dim

    def face_sum(wplus_of, wminus_of):
        tot = None
        for d in range(dim):
            wL, wR = wplus_of(d), _sh(wminus_of(d), d, 1)
            F = 0.5 * (flux64(wL, d, pde) + flux64(wR, d, pde)) - (0.5 * np.maximum(eig64(wL, d, pde), eig64(wR, d, pde)))[..., None] * (wR - wL)
            dd = F - _sh(F, d, -1)
            tot = dd if tot is None else tot + dd
        return tot
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if scheme == "rusanov":
            return (q - r * face_sum(lambda d: q, lambda d: q))[cut]
        s = []
        for e in range(dim):
            a, b = q - _sh(q, e, -1), _sh(q, e, 1) - q
            s.append(np.where((a > 0) & (b > 0), np.minimum(a, b), np.where((a < 0) & (b < 0), np.maximum(a, b), 0.0)))
        sumd = None
        for e in range(dim):
            dd = flux64(q + 0.5 * s[e], e, pde) - flux64(q - 0.5 * s[e], e, pde)
            sumd = dd if sumd is None else sumd + dd
        delta = (-0.5 * r) * sumd
        return (q - r * face_sum(lambda d: (q + 0.5 * s[d]) + delta, lambda d: (q - 0.5 * s[d]) + delta))[cut]


def fp64_update(Q, dt, h, dim, P, H, n_real, pde):
    """update() in plain fp64 -> new [as Q]"""
    Q = np.asarray(Q, dtype=np.float64)
    new = Q.copy()
    new[interior(dim, P, H) + (slice(0, n_real),)] = fp64_block(Q[(slice(None),) + (slice(H - 2, H + P + 2),) * dim], dt, h, dim, n_real, pde)
    return new


def run_global(G, t_end, h, dim, m, pde, cfl=0.4, scheme="muscl", conditions=None):
    """Advance the global array G [N.., V] (fp64) to t_end with dt = cfl h / (dim lambda_max) over the volumes -- the loop of FVPatchGrid.run;
    -> (G, steps)"""
    G = np.array(G, dtype=np.float64)
    t, steps = 0.0, 0
    while t < t_end * (1 - 1e-14):
        lam = max(float(np.max(eig64(G[..., :m], d, pde))) for d in range(dim))
        dt = min(cfl * h / dim / lam, t_end - t)
        A = global_with_ghosts(G, dim, conditions=conditions)[None]
        G[..., :m] = fp64_block(A, dt, h, dim, m, pde, scheme)[0]
        t += dt
        steps += 1
    return G, steps


# ---- the recorded runs (tests/golden/fv_muscl_runs.json; `python -m tests.fv_muscl_ref` rewrites the file) -------------------------------
def sine_advection(N):
    """q = sin(2 pi (x + y)) on the unit square, N x N volumes, advected with (1, 1/2): -> (G [N, N, 1], exact(t) [N, N])"""
    x = (np.arange(N) + 0.5) / N
    X, Y = np.meshgrid(x, x, indexing="ij")
    f = lambda t: np.sin(2 * np.pi * ((X - 1.0 * t) + (Y - 0.5 * t)))     # noqa: E731
    return f(0.0)[..., None], f


def density_wave(N, amp=0.5, vel=(1.0, 0.5)):
    """Euler: rho = 1 + 0.5 sin(2 pi (x + y)), velocity (1, 1/2, 0), p = 1 -- the density profile moves with the flow: -> (G [N, N, 5], exact rho(t))"""
    x = (np.arange(N) + 0.5) / N
    X, Y = np.meshgrid(x, x, indexing="ij")
    rho = lambda t: 1.0 + amp * np.sin(2 * np.pi * ((X - vel[0] * t) + (Y - vel[1] * t)))     # noqa: E731
    G = np.zeros((N, N, 5))
    G[..., 0] = rho(0.0)
    G[..., 1], G[..., 2] = G[..., 0] * vel[0], G[..., 0] * vel[1]
    G[..., 4] = 1.0 / 0.4 + 0.5 * G[..., 0] * (vel[0] ** 2 + vel[1] ** 2)
    return G, rho


def golden_runs():
    """the runs of the issue's table, by the fp64 form of the restatement at CFL 0.4"""
    from examples.sod_tube_fv_walls import initial_state, l1_density
    from exahype_amd.boundary import Wall, fv_faces
    out = {"cfl": 0.4, "advection": {}, "density_wave": {}}
    for N in (64, 128):
        for name, (G, exact), t_end, m, pde in (("advection", sine_advection(N), 0.5, 1, R.PDE_ADVECTION), ("density_wave", density_wave(N), 0.25, 5, R.PDE_EULER)):
            for scheme in ("muscl", "rusanov"):
                Gn, steps = run_global(G, t_end, 1.0 / N, 2, m, pde, 0.4, scheme)
                out[name]["%s_%d" % (scheme, N)] = {"l1": float(np.mean(np.abs(Gn[..., 0] - exact(t_end)))), "steps": steps}
    for name in ("advection", "density_wave"):
        for scheme in ("muscl", "rusanov"):
            out[name]["order_" + scheme] = float(np.log2(out[name][scheme + "_64"]["l1"] / out[name][scheme + "_128"]["l1"]))
    nx, P = 64, 4
    U = initial_state(nx, P)
    cond = fv_faces({(0, 0): Wall(), (0, 1): Wall()}, 2, 5, 0, R.PDE_EULER)[2]          # (the walls' signs resolved)
    out["sod"] = {"volumes": nx * P, "t_end": 0.1}
    for scheme in ("muscl", "rusanov"):
        Gn, steps = run_global(R.assemble(U, 2), 0.1, 1.0 / (nx * P), 2, 5, R.PDE_EULER, 0.4, scheme, conditions=cond)
        u = R.cut_patches(Gn, 2, (nx, 1), P)
        p = 0.4 * (u[..., 4] - 0.5 * (u[..., 1] ** 2 + u[..., 2] ** 2 + u[..., 3] ** 2) / u[..., 0])
        out["sod"][scheme] = {"l1": l1_density(u[..., 0], 0.1), "steps": steps, "min_rho": float(u[..., 0].min()), "min_p": float(p.min())}
    return out


if __name__ == "__main__":
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fv_muscl_runs.json")
    with open(path, "w") as f:
        json.dump(golden_runs(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(path).read())

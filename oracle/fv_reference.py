"""Long-double restatement of the corrected FV Rusanov update -- TEST INFRASTRUCTURE ONLY.

    Q_c <- Q_c - (dt/h) sum_d (F*_{c+1/2,d} - F*_{c-1/2,d}),
    F*_{c+1/2,d} = 1/2 (f_d(Q_c) + f_d(Q_n)) - 1/2 max(l_d(Q_c), l_d(Q_n)) (Q_n - Q_c)

for the n_real evolved variables of every interior volume; halo layers and auxiliary variables are returned untouched.  Written from the
formula in vectorised numpy (np.longdouble: 64-bit mantissa on x86), not from oracle/exa_oracle.c.  Term sets: Euler (rho, m0, m1, m2, E;
2-D and 3-D) and the built-in advection (velocity 1, 1/2, -3/4 for every variable).

Beside the new state, update() returns two arrays over the evolved variables of the interior volumes:

  M  the MAGNITUDE of the output: the same expression with every product and sum over absolute values,
         |Q_c| + |dt/h| sum_faces (1/2 (|F|_c + |F|_n) + 1/2 s (|Q_n| + |Q_c|)),
     |F| built from |u_n| |q| and |p| <= (gamma - 1)(|E| + ke), s the face's eigenvalue.
  E  the ROUNDING BOUND of an fp64 evaluation in units of 2^-53: the operation count of the formula applied term by term (a running first-order
     error bound).  Every fp64 operation of the straightforward evaluation -- the order of orc_fv_rusanov / `flux_rt` / `maxeig`:
         irho = 1 / rho;  p = (g-1) (E - 1/2 irho (m0^2 + m1^2 + m2^2));  coeff = irho m_n;  F_v = coeff q_v (+ p);  F_E = coeff E + coeff p;
         c = sqrt(g |p| irho);  l = max(|m_n irho - c|, |m_n irho + c|);
         acc += 1/2 (F_c + F_n) - 1/2 s (Q_n - Q_c)  (2 dim faces);  Q_c - (dt/h) acc
     adds |result| (one rounding, 2^-53 relative) to the bound carried by its operands: a + b: e_a + e_b + |a + b|;  a b: |a| e_b + |b| e_a + |a b|;
     1 / x: e_x / x^2 + R_rcp / |x|;  sqrt(x): e_x / (2 sqrt x) + R_sqrt sqrt(x);  max: the larger bound;  abs, a factor 1/2, a sign: none.
     Products with the fp64 constants (g - 1 = fl(1.4) - 1, g = fl(1.4), the advection velocities) use the same constants here, so they cost the
     one rounding of the product.
     The flat form, per evolved Euler variable in 3-D, in units of 2^-53 of the term's magnitude (the largest case, the energy):
       pressure p            7 on its kinetic part (3 squares and 2 sums count 3 along the longest path, irho 1, the product 1, the subtraction 1,
                             times g - 1: 1), 2 on E (subtraction, product);  relative to |p| itself: 7 k, with
                             k = (|E| + ke) / |E - ke| the cancellation in the pressure (1 at rest, 6.8 in the supersonic family)
       flux F_E              coeff = irho m_n: 2;  coeff E: 3;  coeff p: 2 + 7 + 1 = 10;  their sum: + 1  ->  11
       sound speed c         radicand g |p| irho: 7 k + 1 (irho) + 2 (products);  the square root halves it and adds 1  ->  (7 k + 3) / 2 + 1
       eigenvalue l          u_n = m_n irho: 2;  |u_n -+ c|: + 1  ->  at most (7 k + 3) / 2 + 2, i.e. 31.5 at k = 8
       face term             Q_n - Q_c: 1;  times l: + 1;  1/2 (F_c + F_n) minus it: + 1  ->  l's count + 3 = 34.5 (it exceeds the flux part's 11 + 2)
       accumulation          2 dim sums: 6
       Q_c - (dt/h) acc      the quotient dt / h, the product, the sum: 3
     together 43.5: a flat constant C with E <= C M is 44 at k <= 8 (C_ieee).  The bound the tests use is E itself, which is never larger
     (tests/test_fv_reference.py asserts E <= 44 M) and follows k volume by volume instead of assuming its largest value everywhere.
     The primitives' accuracies are parameters: IEEE (correctly rounded division and square root: R_rcp = R_sqrt = 1) gives E_ieee; DEVICE
     (`fast_rcp` <= 11 ulp = 22 units of 2^-53, `fast_sqrt` <= 1 ulp = 2 units: exa_pde.hpp, measured by scripts/rcp_accuracy.hip) pushed through
     the same count gives E_dev (flat: irho 22 in place of 1, so p's kinetic part 28 -> 28 k, radicand 28 k + 22 + 2, c (28 k + 24) / 2 + 2 = 126 at
     k = 8, eigenvalue 127, face term 130, in all C_dev = 139 at k <= 8).  Contraction into fma, a flux kept as q_n instead of (q_n / rho) rho, and |u_n| + c
     for the maximum remove roundings and add none, so the forms the kernels use stay inside the same count.
     A result is accepted when |got - new| <= 2^-53 E (the reference's own error, ~2^-64 M, is 2^-11 of that unit).

grid_update() is the global-array form of a grid step: halo-less patches [g.., P.., V] are assembled into one periodic or Dirichlet array,
updated as one array and cut back into patches.  max_eigenvalue() is the eigenvalue in long double (optionally with its rounding bound).

MUTANTS: each changes a single thing of the formula (tests/test_fv_reference.py: every one leaves the device bound 100-fold).
"""
import collections

import numpy as np

LD = np.longdouble
U53 = LD(2) ** -53
PDE_EULER, PDE_ADVECTION = 1, 2
GAMMA = LD(np.float64(1.4))
GM1 = LD(np.float64(1.4) - np.float64(1.0))              # what `GAMMA - 1` is in fp64
ADV_A = (LD(1.0), LD(0.5), LD(-0.75))
IEEE = {"rcp": 1.0, "sqrt": 1.0}                         # half an ulp
DEVICE = {"rcp": 22.0, "sqrt": 2.0}                      # fast_rcp <= 11 ulp, fast_sqrt <= 1 ulp (exa_pde.hpp)
MUTANTS = ("spacing",             # dt/h along the last axis with the spacing patch length / (P + 2): the extent with the stencil's halo layers
           "no_max",              # dissipation with lambda_c alone
           "quarter",             # dissipation coefficient 1/2 -> 1/4
           "wrong_axis",          # 3-D: the neighbours of axis 1 taken across axis 2
           "plus_for_minus",      # axis 0: the plus-side state in place of the minus side
           "no_pressure_energy",  # Euler: the energy flux without the pressure
           "rcp_2m40",            # Euler: 1 / rho with a relative error of 2^-40 (a reciprocal one Newton step short)
           "halo_next_patch")     # the face-halo layers of patch k read from patch k + 1
Result = collections.namedtuple("Result", "new M E")


def mutant_exemption(mutant, dim, n_patches, pde):
    """None when the mutant applies to such a row, else the reason it cannot."""
    if mutant == "wrong_axis" and dim == 2:
        return "a 2-D row has no third axis"
    if mutant == "halo_next_patch" and n_patches == 1:
        return "there is no next patch"
    if mutant in ("no_pressure_energy", "rcp_2m40") and pde == PDE_ADVECTION:
        return "the advection has neither a pressure nor a reciprocal"
    if mutant == "no_max" and pde == PDE_ADVECTION:
        return "the advection's eigenvalue is the same constant in every volume: the maximum of two equal values"
    return None


class _V:
    """value (long double array) and its rounding bound in units of 2^-53 (None: not tracked)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v, self.e = v, e


def _in(v, track):
    return _V(v, np.zeros_like(v) if track else None)


def _add(a, b, sign=1):
    v = a.v + b.v if sign > 0 else a.v - b.v
    return _V(v, None if a.e is None else a.e + b.e + np.abs(v))


def _mul(a, b):
    v = a.v * b.v
    return _V(v, None if a.e is None else np.abs(a.v) * b.e + np.abs(b.v) * a.e + np.abs(v))


def _exact(a, c):
    """times a power of two or a sign"""
    return _V(a.v * c, None if a.e is None else a.e * abs(c))


def _const(a, c):
    """times an fp64 constant: the product's rounding"""
    v = a.v * c
    return _V(v, None if a.e is None else a.e * abs(c) + np.abs(v))


def _rcp(a, R):
    v = 1 / a.v
    return _V(v, None if a.e is None else a.e * v * v + R * np.abs(v))


def _sqrt(a, R):
    v = np.sqrt(a.v)
    if a.e is None:
        return _V(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(v > 0, a.e / (2 * v), 0) + R * v
    return _V(v, e)


def _abs(a):
    return _V(np.abs(a.v), a.e)


def _max(a, b):
    return _V(np.maximum(a.v, b.v), None if a.e is None else np.maximum(a.e, b.e))


def _terms(q, dim, pde, prim, mutant):
    """q: the m evolved variables (_V, any shape) -> F[d][v], lam[d] (_V) and |F|[d][v] (plain arrays)"""
    m = len(q)
    if pde == PDE_ADVECTION:
        F = [[_const(q[v], ADV_A[d]) for v in range(m)] for d in range(dim)]
        lam = [_V(np.full_like(q[0].v, abs(ADV_A[d])), None if q[0].e is None else np.zeros_like(q[0].v)) for d in range(dim)]
        Fabs = [[abs(ADV_A[d]) * np.abs(q[v].v) for v in range(m)] for d in range(dim)]
        return F, lam, Fabs
    assert pde == PDE_EULER and m >= 5
    rho, mom, en = q[0], q[1:4], q[4]
    wrong = (1 + LD(2) ** -40) if mutant == "rcp_2m40" else None
    irho = _rcp(rho, prim["rcp"])
    if wrong is not None:
        irho = _V(irho.v * wrong, irho.e)
    sq = _add(_add(_mul(mom[0], mom[0]), _mul(mom[1], mom[1])), _mul(mom[2], mom[2]))
    p = _const(_add(en, _exact(_mul(irho, sq), 0.5), -1), GM1)
    pb = GM1 * (np.abs(en.v) + 0.5 * np.abs(irho.v) * sq.v)                       # |p| <= (g - 1)(|E| + ke)
    # eigenvalue: 1 / |rho| is a reciprocal of its own in the straightforward form
    irho_a = _rcp(_abs(rho), prim["rcp"])
    if wrong is not None:
        irho_a = _V(irho_a.v * wrong, irho_a.e)
    p_a = _const(_add(en, _exact(_mul(irho_a, sq), 0.5), -1), GM1)
    c = _sqrt(_mul(_const(_abs(p_a), GAMMA), irho_a), prim["sqrt"])
    F, lam, Fabs = [], [], []
    for d in range(dim):
        coeff = _mul(irho, mom[d])
        f = [_mul(coeff, q[v]) for v in range(4)]
        f.append(_mul(coeff, en) if mutant == "no_pressure_energy" else _add(_mul(coeff, en), _mul(coeff, p)))
        f[d + 1] = _add(f[d + 1], p)
        f += [_V(np.zeros_like(rho.v), None if rho.e is None else np.zeros_like(rho.v)) for _ in range(m - 5)]
        un = _mul(mom[d], irho_a)
        F.append(f)
        lam.append(_max(_abs(_add(un, c, -1)), _abs(_add(un, c))))
        ua = np.abs(irho.v * mom[d].v)
        fa = [ua * np.abs(q[v].v) for v in range(4)] + [ua * (np.abs(en.v) + pb)] + [np.zeros_like(rho.v)] * (m - 5)
        fa[d + 1] = fa[d + 1] + pb
        Fabs.append(fa)
    return F, lam, Fabs


def _update_block(A, dt, h, dim, m, pde, prim, mutant, track):
    """A [..., n0 + 2, .., n_{dim-1} + 2, V] (long double): the update of every volume that has both neighbours along every axis ->
    (new [..., n0, .., m], M, E)."""
    nd = A.ndim
    ax0 = nd - 1 - dim

    def cut(x, axis=None, shift=0):
        idx = [slice(None)] * x.ndim
        for a in range(dim):
            n = x.shape[ax0 + a]
            s = shift if a == axis else 0
            idx[ax0 + a] = slice(1 + s, n - 1 + s)
        return x[tuple(idx)]

    def cutv(x, axis=None, shift=0):
        return _V(cut(x.v, axis, shift), None if x.e is None else cut(x.e, axis, shift))

    q = [_in(np.ascontiguousarray(A[..., v]), track) for v in range(m)]
    F, lam, Fabs = _terms(q, dim, pde, prim, mutant)
    doh_v = LD(dt) / LD(h)
    half_d = 0.25 if mutant == "quarter" else 0.5
    new, M, E = [], [], []
    for v in range(m):
        qc = cutv(q[v])
        acc, mag = None, 0
        for d in range(dim):
            na = 2 if (mutant == "wrong_axis" and d == 1 and dim == 3) else d
            lc, Fc = cutv(lam[d]), cutv(F[d][v])
            sides = {}
            for sgn in (1, -1):
                s_eff = 1 if (mutant == "plus_for_minus" and d == 0) else sgn
                sides[sgn] = (cutv(q[v], na, s_eff), cutv(F[d][v], na, s_eff), cutv(lam[d], na, s_eff),
                              np.abs(cut(q[v].v, na, s_eff)), cut(Fabs[d][v], na, s_eff))
            n_d = A.shape[ax0 + d] - 2
            fac = LD(n_d) / LD(n_d + 2) if (mutant == "spacing" and d == dim - 1) else LD(1)      # h -> h (n + 2) / n along the last axis
            for sgn in (1, -1):
                qn, Fn, ln, qna, Fna = sides[sgn]
                s = lc if mutant == "no_max" else _max(lc, ln)
                if sgn > 0:
                    term = _add(_exact(_add(Fc, Fn), 0.5), _mul(_exact(s, half_d), _add(qn, qc, -1)), -1)
                else:
                    term = _add(_exact(_add(Fn, Fc), 0.5), _mul(_exact(s, half_d), _add(qc, qn, -1)), -1)
                if fac != 1:
                    term = _V(term.v * fac, term.e)
                acc = (term if sgn > 0 else _exact(term, -1)) if acc is None else _add(acc, term, sgn)
                mag = mag + 0.5 * (cut(Fabs[d][v]) + Fna) + 0.5 * s.v * (qna + np.abs(qc.v))
        doh = _V(np.full_like(qc.v, doh_v), None if not track else np.full_like(qc.v, abs(doh_v)))
        out = _add(qc, _mul(doh, acc), -1)
        new.append(out.v)
        M.append(np.abs(qc.v) + abs(doh_v) * mag)
        E.append(out.e if track else np.zeros_like(out.v))
    return np.stack(new, -1), np.stack(M, -1), np.stack(E, -1)


def interior(dim, P, H):
    """index of the interior volumes of a patch array [n, S.., V]"""
    return (slice(None),) + (slice(H, H + P),) * dim


def halo_from_next_patch(Q, dim, P, H):
    """the mutant's input: every patch's halo layers are those of the next patch (cyclically)"""
    out = np.array(Q, copy=True)
    nxt = np.roll(Q, -1, axis=0)
    S = P + 2 * H
    co = np.indices((S,) * dim)
    halo = np.zeros((S,) * dim, dtype=bool)
    for a in range(dim):
        halo |= (co[a] < H) | (co[a] >= H + P)
    out[:, halo] = nxt[:, halo]
    return out


def update(Q, dt, h, dim, P, H, n_real, n_aux=0, pde=PDE_EULER, prim=IEEE, mutant=None, track=True):
    """Q [n_patches, S.., n_real + n_aux] (S = P + 2 H, any H >= 1) -> Result(new [as Q, long double], M, E [n_patches, P.., n_real])."""
    Q = np.asarray(Q)
    S = P + 2 * H
    assert H >= 1 and Q.shape[1:] == (S,) * dim + (n_real + n_aux,), Q.shape
    assert mutant is None or mutant in MUTANTS
    src = halo_from_next_patch(Q, dim, P, H) if mutant == "halo_next_patch" else Q
    A = src[(slice(None),) + (slice(H - 1, H + P + 1),) * dim].astype(LD)
    new_i, M, E = _update_block(A, dt, h, dim, n_real, pde, prim, mutant, track)
    new = Q.astype(LD)
    new[interior(dim, P, H) + (slice(0, n_real),)] = new_i
    return Result(new, M, E)


def assemble(U, dim):
    """[g.., P.., V] -> the global array [g0 P, g1 P, (g2 P,) V]"""
    g, P = U.shape[:dim], U.shape[dim]
    perm = [x for a in range(dim) for x in (a, dim + a)] + [2 * dim]
    return np.transpose(U, perm).reshape(tuple(ga * P for ga in g) + (U.shape[-1],))


def cut_patches(G, dim, grid, P):
    """the inverse of assemble()"""
    shp = [x for a in range(dim) for x in (grid[a], P)] + [G.shape[-1]]
    perm = [2 * a for a in range(dim)] + [2 * a + 1 for a in range(dim)] + [2 * dim]
    return np.transpose(G.reshape(shp), perm)


def grid_update(U, dt, h, dim, n_real, pde=PDE_EULER, boundary=None, prim=IEEE, track=True):
    """One step of a Cartesian grid of halo-less patches U [g.., P.., V] as ONE array: periodic (boundary None) or with the prescribed states
    boundary[(axis, side)] beyond the domain faces.  -> Result(new [as U, long double], M, E [g.., P.., n_real])."""
    U = np.asarray(U)
    grid, P = U.shape[:dim], U.shape[dim]
    G = assemble(U, dim).astype(LD)
    pad = [(1, 1)] * dim + [(0, 0)]
    A = np.pad(G, pad, mode="wrap")
    if boundary is not None:
        for a in range(dim):
            for side in range(2):
                idx = [slice(None)] * (dim + 1)
                idx[a] = 0 if side == 0 else A.shape[a] - 1
                A[tuple(idx)] = np.asarray(boundary[(a, side)] if isinstance(boundary, dict) else boundary, dtype=np.float64).astype(LD)
    new_i, M, E = _update_block(A[None], dt, h, dim, n_real, pde, prim, None, track)
    Gn = G.copy()
    Gn[..., :n_real] = new_i[0]
    return Result(cut_patches(Gn, dim, grid, P), cut_patches(M[0], dim, grid, P), cut_patches(E[0], dim, grid, P))


def max_eigenvalue(q, d, pde=PDE_EULER, prim=None):
    """largest absolute eigenvalue along d of the states q [..., >= n_real] in long double; with `prim`: (value, rounding bound in units of 2^-53)"""
    q = np.asarray(q)
    m = 5 if pde == PDE_EULER else min(q.shape[-1], 8)
    dim = max(d + 1, 2)
    qq = [_in(np.ascontiguousarray(q[..., v]).astype(LD), prim is not None) for v in range(m)]
    lam = _terms(qq, dim, pde, prim or IEEE, None)[1][d]
    return lam.v if prim is None else (lam.v, lam.e)


def ratio(got, res, sel=None):
    """largest |got - new| / (2^-53 E) over the evolved interior values; got, res.new [n, S.., V] (sel: their interior index) or already cut"""
    E = res.E
    new = res.new if sel is None else res.new[sel]
    got = np.asarray(got) if sel is None else np.asarray(got)[sel]
    m = E.shape[-1]
    err = np.abs(got[..., :m].astype(LD) - new[..., :m])
    assert np.all(E > 0)
    return float(np.max(err / (U53 * E)))

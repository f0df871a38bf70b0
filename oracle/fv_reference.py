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

GENERATED TERM SETS (exahype_amd/pde_codegen.py SympyPDE; user_update, user_grid_update, user_max_eigenvalue, USER_MUTANTS).  The side library
instantiates the same kernels for exa::UserPDE, with paths no built-in term set has; the statement the kernel evaluates, and this module too, is

    Q_c <- Q_c - (dt/h) sum_d (F*_{c+1/2,d} - F*_{c-1/2,d} + 1/2 (D_{c,c+1} + D_{c-1,c})) + dt S(Q_c, x_c, t),
    F* as above with f_d(Q, x, t) and l_d(Q, x, t): the volume's terms at x_c, the neighbours' at x_c +- h e_d,
    D = B_d((Q_L + Q_R) / 2, x_c +- (h/2) e_d, t) (Q_R - Q_L)   (the path-conservative jump term at the face's mean state and mid point),
    x_c[a] = centre[patch][a] + (i_a - H + 1/2 - P/2) h,   the CFL scan of a grid step: l_d(Q_new, x_c, t + dt).

  Value.  UserTerms walks the user's own expressions (flux_exprs, eig_exprs, source_exprs, ncp_exprs over q, dq, x, t) node by node on _V: Add, Mul,
     Pow with an integer exponent up to +-4 or +-1/2, Abs, Max, Min and numbers.  A Float is its fp64 value, a Rational p/q is fl(p / q) in fp64 (the C
     printer's `p.0/q.0`); any other node (sin, exp, Piecewise, ..) raises with its name -- no accuracy of the device's libm is recorded.
  Bound.  The rules above with the IEEE primitives (flux_rt / flux_xt, maxeig, source and ncp of a generated term set use IEEE division and square root;
     the FV unit of a side library is compiled without contraction).  Two things follow from the TREE not fixing the order of evaluation -- SymPy keeps a
     sum's terms in its own canonical order, and the generator's common-subexpression pass shares partial sums and products:
       a sum of n terms, in whatever association: every partial sum is at most sum |a_i| and the last one is the result, so it adds
         (n - 2) sum |a_i| + |result|  to the bounds of its terms (n = 2: the rule a + b above);
       a product of n factors: (n - 1) |result| plus the factors' relative bounds, which the rule a b gives in any order;
       a numeric coefficient costs the product's rounding unless it is a sign or a power of two;  x^n: n - 1 products;  x^-n: those and a reciprocal;
       a quotient a / b is counted as a (1 / b): two roundings where the printer's `a/b` has one.
     The coordinates are computed in long double from the fp64 inputs and seeded with the roundings of the kernel's fp64 arithmetic:
       x_c               |k h| + |x_c|  (k = i - H + 1/2 - P/2 is exact; the product with h, the sum with the centre; no centres: the kernel adds 0.0, exact)
       x_c +- h, +- h/2  + |result|     (h and h/2 are exact)
       t + dt            |t + dt|
     and the terms carry them on: a term set whose velocity is 0.3 x turns a coordinate's bound e_x into 0.3 e_x |q| of the flux.
     The count of the new terms, per evolved variable, beyond the count of the term set's own expressions:
       ncp               mean state (Q_c + Q_o) / 2: 1;  jump Q_o - Q_c: 1;  the face's coordinate: 1;  each 1/2 D added to the accumulator: 1 (two per axis)
       source            the product with dt: 1;  the sum: 1
     The magnitude M gains |dt/h| 1/2 (|D|_+ + |D|_-) and |dt| |S|, each the same expression over absolute values.
  Forms.  tests/test_fv_user_reference.py evaluates the statement in fp64 numpy with the terms as written, expanded, after sympy.cse (what the
     generator prints for the FV path) and with the flux in the generator's cached scalars (_aux, _flux_a), on every row of tests/fv_user_cases.py: all of
     them stay inside the bound over the user's tree, so that bound is the one the tests use.  UserTerms(spde, forms=[..]) takes the larger of it and the
     same count over further, algebraically equal expression sets, for a term set whose emitted form the tree's bound does not admit.
  USER_MUTANTS: the new terms' own (no source, the source at the patch centre, terms at t + dt, neighbour terms at x_c, the face mid point at x_c +- h
     or x_c, the ncp at Q_c, not halved, on the plus side only, the next patch's centre, the coordinate without - H) and the six above that do not depend on
     the term set.
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


# ---- term sets generated from SymPy expressions (exahype_amd/pde_codegen.py SympyPDE) -----------------------------------------------------
USER_MUTANTS = ("no_source",             # the update without + dt S
                "source_patch_centre",   # S at the patch centre instead of the volume centre
                "terms_t_plus_dt",       # every term at t + dt
                "nbr_unshifted",         # flux and eigenvalue of the neighbours at the volume's own x_c
                "face_full_h",           # ncp at x_c +- h e_d instead of the face mid point
                "face_at_centre",        # ncp at x_c
                "ncp_at_qc",             # ncp at q_c instead of the face's mean state
                "ncp_not_halved",        # D instead of D / 2
                "ncp_plus_only",         # the jump term of the plus-side face only
                "next_patch_centre",     # centre[patch + 1] in place of centre[patch]
                "no_halo_offset",        # (i + 1/2 - P/2) h with i counted from the array's first (halo) layer: the coordinate without - H
                "spacing", "no_max", "quarter", "wrong_axis", "plus_for_minus", "halo_next_patch")


def _min(a, b):
    return _V(np.minimum(a.v, b.v), None if a.e is None else np.maximum(a.e, b.e))


def _sum_any_order(ts):
    """a_1 + .. + a_n in WHATEVER association: every partial sum is at most sum |a_i| and the last one is the result"""
    v = ts[0].v
    for x in ts[1:]:
        v = v + x.v
    if ts[0].e is None:
        return _V(v)
    return _V(v, sum(x.e for x in ts) + (len(ts) - 2) * sum(np.abs(x.v) for x in ts) + np.abs(v))


class _Walk:
    """One evaluation of expressions over an environment {symbol: (_V, magnitude)}: node by node, shared sub-trees once"""

    def __init__(self, env, prim, like):
        self.env, self.prim, self.like, self.cache = env, prim, like, {}

    def const(self, c):
        v = np.full_like(self.like.v, c)
        return _V(v, None if self.like.e is None else np.zeros_like(v)), np.abs(v)

    @staticmethod
    def number(e):
        """the fp64 constant the C printer's text becomes: a Float is its fp64 value, p/q is fl(p.0 / q.0)"""
        if e.is_Integer:
            return float(int(e))
        if e.is_Rational:
            return float(np.float64(int(e.p)) / np.float64(int(e.q)))
        if e.is_Float:
            return float(e)
        raise NotImplementedError("fv_reference: the number %r is not supported" % (e,))

    def __call__(self, e):
        r = self.cache.get(e)
        if r is None:
            r = self.cache[e] = self._node(e)
        return r

    def _node(self, e):
        if e.is_Symbol:
            return self.env[e]
        if e.is_Number:
            return self.const(self.number(e))
        if e.is_Add:
            ts = [self(a) for a in e.args]
            return _sum_any_order([x[0] for x in ts]), sum(x[1] for x in ts)
        if e.is_Mul:
            c, out = 1.0, None
            for a in e.args:
                if a.is_Number:
                    c *= self.number(a)
                    continue
                x = self(a)
                out = x if out is None else (_mul(out[0], x[0]), out[1] * x[1])
            if out is None:
                return self.const(c)
            if c == 1.0:
                return out
            two = np.frexp(abs(c))[0] == 0.5                                    # a sign or a power of two is exact
            return (_exact(out[0], c) if two else _const(out[0], c)), abs(c) * out[1]
        if e.is_Pow:
            b, ex = self(e.base), e.exp
            if ex.is_Integer and 1 <= abs(int(ex)) <= 4:
                r = b
                for _ in range(abs(int(ex)) - 1):
                    r = (_mul(r[0], b[0]), r[1] * b[1])
                return r if ex > 0 else (_rcp(r[0], self.prim["rcp"]), 1 / np.abs(r[0].v))
            if ex.is_Rational and ex.q == 2 and abs(ex.p) == 1:
                r = _sqrt(b[0], self.prim["sqrt"])
                return (r, np.sqrt(b[1])) if ex > 0 else (_rcp(r, self.prim["rcp"]), 1 / np.abs(r.v))
            raise NotImplementedError("fv_reference: the power %s is not supported (integer exponents up to +-4, +-1/2)" % (ex,))
        name = type(e).__name__
        if name == "Abs":
            x = self(e.args[0])
            return _abs(x[0]), x[1]
        if name in ("Max", "Min"):
            out = self(e.args[0])
            for a in e.args[1:]:
                x = self(a)
                out = ((_max if name == "Max" else _min)(out[0], x[0]), np.maximum(out[1], x[1]))
            return out
        raise NotImplementedError("fv_reference: %s nodes are not supported (+, *, integer and +-1/2 powers, Abs, Max, Min and numbers: the accuracy "
                                  "of the device's libm is not recorded)" % name)


class UserTerms:
    """A SympyPDE as what the update needs: flux / eig / source / ncp over lists of _V (the state, the position x[0..2], the time), each
    returning (_V, magnitude) per expression.  `forms`: further expression sets {"flux": [[..]], "eig": [..], "source": [..], "ncp": [[..]]} that
    are ALGEBRAICALLY the same terms (a form the generator emits): the bound is then the larger of the counts, the value that of the tree."""

    def __init__(self, spde, forms=()):
        self.spde, self.m, self.forms = spde, spde.n_vars, tuple(forms)
        self.has_source, self.has_ncp, self.uses_xt = spde.source_exprs is not None, spde.ncp_exprs is not None, bool(spde.uses_xt)
        xs, t = set(spde.x), spde.t
        every = lambda: [e for f in spde.flux_exprs for e in f] + list(spde.eig_exprs) + list(spde.source_exprs or []) + [e for f in (spde.ncp_exprs or []) for e in f]
        self.uses_x = any(e.free_symbols & xs for e in every())
        self.uses_t = any(t in e.free_symbols for e in every())
        self.source_x = any(e.free_symbols & xs for e in (spde.source_exprs or []))
        self.eig_varies = any(e.free_symbols for e in spde.eig_exprs)

    def shifts_matter(self, dim, what):
        """do the terms along d depend on x[d] (the coordinate that the neighbours / the face mid points shift) for some d < dim"""
        s = self.spde
        per_d = {"nbr": lambda d: list(s.flux_exprs[d]) + [s.eig_exprs[d]], "ncp": lambda d: list(s.ncp_exprs[d]) if s.ncp_exprs else []}[what]
        return any(s.x[d] in e.free_symbols for d in range(dim) for e in per_d(d))

    def ncp_sees_state(self, dim):
        return self.has_ncp and any(e.free_symbols & set(self.spde.q) for d in range(dim) for e in self.spde.ncp_exprs[d])

    def _eval(self, key, pick, q, x, t, prim, dq=None):
        s = self.spde
        env = {sym: (v, np.abs(v.v)) for sym, v in zip(s.q, q)}
        env.update({sym: (v, np.abs(v.v)) for sym, v in zip(s.x, x)})
        env[s.t] = (t, np.abs(t.v))
        if dq is not None:
            env.update({sym: (v, np.abs(v.v)) for sym, v in zip(s.dq, dq)})
        w = _Walk(env, prim, q[0])
        out = [w(e) for e in pick({"flux": s.flux_exprs, "eig": s.eig_exprs, "source": s.source_exprs, "ncp": s.ncp_exprs}[key])]
        for form in self.forms:
            if form.get(key) is None or out[0][0].e is None:
                continue
            w2 = _Walk(dict(env), prim, q[0])
            for k, e in enumerate(pick(form[key])):
                alt = w2(e)[0]
                out[k] = (_V(out[k][0].v, np.maximum(out[k][0].e, alt.e)), out[k][1])
        return out

    def flux(self, q, x, t, d, prim):
        return self._eval("flux", lambda f: f[d], q, x, t, prim)

    def eig(self, q, x, t, d, prim):
        return self._eval("eig", lambda f: [f[d]], q, x, t, prim)[0][0]

    def source(self, q, x, t, prim):
        return self._eval("source", lambda f: f, q, x, t, prim)

    def ncp(self, q, dq, x, t, d, prim):
        return self._eval("ncp", lambda f: f[d], q, x, t, prim, dq)


def user_mutant_exemption(mutant, terms, dim, n_patches, centred):
    """None when the mutant applies to a row of this term set (centred: the row hands patch centres over), else the reason it cannot."""
    if mutant == "wrong_axis" and dim == 2:
        return "a 2-D row has no third axis"
    if mutant == "halo_next_patch" and n_patches == 1:
        return "there is no next patch"
    if mutant == "no_max" and not terms.eig_varies:
        return "the eigenvalue is the same constant in every volume"
    if mutant in ("no_source", "source_patch_centre") and not terms.has_source:
        return "the term set has no source"
    if mutant == "source_patch_centre" and not terms.source_x:
        return "the source does not depend on position"
    if mutant == "terms_t_plus_dt" and not terms.uses_t:
        return "no term depends on time"
    if mutant == "nbr_unshifted" and not terms.shifts_matter(dim, "nbr"):
        return "flux and eigenvalue do not depend on position"
    if mutant.startswith("ncp") and not terms.has_ncp or mutant.startswith("face") and not terms.has_ncp:
        return "the term set has no ncp"
    if mutant.startswith("face") and not terms.shifts_matter(dim, "ncp"):
        return "the ncp does not depend on position"
    if mutant == "ncp_at_qc" and not terms.ncp_sees_state(dim):
        return "the ncp's matrix does not depend on the state"
    if mutant in ("next_patch_centre", "no_halo_offset") and not terms.uses_x:
        return "no term depends on position"
    if mutant == "next_patch_centre" and (not centred or n_patches == 1):
        return "the row has one patch centre (the origin, or a single patch)"
    return None


def _scalar(like, v, e=None):
    x = np.full_like(like.v, v)
    return _V(x, None if like.e is None else (np.zeros_like(x) if e is None else np.full_like(x, e)))


def volume_centres(centres, n, dim, P, h, T=LD, track=True, offset=0):
    """x_c of the interior volumes, three _V [n, P..]: centre[patch][a] + (i - H + 1/2 - P/2) h, i = H .. H + P - 1 (offset: the mutant's + H).
    In T arithmetic from the fp64 inputs; the bound is seeded with the two roundings of the fp64 evaluation: the product with h and the sum
    with the centre (no centres: the kernel adds 0.0, which is exact)."""
    X = []
    for a in range(3):
        shape = (n,) + (P,) * dim
        if a >= dim:
            z = np.zeros(shape, dtype=T)
            X.append(_V(z, z.copy() if track else None))
            continue
        sh = [1] * (1 + dim)
        sh[1 + a] = P
        kh = ((np.arange(P) + 0.5 - 0.5 * P + offset).astype(T) * T(h)).reshape(sh)
        v = np.broadcast_to(kh if centres is None else np.asarray(centres, dtype=np.float64)[:, a].astype(T).reshape((n,) + (1,) * dim) + kh, shape).copy()
        e = np.broadcast_to(np.abs(kh), shape) + (0 if centres is None else np.abs(v))
        X.append(_V(v, np.array(e, dtype=T) if track else None))
    return X


def _update_block_user(A, X, t, dt, h, dim, m, terms, prim, mutant, track, Xs=None):
    """_update_block for a generated term set.  A [n, n0 + 2, .., V] (long double: the reference; fp64 with track=False: an fp64 evaluation of the same
    statement), X: the centres of the volumes that are updated (volume_centres), Xs: the position the mutant hands the source."""
    T = A.dtype.type
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
    qc = [cutv(x) for x in q]
    tt = _scalar(qc[0], T(t) + T(dt), abs(T(t) + T(dt))) if mutant == "terms_t_plus_dt" else _scalar(qc[0], T(t))

    def shifted(d, f):
        """x_c + f h e_d: f h is exact (f = +-1, +-1/2), the sum rounds once"""
        out = list(X)
        out[d] = _add(X[d], _scalar(qc[0], T(f) * T(h)))
        return out
    doh_v = T(dt) / T(h)
    half_d = 0.25 if mutant == "quarter" else 0.5
    acc, mag = [None] * m, [0] * m
    for d in range(dim):
        na = 2 if (mutant == "wrong_axis" and d == 1 and dim == 3) else d
        # terms of the state alone: evaluated once over the whole block and cut, like _update_block (the same values, volume by volume)
        whole = not getattr(terms, "uses_xt", True)
        if whole:
            X0 = [_scalar(q[0], T(0))] * 3
            lw, Fw = terms.eig(q, X0, _scalar(q[0], T(t)), d, prim), terms.flux(q, X0, _scalar(q[0], T(t)), d, prim)
            lc, Fc = cutv(lw), [(cutv(f), None if a is None else cut(a)) for f, a in Fw]
        else:
            lc, Fc = terms.eig(qc, X, tt, d, prim), terms.flux(qc, X, tt, d, prim)
        n_d = A.shape[ax0 + d] - 2
        fac = T(n_d) / T(n_d + 2) if (mutant == "spacing" and d == dim - 1) else T(1)
        nbr = {}
        for sgn in (1, -1):
            s_eff = 1 if (mutant == "plus_for_minus" and d == 0) else sgn
            qn = [cutv(x, na, s_eff) for x in q]
            xn = X if mutant == "nbr_unshifted" else shifted(d, sgn)
            nbr[sgn] = qn
            if whole:
                ln, Fn = cutv(lw, na, s_eff), [(cutv(f, na, s_eff), None if a is None else cut(a, na, s_eff)) for f, a in Fw]
            else:
                ln, Fn = terms.eig(qn, xn, tt, d, prim), terms.flux(qn, xn, tt, d, prim)
            s = lc if mutant == "no_max" else _max(lc, ln)
            for v in range(m):
                if sgn > 0:
                    term = _add(_exact(_add(Fc[v][0], Fn[v][0]), 0.5), _mul(_exact(s, half_d), _add(qn[v], qc[v], -1)), -1)
                else:
                    term = _add(_exact(_add(Fn[v][0], Fc[v][0]), 0.5), _mul(_exact(s, half_d), _add(qc[v], qn[v], -1)), -1)
                if fac != 1:
                    term = _V(term.v * fac, term.e)
                acc[v] = (term if sgn > 0 else _exact(term, -1)) if acc[v] is None else _add(acc[v], term, sgn)
                if track:
                    mag[v] = mag[v] + 0.5 * (Fc[v][1] + Fn[v][1]) + 0.5 * s.v * (np.abs(qn[v].v) + np.abs(qc[v].v))
        if terms.has_ncp:                                  # + 1/2 D_{c,c+1} + 1/2 D_{c-1,c}, D = B_d(mean state, face mid point, t) (q_R - q_L)
            for sgn in ((1,) if mutant == "ncp_plus_only" else (1, -1)):
                qo = nbr[sgn]
                qa = qc if mutant == "ncp_at_qc" else [_exact(_add(qc[v], qo[v]), 0.5) for v in range(m)]
                dq = [_add(qo[v], qc[v], -1) if sgn > 0 else _add(qc[v], qo[v], -1) for v in range(m)]
                xf = X if mutant == "face_at_centre" else shifted(d, sgn * (1.0 if mutant == "face_full_h" else 0.5))
                D = terms.ncp(qa, dq, xf, tt, d, prim)
                for v in range(m):
                    half = _exact(D[v][0], 1.0 if mutant == "ncp_not_halved" else 0.5)
                    if fac != 1:
                        half = _V(half.v * fac, half.e)
                    acc[v] = _add(acc[v], half)
                    if track:
                        mag[v] = mag[v] + 0.5 * D[v][1]
    S = terms.source(qc, Xs if Xs is not None else X, tt, prim) if (terms.has_source and mutant != "no_source") else None
    new, M, E = [], [], []
    for v in range(m):
        doh = _scalar(qc[v], doh_v, abs(doh_v))
        out = _add(qc[v], _mul(doh, acc[v]), -1)
        Mv = (np.abs(qc[v].v) + abs(doh_v) * mag[v]) if track else None
        if S is not None:                                  # + dt S(q_c, x_c, t): the product with dt and the sum
            out = _add(out, _const(S[v][0], T(dt)))
            if track:
                Mv = Mv + abs(T(dt)) * S[v][1]
        new.append(out.v)
        M.append(Mv if track else np.zeros_like(out.v))
        E.append(out.e if track else np.zeros_like(out.v))
    return np.stack(new, -1), np.stack(M, -1), np.stack(E, -1)


def user_update(Q, dt, h, dim, P, H, terms, n_aux=0, centres=None, t=0.0, prim=IEEE, mutant=None, track=True, dtype=LD):
    """update() for a generated term set (UserTerms): centres [n_patches, dim] (fp64; None: the origin) and t as the kernel gets them.
    dtype=np.float64 with track=False evaluates the same statement in fp64 (tests/test_fv_user_reference.py: the bound admits it)."""
    Q = np.asarray(Q)
    S, m, n = P + 2 * H, terms.m, len(Q)
    assert H >= 1 and Q.shape[1:] == (S,) * dim + (m + n_aux,), Q.shape
    assert mutant is None or mutant in USER_MUTANTS, mutant
    src = halo_from_next_patch(Q, dim, P, H) if mutant == "halo_next_patch" else Q
    A = src[(slice(None),) + (slice(H - 1, H + P + 1),) * dim].astype(dtype)
    cen = None if centres is None else np.asarray(centres, dtype=np.float64).reshape(n, dim)
    if mutant == "next_patch_centre":
        cen = np.roll(cen, -1, axis=0)
    X = volume_centres(cen, n, dim, P, h, dtype, track, offset=H if mutant == "no_halo_offset" else 0)
    Xs = None
    if mutant == "source_patch_centre":
        Xs = [_V(np.broadcast_to((np.zeros(n) if (cen is None or a >= dim) else cen[:, a]).astype(dtype).reshape((n,) + (1,) * dim), X[0].v.shape).copy(), None)
              for a in range(3)]
    new_i, M, E = _update_block_user(A, X, t, dt, h, dim, m, terms, prim, mutant, track, Xs)
    new = Q.astype(dtype)
    new[interior(dim, P, H) + (slice(0, m),)] = new_i
    return Result(new, M, E)


def user_grid_update(U, dt, h, dim, terms, centres=None, t=0.0, boundary=None, prim=IEEE, track=True, dtype=LD):
    """grid_update() for a generated term set: the patches' volume centres are assembled into the global array like the states (centres
    [n_patches, dim] in the grid's row-major patch order, as FVPatchGrid.centres)."""
    U = np.asarray(U)
    grid, P, m = U.shape[:dim], U.shape[dim], terms.m
    n = int(np.prod(grid))
    G = assemble(U, dim).astype(dtype)
    A = np.pad(G, [(1, 1)] * dim + [(0, 0)], mode="wrap")
    if boundary is not None:
        for a in range(dim):
            for side in range(2):
                idx = [slice(None)] * (dim + 1)
                idx[a] = 0 if side == 0 else A.shape[a] - 1
                A[tuple(idx)] = np.asarray(boundary[(a, side)] if isinstance(boundary, dict) else boundary, dtype=np.float64).astype(dtype)
    glob = lambda x: assemble(x.reshape(grid + (P,) * dim + (1,)), dim)[None, ..., 0]
    X = [_V(glob(x.v), glob(x.e) if track else None) for x in volume_centres(centres, n, dim, P, h, dtype, track)]
    new_i, M, E = _update_block_user(A[None], X, t, dt, h, dim, m, terms, prim, None, track)
    Gn = G.copy()
    Gn[..., :m] = new_i[0]
    return Result(cut_patches(Gn, dim, grid, P), cut_patches(M[0], dim, grid, P), cut_patches(E[0], dim, grid, P))


def user_max_eigenvalue(terms, q, d, X=None, t=0.0, t_bound=0.0, prim=None):
    """max_eigenvalue() for a generated term set: states q [..., >= n_vars] at the positions X (three _V of q's leading shape; None: the origin)
    and the time t, whose own rounding bound is t_bound (the scan of a grid step evaluates at fl(t + dt): |t + dt|)."""
    q = np.asarray(q)
    track = prim is not None
    qq = [_in(np.ascontiguousarray(q[..., v]).astype(LD), track) for v in range(terms.m)]
    if X is None:
        X = [_scalar(qq[0], LD(0)) for _ in range(3)]
    lam = terms.eig(qq, X, _scalar(qq[0], LD(t), t_bound), d, prim or IEEE)
    return lam.v if not track else (lam.v, lam.e)

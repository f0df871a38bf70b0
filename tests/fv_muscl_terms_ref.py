"""Long-double restatement of the MUSCL-Hancock patch update WITH a source and a non-conservative product (term sets generated with
SympyPDE(muscl_hancock=True, muscl_terms=True); EXA_PDE_FLAG_MUSCL_TERMS) -- TEST INFRASTRUCTURE ONLY.

Written from the five statements of the scheme in vectorised numpy, not from exahype_amd/csrc/exa_fv_muscl.hpp.  On a window Q[n][n_a + 4 ..][V],
evolved variables v < m, r = dt / h, the term set's source S(q) and non-conservative product B_d(q) dq:

  1. slopes       s_e(c) = minmod(Q_c - Q_{c-e}, Q_{c+e} - Q_c) for every axis e (tests/fv_muscl_ref.py: _minmod)
  2. predictor    delta_c = -(r/2) sum_e [f_e(Q_c + s_e/2) - f_e(Q_c - s_e/2) + B_e(Q_c) s_e(c)] + (dt/2) S(Q_c)
  3. face states  w_c^{+-d} = (Q_c +- s_d(c)/2) + delta_c
  4. face flux    F*_{c+1/2,d} = (f_d(w_L) + f_d(w_R))/2 - max(l_d(w_L), l_d(w_R))/2 (w_R - w_L),  w_L = w_c^{+d}, w_R = w_{c+e_d}^{-d}
     face jump    D_{c+1/2,d} = B_d((w_L + w_R)/2) (w_R - w_L)
  5. update       Q_c <- Q_c - r sum_d [(F*_{c+1/2,d} - F*_{c-1/2,d}) + 1/2 (D_{c+1/2,d} + D_{c-1/2,d}) + B_d(Q_c + delta_c) s_d(c)] + dt S(Q_c + delta_c)

With zero slopes and no source this is the first-order Rusanov + ncp update; for a constant B_d = a_d the ncp form and the flux form f_d = a_d q
are the same scheme in exact arithmetic; the source is taken at the half-step state (midpoint rule in time).

update_block() returns (new, M, E) like tests/fv_muscl_ref.py: the new state in long double, the magnitude M and the rounding bound E of an fp64
evaluation in units of 2^-53, by the rules of oracle/fv_reference.py (its _V, _add, _mul, _exact, _const, _max, _sum_any_order and UserTerms are
imported; _minmod and _takev come from tests/fv_muscl_ref.py; all three modules are untouched).  The count of the new operations:

  UserTerms.source / .ncp   carry their own bound over the user's expression tree, as in oracle/fv_reference.py _update_block_user
  mean state                (w_L + w_R)/2: 1 for the sum, the half is free;   w_R - w_L: 1
  Q_c + delta_c             1
  1/2 D                     free
  the added terms           the terms of step 2's bracket over all axes (per axis f(+) - f(-), which costs 1, and B_e s_e) form ONE sum counted
                            with the association-free rule (_sum_any_order), and so do the terms of step 5's bracket (per axis F*_+ - F*_-, which
                            costs 1, 1/2 D_+, 1/2 D_- and B_d s_d): a kernel may add them in any order
  the source                the product with dt (_const) and the sum (_add), as for the Rusanov source; in the predictor dt/2 is as exact as dt
A term set without either term goes through the same lines with empty lists: the values are those of tests/fv_muscl_ref.update_block bit for bit.

MUTANTS, each a single change: no_source (step 5 without + dt S), source_at_old_state (S(Q_c) in step 5), predictor_without_source,
source_times_r (r in place of dt in step 5; seen because h = 0.1), predictor_without_ncp, jump_missing, jump_not_halved, jump_at_left_state
(B at w_L), volume_ncp_missing, volume_ncp_at_old_state (B_d(Q_c) in step 5), volume_ncp_neighbour_slope (the slope of the plus-side neighbour).

fp64_block() is a separately written plain fp64 form of the same statements (the analogue of tests/fv_muscl_ref.fp64_block: rolls over the whole
window, the user's expressions compiled to numpy functions by sympy.lambdify instead of walked), the form the CPU tests hold to the bound;
run_global() is the loop of FVPatchGrid.run on one periodic array; `python -m tests.fv_muscl_terms_ref` writes
tests/golden/fv_muscl_terms_runs.json: the advection-reaction wave q_t + a . grad q = -k q of examples/advection_reaction_fv_second_order.py at 64^2
and 128^2 volumes, in flux form and in ncp form, second order and first order.
"""
import numpy as np

from oracle import fv_reference as R
from oracle.fv_reference import UserTerms, _V, _add, _const, _exact, _max, _mul, _sum_any_order  # noqa: F401
from tests import fv_muscl_ref as M
from tests.fv_muscl_ref import _minmod, _takev

LD = np.longdouble
SOURCE_MUTANTS = ("no_source", "source_at_old_state", "predictor_without_source", "source_times_r")
NCP_MUTANTS = ("predictor_without_ncp", "jump_missing", "jump_not_halved", "jump_at_left_state", "volume_ncp_missing", "volume_ncp_at_old_state",
               "volume_ncp_neighbour_slope")
MUTANTS = SOURCE_MUTANTS + NCP_MUTANTS
Result = M.Result


def mutant_exemption(mutant, terms):
    """None when the mutant applies to a row of this term set, else the reason it cannot."""
    if mutant in SOURCE_MUTANTS and not (terms is not None and terms.has_source):
        return "the term set has no source"
    if mutant in NCP_MUTANTS and not (terms is not None and terms.has_ncp):
        return "the term set has no ncp"
    if mutant in ("jump_at_left_state", "volume_ncp_at_old_state") and not terms.ncp_sees_state(terms.spde.max_dim):
        return "the ncp's matrix does not depend on the state"
    return None


def update_block(A, dt, h, dim, m, pde=R.PDE_EULER, terms=None, prim=R.IEEE, mutant=None, track=True):
    """A [n, n_0 + 4, .., n_{dim-1} + 4, V] (long double: the reference; fp64 with track=False: an fp64 evaluation of the same statements): the
    update of every volume that has two neighbours on either side along every axis -> (new [n, n_0, .., m], M, E)."""
    assert mutant is None or mutant in MUTANTS, mutant
    T = A.dtype.type
    has_src = terms is not None and terms.has_source
    has_ncp = terms is not None and terms.has_ncp
    q = [_V(np.ascontiguousarray(A[..., v]), np.zeros(A.shape[:-1], dtype=A.dtype) if track else None) for v in range(m)]
    one, two = [1] * dim, [2] * dim
    r = T(dt) / T(h)
    rV = lambda like, c: _V(np.full_like(like.v, c * r), None if not track else np.full_like(like.v, abs(c * r)))     # noqa: E731  (c r: r's one rounding)

    def nowhere(like):                                            # x = 0, t = 0: the terms of this mode see the state alone
        z = _V(np.zeros_like(like.v), None if not track else np.zeros_like(like.v))
        return [z, z, z], z

    def ncp(state, dq, d):
        X, t0 = nowhere(state[0])
        return terms.ncp(state, dq, X, t0, d, prim)               # [(value, magnitude)] per variable

    def source(state):
        X, t0 = nowhere(state[0])
        return terms.source(state, X, t0, prim)

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # 1. slopes on the window minus one layer
        q1 = [_takev(x, 0, one, one) for x in q]
        s = []
        for e in range(dim):
            lo, hi = list(one), list(one)
            lo[e], hi[e] = 0, 2
            qm = [_takev(x, 0, lo, hi) for x in q]
            lo[e], hi[e] = 2, 0
            qp = [_takev(x, 0, lo, hi) for x in q]
            s.append([_minmod(_add(q1[v], qm[v], -1), _add(qp[v], q1[v], -1)) for v in range(m)])
        # 2. predictor
        bracket = [[] for _ in range(m)]
        for e in range(dim):
            wp = [_add(q1[v], _exact(s[e][v], 0.5)) for v in range(m)]
            wm = [_add(q1[v], _exact(s[e][v], 0.5), -1) for v in range(m)]
            Fp, Fm = M._eval(wp, dim, pde, terms, prim)[0][e], M._eval(wm, dim, pde, terms, prim)[0][e]
            for v in range(m):
                bracket[v].append(_add(Fp[v], Fm[v], -1))
        if has_ncp and mutant != "predictor_without_ncp":
            for e in range(dim):
                Bs = ncp(q1, s[e], e)
                for v in range(m):
                    bracket[v].append(Bs[v][0])
        dl = [_mul(rV(q1[0], -0.5), bracket[v][0] if len(bracket[v]) == 1 else _sum_any_order(bracket[v])) for v in range(m)]
        if has_src and mutant != "predictor_without_source":
            S1 = source(q1)
            dl = [_add(dl[v], _exact(_const(S1[v][0], T(dt)), 0.5)) for v in range(m)]
        # 3. - 5.
        qc = [_takev(x, 0, two, two) for x in q]
        dc = [_takev(x, 1, two, two) for x in dl]
        qh = [_add(qc[v], dc[v]) for v in range(m)] if (has_src or has_ncp) else None        # the half-step state
        parts, mag = [[] for _ in range(m)], [0] * m
        for d in range(dim):
            lo, hi = list(two), list(two)
            lo[d], hi[d] = 1, 1                                       # the interior and one more volume on either side along d
            qe = [_takev(q1[v], 1, lo, hi) for v in range(m)]
            se = [_takev(s[d][v], 1, lo, hi) for v in range(m)]
            de = [_takev(dl[v], 1, lo, hi) for v in range(m)]
            wplus = [_add(_add(qe[v], _exact(se[v], 0.5)), de[v]) for v in range(m)]
            wminus = [_add(_add(qe[v], _exact(se[v], 0.5), -1), de[v]) for v in range(m)]

            def along(x, a, b, d=d):                                 # volumes a .. n - b of the extended range along d
                idx = [slice(None)] * x.v.ndim
                idx[1 + d] = slice(a, x.v.shape[1 + d] - b)
                return _V(x.v[tuple(idx)], None if x.e is None else x.e[tuple(idx)])

            def along_plain(x, a, b, d=d):
                idx = [slice(None)] * x.ndim
                idx[1 + d] = slice(a, x.shape[1 + d] - b)
                return x[tuple(idx)]
            wL = [along(x, 0, 1) for x in wplus]
            wR = [along(x, 1, 0) for x in wminus]
            FL, lL, FLa = M._eval(wL, dim, pde, terms, prim)
            FR, lR, FRa = M._eval(wR, dim, pde, terms, prim)
            lam = _max(lL[d], lR[d])
            face = [_add(_exact(_add(FL[d][v], FR[d][v]), 0.5), _mul(_exact(lam, 0.5), _add(wR[v], wL[v], -1)), -1) for v in range(m)]
            for v in range(m):
                parts[v].append(_add(along(face[v], 1, 0), along(face[v], 0, 1), -1))
                if track:
                    fm = 0.5 * (FLa[d][v] + FRa[d][v]) + 0.5 * lam.v * (np.abs(wR[v].v) + np.abs(wL[v].v))
                    mag[v] = mag[v] + along_plain(fm, 1, 0) + along_plain(fm, 0, 1)
            if has_ncp and mutant != "jump_missing":              # the jump term of the face, half to either side
                at = wL if mutant == "jump_at_left_state" else [_exact(_add(wL[v], wR[v]), 0.5) for v in range(m)]
                D = ncp(at, [_add(wR[v], wL[v], -1) for v in range(m)], d)
                c = 1.0 if mutant == "jump_not_halved" else 0.5
                for v in range(m):
                    parts[v] += [_exact(along(D[v][0], 1, 0), c), _exact(along(D[v][0], 0, 1), c)]
                    if track:
                        mag[v] = mag[v] + 0.5 * (along_plain(D[v][1], 1, 0) + along_plain(D[v][1], 0, 1))
            if has_ncp and mutant != "volume_ncp_missing":        # B_d at the half-step state times the volume's own slope
                sc = [along(x, 2, 0) if mutant == "volume_ncp_neighbour_slope" else along(x, 1, 1) for x in se]
                Bs = ncp(qc if mutant == "volume_ncp_at_old_state" else qh, sc, d)
                for v in range(m):
                    parts[v].append(Bs[v][0])
                    if track:
                        mag[v] = mag[v] + Bs[v][1]
        S2 = None
        if has_src and mutant != "no_source":
            S2 = source(qc if mutant == "source_at_old_state" else qh)
        new, Mo, E = [], [], []
        for v in range(m):
            out = _add(qc[v], _mul(rV(qc[v], 1.0), _sum_any_order(parts[v])), -1)
            Mv = np.abs(qc[v].v) + abs(r) * mag[v] if track else None
            if S2 is not None:
                k = r if mutant == "source_times_r" else T(dt)
                out = _add(out, _const(S2[v][0], k))
                if track:
                    Mv = Mv + abs(k) * S2[v][1]
            new.append(out.v)
            Mo.append(Mv if track else np.zeros_like(out.v))
            E.append(out.e if track else np.zeros_like(out.v))
    return np.stack(new, -1), np.stack(Mo, -1), np.stack(E, -1)


def interior(dim, P, H):
    return R.interior(dim, P, H)


def update(Q, dt, h, dim, P, H, n_real, n_aux=0, pde=R.PDE_EULER, terms=None, prim=R.IEEE, mutant=None, track=True, dtype=LD):
    """Q [n_patches, S.., n_real + n_aux] (S = P + 2 H, H >= 2) -> Result(new [as Q], M, E [n_patches, P.., n_real]); halo layers and auxiliary
    variables are returned untouched.  dtype=np.float64 with track=False evaluates the same statements in fp64."""
    Q = np.asarray(Q)
    S = P + 2 * H
    assert H >= 2 and Q.shape[1:] == (S,) * dim + (n_real + n_aux,), Q.shape
    A = Q[(slice(None),) + (slice(H - 2, H + P + 2),) * dim].astype(dtype)
    new_i, Mo, E = update_block(A, dt, h, dim, n_real, pde, terms, prim, mutant, track)
    new = Q.astype(dtype)
    new[interior(dim, P, H) + (slice(0, n_real),)] = new_i
    return Result(new, Mo, E)


def grid_update(U, dt, h, dim, n_real, pde=R.PDE_EULER, terms=None, boundary=None, conditions=None, prim=R.IEEE, track=True, dtype=LD):
    """One step of a Cartesian grid of halo-less patches U [g.., P.., V] as ONE array (ghost layers: tests/fv_muscl_ref.global_with_ghosts)
    -> Result(new [as U], M, E [g.., P.., n_real])."""
    U = np.asarray(U)
    grid, P = U.shape[:dim], U.shape[dim]
    G = R.assemble(U, dim)
    A = M.global_with_ghosts(G, dim, boundary, conditions).astype(dtype)
    new_i, Mo, E = update_block(A[None], dt, h, dim, n_real, pde, terms, prim, None, track)
    Gn = G.astype(dtype)
    Gn[..., :n_real] = new_i[0]
    return Result(R.cut_patches(Gn, dim, grid, P), R.cut_patches(Mo[0], dim, grid, P), R.cut_patches(E[0], dim, grid, P))


def ratio(got, res, sel=None):
    return R.ratio(got, res, sel)


# ---- the same statements in fp64, and the runs behind tests/golden/fv_muscl_terms_runs.json --------------------------------------------------
class Terms64:
    """the user's expressions as plain numpy functions of fp64 arrays [..., m] (sympy.lambdify: another order of evaluation than the tree walk of
    UserTerms, the same terms)"""

    def __init__(self, spde):
        import sympy
        q, dq, md = list(spde.q), list(spde.dq), spde.max_dim
        assert not spde.uses_xt
        mk = lambda args, exprs: sympy.lambdify(args, list(exprs), modules="numpy")     # noqa: E731
        self.m = spde.n_vars
        self._flux = [mk(q, spde.flux_exprs[d]) for d in range(md)]
        self._eig = [mk(q, [spde.eig_exprs[d]]) for d in range(md)]
        self._src = mk(q, spde.source_exprs) if spde.source_exprs is not None else None
        self._ncp = [mk(q + dq, spde.ncp_exprs[d]) for d in range(md)] if spde.ncp_exprs is not None else None

    @staticmethod
    def _call(fn, like, *arrays):
        args = [a[..., v] for a in arrays for v in range(a.shape[-1])]
        return np.stack([np.broadcast_to(np.asarray(x, dtype=np.float64), like.shape[:-1]) for x in fn(*args)], -1)

    def flux(self, w, d):
        return self._call(self._flux[d], w, w)

    def eig(self, w, d):
        return self._call(self._eig[d], w, w)[..., 0]

    def source(self, w):
        return self._call(self._src, w, w) if self._src is not None else None

    def ncp(self, w, dw, d):
        return self._call(self._ncp[d], w, w, dw) if self._ncp is not None else None


def fp64_block(A, dt, h, dim, m, terms):
    """the update of update_block() in plain fp64 on the whole window (rolls, as tests/fv_muscl_ref.fp64_block), cut to the volumes it is valid
    for -> new [n, n_0, .., m].  terms: UserTerms (its SympyPDE is compiled to numpy functions) or Terms64."""
    t = terms if isinstance(terms, Terms64) else Terms64(terms.spde)
    q = np.ascontiguousarray(np.asarray(A)[..., :m], dtype=np.float64)
    r = np.float64(dt) / np.float64(h)
    dt = np.float64(dt)
    sh = M._sh
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = []
        for e in range(dim):
            a, b = q - sh(q, e, -1), sh(q, e, 1) - q
            s.append(np.where((a > 0) & (b > 0), np.minimum(a, b), np.where((a < 0) & (b < 0), np.maximum(a, b), 0.0)))
        pred = None
        for e in range(dim):
            dd = t.flux(q + 0.5 * s[e], e) - t.flux(q - 0.5 * s[e], e)
            B = t.ncp(q, s[e], e)
            if B is not None:
                dd = dd + B
            pred = dd if pred is None else pred + dd
        delta = (-0.5 * r) * pred
        S = t.source(q)
        if S is not None:
            delta = delta + (0.5 * dt) * S
        qh = q + delta
        tot = None
        for d in range(dim):
            wL, wR = (q + 0.5 * s[d]) + delta, sh((q - 0.5 * s[d]) + delta, d, 1)
            F = 0.5 * (t.flux(wL, d) + t.flux(wR, d)) - (0.5 * np.maximum(t.eig(wL, d), t.eig(wR, d)))[..., None] * (wR - wL)
            dd = F - sh(F, d, -1)
            D = t.ncp(0.5 * (wL + wR), wR - wL, d)
            if D is not None:
                dd = dd + (0.5 * D + 0.5 * sh(D, d, -1)) + t.ncp(qh, s[d], d)
            tot = dd if tot is None else tot + dd
        new = q - r * tot
        S = t.source(qh)
        if S is not None:
            new = new + dt * S
    return new[(slice(None),) + (slice(2, -2),) * dim]


def fp64_update(Q, dt, h, dim, P, H, n_real, n_aux, terms):
    """update() in plain fp64 -> new [as Q]"""
    Q = np.asarray(Q, dtype=np.float64)
    new = Q.copy()
    new[interior(dim, P, H) + (slice(0, n_real),)] = fp64_block(Q[(slice(None),) + (slice(H - 2, H + P + 2),) * dim], dt, h, dim, n_real, terms)
    return new


def fp64_grid_update(U, dt, h, dim, n_real, terms, conditions=None):
    """grid_update() in plain fp64 -> new [as U]"""
    U = np.asarray(U, dtype=np.float64)
    grid, P = U.shape[:dim], U.shape[dim]
    G = R.assemble(U, dim).copy()
    G[..., :n_real] = fp64_block(M.global_with_ghosts(G, dim, None, conditions)[None], dt, h, dim, n_real, terms)[0]
    return R.cut_patches(G, dim, grid, P)


def rusanov64_block(A1, dt, h, dim, m, terms):
    """the first-order Rusanov + ncp + source update of oracle/fv_reference.py in fp64 on a window with ONE ghost layer -> new [n, n_0, .., m]"""
    A1 = np.ascontiguousarray(A1, dtype=np.float64)
    z = _V(np.zeros(tuple(x - 2 for x in A1.shape[1:1 + dim]), dtype=np.float64)[None], None)
    return R._update_block_user(A1, [z, z, z], 0.0, dt, h, dim, m, terms, R.IEEE, None, False)[0]


def run_global(G, t_end, h, dim, terms, cfl=0.4, scheme="muscl"):
    """Advance the periodic global array G [N.., m] (fp64) to t_end with dt = cfl h / (dim lambda_max) -- the loop of FVPatchGrid.run; -> (G, steps)"""
    G = np.array(G, dtype=np.float64)
    m = terms.m
    t64 = Terms64(terms.spde)
    t, steps = 0.0, 0
    while t < t_end * (1 - 1e-14):
        lam = max(float(np.max(R.user_max_eigenvalue(terms, G, d))) for d in range(dim))
        dt = min(cfl * h / dim / lam, t_end - t)
        A = M.global_with_ghosts(G, dim)[None]
        if scheme == "muscl":
            G[..., :m] = fp64_block(A, dt, h, dim, m, t64)[0]
        else:
            G[..., :m] = rusanov64_block(A[(slice(None),) + (slice(1, -1),) * dim], dt, h, dim, m, terms)[0]
        t += dt
        steps += 1
    return G, steps


def golden_runs():
    """the advection-reaction wave at CFL 0.4, t_end = 0.5: flux form and ncp form, second and first order, 64^2 and 128^2 volumes"""
    from examples import advection_reaction_fv_second_order as X
    out = {"cfl": X.CFL, "t_end": X.T_END, "k": X.K, "velocity": list(X.A)}
    for form in X.FORMS:
        terms = UserTerms(X.term_set(form))
        res = {}
        for N in (64, 128):
            G, exact = X.wave(N)
            for scheme in ("muscl", "rusanov"):
                Gn, steps = run_global(G, X.T_END, 1.0 / N, 2, terms, X.CFL, scheme)
                res["%s_%d" % (scheme, N)] = {"l1": float(np.mean(np.abs(Gn[..., 0] - exact(X.T_END)))), "steps": steps}
        for scheme in ("muscl", "rusanov"):
            res["order_" + scheme] = float(np.log2(res[scheme + "_64"]["l1"] / res[scheme + "_128"]["l1"]))
        out[form] = res
    return out


if __name__ == "__main__":
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fv_muscl_terms_runs.json")
    with open(path, "w") as f:
        json.dump(golden_runs(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(open(path).read())

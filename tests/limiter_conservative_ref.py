"""numpy restatement of the conservative DG / FV interface of the a-posteriori subcell limiter -- SubcellLimiter.step(conservative=True),
step_a_posteriori(conservative=True, rounds=) / run and the two kernels behind them (exa_lim_face_flux, exa_lim_interface_correct) -- for
tests/test_limiter_conservative.py and scripts/make_limiter_conservative_golden.py.  Test infrastructure: built on tests/limiter_mood_ref.py,
the oracle's ADER-DG step with its stages and the oracle's FV patch update, never imported by the product.

The scheme ("correct, re-detect, repeat"), per step: the DG candidate everywhere, then `rounds` times
  1. detect on the current u against the bounds of u^n;  new = detected & ~mask;  mask |= new
  2. the new cells' patches from the projected u^n, with halos
  3. the FV face flux of every face of a new cell between the patch's boundary layer and its halo layer (minus state: lower index),
         g = 1/2 (f_d(Q-) + f_d(Q+)) - 1/2 max(l_d(Q-), l_d(Q+)) (Q+ - Q-),
     brought to the DG face nodes with the limiter's mean-preserving reconstruction: F~ = (R x R) g
  4. FV update and reconstruction of the new cells
  5. every face between a new cell T and a neighbour D outside the cumulative mask: with F* the DG face flux of the step and dF = F~ - F*
         u_D[..i..] -= dt/dx_d phiR_i / w_i dF   (D's upper face),      u_D[..i..] += dt/dx_d phiL_i / w_i dF   (D's lower face)
     -- the corrector's own lift, so D's mean changes by what T's mean changed, with the opposite sign.  A domain face with a boundary
     condition has no neighbour; a face to a cell already in the mask needs nothing (FV on both sides, the same projected states).

bcs: {(axis, side): ("outflow",) | ("wall", sign[V])} as tests/dg_boundary_numpy.py takes them; a face not named is periodic."""
import numpy as np

from oracle import aderdg_numpy as A
from oracle.limiter_numpy import apply_all_axes, build_patch, projection_matrix, reconstruction_matrix
from tests import dg_boundary_numpy as B
from tests import limiter_mood_ref as M
from tests import limiter_ref as L

U53 = 2.0 ** -53


def bound(steps):
    """the conservation bound of a run: 16 roundings of 2^-53 per step in the normalisation of limiter_mood_ref.defects"""
    return 16.0 * steps * U53


def limiter_matrices(ops):
    Ns = 2 * ops["N"] - 1
    P = projection_matrix(ops["xi"], Ns)
    return P, reconstruction_matrix(P, ops["w"])


def dg_step(u, dt, dx, ops, pde, bcs=None):
    """(candidate, Ff): Ff[a][.., f along a, .., face nodes.., var] = the DG face flux F* on the n_a + 1 faces along axis a (face f lies between
    cell f - 1 and cell f; periodic: face 0 and face n_a are the same face)"""
    dim = M._dim(u)
    if bcs:
        st = B.step(u, dt, dx, ops, pde, bcs, stages=True)
        return st["unew"], st["Ffaces"]
    st = A.step(u, dt, dx, ops, pde, stages=True)
    Ff = [np.concatenate([np.take(st["Fstar"][a], [u.shape[a] - 1], axis=a), st["Fstar"][a]], axis=a) for a in range(dim)]
    return st["unew"], Ff


def face_fluxes(patch, pde):
    """g[(a, side)][transverse subcells.., V]: the corrected-mode Rusanov flux between the boundary layer and the halo layer of every face"""
    dim = patch.ndim - 1
    Ns = patch.shape[0] - 2
    out = {}
    for a in range(dim):
        for side in range(2):
            lo = [slice(1, -1)] * dim
            hi = [slice(1, -1)] * dim
            lo[a] = 0 if side == 0 else Ns
            hi[a] = lo[a] + 1
            qm, qp = patch[tuple(lo)], patch[tuple(hi)]
            lam = np.maximum(pde.maxeig(qm, a), pde.maxeig(qp, a))
            out[(a, side)] = 0.5 * (pde.flux(qm, a) + pde.flux(qp, a)) - 0.5 * lam[..., None] * (qp - qm)
    return out


def to_face_nodes(g, R):
    """(R x R) g: [Ns.., V] -> [N.., V]"""
    return apply_all_axes(R, g, g.ndim - 1, 0) if g.ndim > 1 else g


def one_round(u_old, cur, new, cum, Ff, dt, dx, ops, bcs=None, pde=None, fluxes=None):
    """cur with the cells of `new` redone by the FV update of the projected u_old and their neighbours outside `cum` (which includes new)
    corrected.  fluxes (dict, optional): receives F~ per (cell index, axis, side) as [face nodes.., V]."""
    pde = pde or A.Euler()
    bcs = bcs or {}
    dim = M._dim(u_old)
    N = ops["N"]
    w, phiL, phiR = np.asarray(ops["w"]), np.asarray(ops["phiL"]), np.asarray(ops["phiR"])
    P, R = limiter_matrices(ops)
    Ns = 2 * N - 1
    out = cur.copy()
    if not new.any():
        return out
    proj = apply_all_axes(P, u_old, dim, dim)
    fv = M.fv_update(dim, u_old.shape[-1])
    core = (slice(1, -1),) * dim
    Ft = {}
    cells = list(zip(*np.nonzero(new)))
    for idx in cells:
        patch = build_patch(proj, idx, bcs)
        for key, g in face_fluxes(patch, pde).items():
            Ft[(idx,) + key] = to_face_nodes(g, R)
        out[idx] = apply_all_axes(R, fv(patch, dt, dx[0] / Ns)[core], dim, 0)
    if fluxes is not None:
        fluxes.update(Ft)
    for idx in cells:
        for a in range(dim):
            for side, off in ((0, -1), (1, +1)):
                if (a, side) in bcs and idx[a] == (0 if side == 0 else u_old.shape[a] - 1):
                    continue                                   # a domain face with a condition: no neighbour
                nb = list(idx)
                nb[a] = (nb[a] + off) % u_old.shape[a]
                nb = tuple(nb)
                if cum[nb]:
                    continue
                f = list(idx)
                f[a] = idx[a] + side
                dF = np.expand_dims(Ft[(idx, a, side)] - Ff[a][tuple(f)], a)
                sh = [1] * (dim + 1)
                sh[a] = N
                if side == 1:                                  # T's upper face is D's lower face
                    out[nb] += dt / dx[a] * (phiL / w).reshape(sh) * dF
                else:
                    out[nb] -= dt / dx[a] * (phiR / w).reshape(sh) * dF
    return out


def step_with_mask(u, mask, dt, dx, ops, bcs=None, pde=None, conservative=True, fluxes=None):
    """SubcellLimiter.step(dt, mask, conservative): one round with the given mask"""
    pde = pde or A.Euler()
    mask = np.asarray(mask, dtype=bool)
    with np.errstate(all="ignore"):
        cand, Ff = dg_step(u, dt, dx, ops, pde, bcs)
        cum = mask if conservative else np.ones_like(mask)     # (no neighbour outside an all-set mask: nothing is corrected)
        return one_round(u, cand, mask, cum, Ff, dt, dx, ops, bcs, pde, fluxes)


def step(u, dt, dx, ops, rounds=3, bcs=None, pde=None, d0=M.D0, eps=M.EPS, floor=M.FLOOR, info=None):
    """One conservative a-posteriori step: (u_new, cumulative mask, unresolved) -- unresolved: the cells one more detection would still mark.
    info (dict, optional): receives "new" (cells added per round) and "margin" (the smallest decision margin of every round's detection)."""
    pde = pde or A.Euler()
    no_nb = tuple(bcs) if bcs else ()
    with np.errstate(all="ignore"):
        bounds = M.cell_bounds(u)
        cur, Ff = dg_step(u, dt, dx, ops, pde, bcs)
        cum = np.zeros(u.shape[:M._dim(u)], dtype=bool)
        for _ in range(rounds):
            det, margin = M.detect(cur, bounds, d0, eps, floor, no_neighbour=no_nb)
            new = det & ~cum
            cum = cum | new
            if info is not None:
                info.setdefault("new", []).append(int(new.sum()))
                info.setdefault("margin", []).append(float(margin.min()))
            cur = one_round(u, cur, new, cum, Ff, dt, dx, ops, bcs, pde)
        det, _ = M.detect(cur, bounds, d0, eps, floor, no_neighbour=no_nb)
    return cur, cum, int((det & ~cum).sum())


def run_tube(N, nx, dim, rounds=3, t_end=0.1, cfl=0.4, max_steps=100000):
    """limiter_mood_ref.run_tube with the conservative step.  Returns steps, l1, min_rho, min_p (over every step's result), max_troubled
    (cells in one step's cumulative mask), unresolved (summed over the steps), cons (relative defect of every conserved total) -- or, if
    the run leaves the admissible states, what it had until then and "failed"."""
    u0 = M.tube_initial(N, nx, dim)
    pde = A.Euler()
    out = dict(N=N, nx=nx, dim=dim, rounds=rounds, unresolved=0)

    def one(u, dt, dx, ops):
        u, mask, left = step(u, dt, dx, ops, rounds, pde=pde)
        out["unresolved"] += left
        return u, mask
    u, ops = L.run(u0, pde, N, nx, t_end, cfl, max_steps, one, M.track_minima(out), out)
    if "failed" not in out:
        out.update(l1=M.tube_l1(u, ops["xi"], ops["w"], t_end), cons=M.defects(M.totals(u0, ops["w"]), M.totals(u, ops["w"])))
    return out

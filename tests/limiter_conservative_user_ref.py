"""numpy restatement of the conservative DG / FV interface of the a-posteriori subcell limiter for ANY term set with the flux / maxeig
interface of oracle/aderdg_numpy.py (optionally source) -- what a generated term set with SympyPDE(conservative_interface=True) runs on the
device -- for tests/test_limiter_conservative_user.py and scripts/make_limiter_conservative_user_golden.py.  Test infrastructure, never
imported by the product.

A composition: the round is tests/limiter_conservative_ref.one_round (restated here, because that one hard-wires the compiled Euler FV
oracle) with the FV update of tests/limiter_admissible_ref.fv_rusanov (+ dt S for a term set with a source: the statement of
fv_rusanov.hip), the DG step and the face fluxes are limiter_conservative_ref's (the oracle's step carries the source), and detection is
tests/limiter_ref.detect with the term set's admissible / dmp."""
import numpy as np

from oracle.limiter_numpy import apply_all_axes, build_patch
from tests import limiter_admissible_ref as R
from tests import limiter_conservative_ref as K
from tests import limiter_mood_ref as M
from tests import limiter_ref as L

bound = K.bound


def fv_update(pde, dim):
    """fv(patch, dt, h) -> patch: corrected-mode Rusanov update of the interior volumes, + dt S(q) of the volume itself with a source"""
    rusanov = R.fv_rusanov(pde, dim)
    if not hasattr(pde, "source"):
        return rusanov
    core = (slice(1, -1),) * dim

    def fv(patch, dt, h):
        out = rusanov(patch, dt, h)
        out[core] += dt * pde.source(patch[core])
        return out
    return fv


def one_round(u_old, cur, new, cum, Ff, dt, dx, ops, pde, bcs=None, fluxes=None):
    """limiter_conservative_ref.one_round for the term set `pde`: cur with the cells of `new` redone by the FV update of the projected u_old
    and their neighbours outside `cum` (which includes new) corrected.  fluxes (dict, optional): receives F~ per (cell index, axis, side)."""
    bcs = bcs or {}
    dim = L._dim(u_old)
    N = ops["N"]
    w, phiL, phiR = np.asarray(ops["w"]), np.asarray(ops["phiL"]), np.asarray(ops["phiR"])
    P, Rm = K.limiter_matrices(ops)
    Ns = 2 * N - 1
    out = cur.copy()
    if not new.any():
        return out
    proj = apply_all_axes(P, u_old, dim, dim)
    fv = fv_update(pde, dim)
    core = (slice(1, -1),) * dim
    Ft = {}
    cells = list(zip(*np.nonzero(new)))
    for idx in cells:
        patch = build_patch(proj, idx, bcs)
        for key, g in K.face_fluxes(patch, pde).items():
            Ft[(idx,) + key] = K.to_face_nodes(g, Rm)
        out[idx] = apply_all_axes(Rm, fv(patch, dt, dx[0] / Ns)[core], dim, 0)
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


def step_with_mask(u, mask, dt, dx, ops, pde, bcs=None, conservative=True, fluxes=None):
    """SubcellLimiter.step(dt, mask, conservative): one round with the given mask"""
    mask = np.asarray(mask, dtype=bool)
    with np.errstate(all="ignore"):
        cand, Ff = K.dg_step(u, dt, dx, ops, pde, bcs)
        cum = mask if conservative else np.ones_like(mask)     # (no neighbour outside an all-set mask: nothing is corrected)
        return one_round(u, cand, mask, cum, Ff, dt, dx, ops, pde, bcs, fluxes)


def step(u, dt, dx, ops, pde, admissible, dmp, rounds=3, bcs=None, d0=L.D0, eps=L.EPS, floor=L.FLOOR, info=None):
    """One conservative a-posteriori step: (u_new, cumulative mask, unresolved) -- unresolved: the cells one more detection would still mark.
    info (dict, optional): receives "new" (cells added per round) and "margin" (the smallest decision margin of every round's detection)."""
    no_nb = tuple(bcs) if bcs else ()
    dim = L._dim(u)
    with np.errstate(all="ignore"):
        bounds = L.cell_bounds(u, dmp)
        cur, Ff = K.dg_step(u, dt, dx, ops, pde, bcs)
        cum = np.zeros(u.shape[:dim], dtype=bool)
        for _ in range(rounds):
            det, margin = L.detect(cur, bounds, admissible, dmp, d0, eps, floor, no_neighbour=no_nb)
            new = det & ~cum
            cum = cum | new
            if info is not None:
                info.setdefault("new", []).append(int(new.sum()))
                info.setdefault("margin", []).append(float(margin.min()))
            cur = one_round(u, cur, new, cum, Ff, dt, dx, ops, pde, bcs)
        det, _ = L.detect(cur, bounds, admissible, dmp, d0, eps, floor, no_neighbour=no_nb)
    return cur, cum, int((det & ~cum).sum())


def run_dam_break(N, nx, rounds=3, dim=2, t_end=0.05, cfl=0.4, max_steps=100000):
    """limiter_admissible_ref.run_dam_break with the conservative step.  Returns steps, min_h (over every step's result), max_troubled (cells
    in one step's cumulative mask), unresolved (summed over the steps), cons (relative defect of the totals of h, hu, hv) and change =
    depth_change against the initial state -- or, if the run leaves the admissible states, what it had until then and "failed"."""
    u0 = R.dam_initial(N, nx, dim)
    pde = R.ShallowWater()
    out = dict(N=N, nx=nx, dim=dim, rounds=rounds, cfl=cfl, t_end=t_end, min_h=np.inf, unresolved=0)

    def one(u, dt, dx, ops):
        u, mask, left = step(u, dt, dx, ops, pde, R.swe_admissible, (0,), rounds)
        out["unresolved"] += left
        return u, mask

    def track(u):
        out["min_h"] = min(out["min_h"], float(u[..., 0].min()))
    u, ops = L.run(u0.copy(), pde, N, nx, t_end, cfl, max_steps, one, track, out)
    if "failed" not in out:
        w = ops["w"]
        out.update(change=R.depth_change(u, u0, w), cons=M.defects(M.totals(u0, w), M.totals(u, w)))
    return out

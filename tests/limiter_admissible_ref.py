"""numpy restatement of the a-posteriori (MOOD) subcell limiter for a term set that says itself what "admissible" means and which variables
the relaxed discrete maximum principle watches (pde_codegen.SympyPDE(admissible=..., dmp=...); exa_lim_detect.hpp) -- for
tests/test_limiter_admissible.py and scripts/make_limiter_admissible_golden.py.  Test infrastructure, built on tests/limiter_mood_ref.py
(the Euler-layout restatement) and the oracle's ADER-DG step and projection / reconstruction operators; never imported by the product."""
import numpy as np
import sympy

from oracle import aderdg_numpy as A
from oracle.dg_operators import operators
from oracle.limiter_numpy import apply_all_axes, projection_matrix, reconstruction_matrix
from tests import limiter_mood_ref as M

D0, EPS, FLOOR = M.D0, M.EPS, M.FLOOR
G_SWE = 9.81


def criterion(spde):
    """admissible(q) for detect() from a SympyPDE with admissibility expressions: q[..., nv] -> [(g_k, scale_k)], scale_k = the sum of
    the absolute values of g_k's additive terms -- the size rounding errors of two evaluations of g_k are proportional to"""
    fs = []
    for e in spde.adm_exprs:
        terms = sympy.Add.make_args(sympy.expand(e))
        fs.append((sympy.lambdify(spde.q, e, "numpy"), sympy.lambdify(spde.q, sum(sympy.Abs(t) for t in terms), "numpy")))

    def admissible(q):
        cols = [q[..., v] for v in range(q.shape[-1])]
        return [(np.broadcast_to(g(*cols), q.shape[:-1]), np.broadcast_to(sc(*cols), q.shape[:-1])) for g, sc in fs]
    return admissible


def cell_bounds(u, dmp):
    """bounds[grid.., 2 K] = min, max of every watched variable over the nodes of every cell (what exa_lim_snapshot writes)"""
    dim = M._dim(u)
    nodes = tuple(range(dim, 2 * dim))
    cols = []
    for v in dmp:
        cols += [u[..., v].min(nodes), u[..., v].max(nodes)]
    return np.stack(cols, axis=-1) if cols else np.zeros(u.shape[:dim] + (0,))


def neighbourhood(bounds, no_neighbour=(), ghost=None):
    """M.neighbourhood for bounds of any width 2 K: lo[grid.., K], hi[grid.., K]; ghost[(d, side)] = [transverse cells.., 2 K]"""
    if ghost is None:
        return M.neighbourhood(bounds, no_neighbour)
    dim = bounds.ndim - 1
    mins, maxs = bounds[..., 0::2], bounds[..., 1::2]
    lo, hi = mins.copy(), maxs.copy()
    for d in range(dim):
        for side, shift in ((0, 1), (1, -1)):
            nl, nh = np.roll(mins, shift, d), np.roll(maxs, shift, d)
            edge = [slice(None)] * dim
            edge[d] = 0 if side == 0 else -1
            edge = tuple(edge)
            if (d, side) in no_neighbour:
                nl[edge], nh[edge] = mins[edge], maxs[edge]
            elif (d, side) in ghost:
                g = np.asarray(ghost[(d, side)]).reshape(mins[edge].shape[:-1] + (bounds.shape[-1],))
                nl[edge], nh[edge] = g[..., 0::2], g[..., 1::2]
            lo, hi = np.minimum(lo, nl), np.maximum(hi, nh)
    return lo, hi


_smallest = [np.inf]


def reset_margin():
    _smallest[0] = np.inf


def smallest_margin():
    """the smallest relative margin of every comparison detect() made since reset_margin()"""
    return _smallest[0]


def detect(cand, bounds, admissible, dmp, d0=D0, eps=EPS, floor=FLOOR, no_neighbour=(), ghost=None):
    """(mask[grid..], margin[grid..]): troubled if (a) a value is not finite or not g_k > floor at a node for one of admissible(cand)'s
    values, or (b) the nodal range of a watched variable leaves [lo - delta, hi + delta], delta = max(d0, eps (hi - lo)).  admissible:
    q[..., nv] -> list of g_k or of (g_k, scale_k) (see criterion()), or None.  margin: the smallest relative distance of a decision
    quantity of the cell from its threshold (g_k: relative to scale_k; inf for a cell with a non-finite value)."""
    dim = M._dim(cand)
    nodes = tuple(range(dim, 2 * dim))
    grid = cand.shape[:dim]
    with np.errstate(all="ignore"):
        fin = np.isfinite(cand).all(-1).reshape(grid + (-1,)).all(-1)
        bad = ~fin
        margin = np.full(grid, np.inf)
        for item in (admissible(cand) if admissible is not None else []):
            g, scale = item if isinstance(item, tuple) else (item, None)
            bad = bad | ~(g.min(nodes) > floor) | np.isnan(g).reshape(grid + (-1,)).any(-1)
            rel = M._rel(g, floor) if scale is None else np.abs(g - floor) / np.maximum(scale, 1e-300)
            margin = np.minimum(margin, rel.min(nodes))
        if len(dmp):
            lo, hi = neighbourhood(bounds, no_neighbour, ghost)
            for k, v in enumerate(dmp):
                q = cand[..., v]
                l, h = lo[..., k], hi[..., k]
                delta = np.maximum(d0, eps * (h - l))
                qmax, qmin = q.max(nodes), q.min(nodes)
                bad = bad | ~(qmax <= h + delta) | ~(qmin >= l - delta)
                margin = np.minimum(margin, np.minimum(M._rel(qmax, h + delta), M._rel(qmin, l - delta)))
        margin = np.where(fin, margin, np.inf)
    _smallest[0] = min(_smallest[0], float(margin.min()))
    return bad, margin


# ---- the limited step for any term set with the interface of oracle/aderdg_numpy.py (flux, maxeig) ---------------------------------------
def fv_rusanov(pde, dim):
    """corrected-mode Rusanov update of one patch [S.., nv] with one halo layer (interior volumes only), the statement of fv_rusanov.hip"""
    def fv(patch, dt, h):
        core = (slice(1, -1),) * dim
        acc = np.zeros_like(patch[core])

        def shifted(d, s):
            sl = [slice(1, -1)] * dim
            sl[d] = slice(1 + s, patch.shape[d] - 1 + s)
            return patch[tuple(sl)]
        qc = patch[core]
        for d in range(dim):
            qp, qm = shifted(d, 1), shifted(d, -1)
            lc, lp, lm = pde.maxeig(qc, d), pde.maxeig(qp, d), pde.maxeig(qm, d)
            Fc, Fp, Fm = pde.flux(qc, d), pde.flux(qp, d), pde.flux(qm, d)
            acc += 0.5 * (Fc + Fp) - 0.5 * np.maximum(lc, lp)[..., None] * (qp - qc)
            acc -= 0.5 * (Fm + Fc) - 0.5 * np.maximum(lm, lc)[..., None] * (qc - qm)
        out = patch.copy()
        out[core] = qc - dt / h * acc
        return out
    return fv


def replace_troubled(u, cand, mask, dt, dx, ops, fv):
    """M.replace_troubled with the FV update given: cand with the troubled cells replaced by the FV patch update of the projected u"""
    dim = M._dim(u)
    N = ops["N"]
    Ns = 2 * N - 1
    P = projection_matrix(ops["xi"], Ns)
    R = reconstruction_matrix(P, ops["w"])
    out = cand.copy()
    if not mask.any():
        return out
    proj = apply_all_axes(P, u, dim, dim)
    S = Ns + 2
    core = (slice(1, -1),) * dim
    for idx in zip(*np.nonzero(mask)):
        patch = np.pad(proj[idx], [(1, 1)] * dim + [(0, 0)], mode="edge")
        for a in range(dim):
            for side, off in ((0, -1), (1, +1)):
                nb = list(idx)
                nb[a] = (nb[a] + off) % u.shape[a]
                sl = [slice(1, -1)] * dim
                sl[a] = 0 if side == 0 else S - 1
                patch[tuple(sl)] = np.take(proj[tuple(nb)], Ns - 1 if side == 0 else 0, axis=a)
        patch = fv(patch, dt, dx[0] / Ns)
        out[idx] = apply_all_axes(R, patch[core], dim, 0)
    return out


def step(u, dt, dx, ops, pde, admissible, dmp, d0=D0, eps=EPS, floor=FLOOR):
    """One a-posteriori limited step on a periodic grid: (u_new, mask)."""
    with np.errstate(all="ignore"):
        cand = A.step(u, dt, dx, ops, pde)
        mask, _ = detect(cand, cell_bounds(u, dmp), admissible, dmp, d0, eps, floor)
        return replace_troubled(u, cand, mask, dt, dx, ops, fv_rusanov(pde, M._dim(u))), mask


# ---- shallow water (h, hu, hv), the periodic double dam break along x ------------------------------------------------------------------
class ShallowWater:
    """q_t + div F(q) = 0 for q = (h, hu, hv): the expressions of tests/test_user_pde.py swe(), g = 9.81"""
    m = 3

    def flux(self, q, d):
        h = q[..., 0]
        un = q[..., 1 + d] / h
        F = q * un[..., None]
        F[..., 1 + d] += 0.5 * G_SWE * h * h
        return F

    def maxeig(self, q, d):
        h = q[..., 0]
        return np.abs(q[..., 1 + d] / h) + np.sqrt(G_SWE * h)


def swe_admissible(q):
    """the criterion of the shallow-water tests: h > floor"""
    return [q[..., 0]]


def dam_initial(N, nx, dim=2):
    """u[nx, 1, N, N, 3]: h = 1 | 0.1 | 1 (the low level inside (0.25, 0.75)), at rest; the jumps sit on cell faces"""
    nc = (nx,) + (1,) * (dim - 1)
    cx = (np.arange(nx) + 0.5) / nx
    inside = ((cx > 0.25) & (cx < 0.75)).reshape((nx,) + (1,) * (2 * dim - 1))
    u = np.zeros(nc + (N,) * dim + (3,))
    u[..., 0] = np.where(inside, 0.1, 1.0)
    return u


def depth_change(u, u0, w):
    """sum over the grid of the integral of |h - h0| in units of the cell volume"""
    dim = M._dim(u)
    v = np.abs(u[..., 0] - u0[..., 0])
    for _ in range(dim):
        v = np.tensordot(v, w, axes=([dim], [0]))
    return float(v.sum())


def run_dam_break(N, nx, dim=2, t_end=0.05, cfl=0.4, max_steps=100000):
    """The double dam break on nx x 1 cells with the CFL step of SubcellLimiter.run, criterion [h], dmp = (0,).  Returns steps, min_h (over
    every step's result), max_troubled (cells in one step), change = depth_change against the initial state, mass (relative defect of the
    total depth) -- or, if the run leaves the admissible states, what it had until then and "failed"."""
    ops = operators(N)
    w = ops["w"]
    dx = [1.0 / nx] * dim
    u0 = dam_initial(N, nx, dim)
    u = u0.copy()
    pde = ShallowWater()
    t, steps, worst, min_h = 0.0, 0, 0, np.inf
    out = dict(N=N, nx=nx, dim=dim, cfl=cfl, t_end=t_end)
    while t < t_end * (1 - 1e-14) and steps < max_steps:
        with np.errstate(all="ignore"):
            lam = max(np.max(pde.maxeig(u, d)) for d in range(dim))
        if not np.isfinite(lam):
            out["failed"] = "lambda_max = %r at step %d" % (lam, steps)
            break
        dt = min(cfl * dx[0] / ((2 * N - 1) * dim * lam), t_end - t)
        u, mask = step(u, dt, dx, ops, pde, swe_admissible, (0,))
        t += dt
        steps += 1
        worst = max(worst, int(mask.sum()))
        if not np.isfinite(u).all():
            out["failed"] = "non-finite u after step %d" % steps
            break
        min_h = min(min_h, float(u[..., 0].min()))
    out.update(steps=steps, min_h=min_h, max_troubled=worst)
    if "failed" not in out:
        out.update(change=depth_change(u, u0, w), mass=M.defects(M.totals(u0, w)[:1], M.totals(u, w)[:1])[0])
    return out

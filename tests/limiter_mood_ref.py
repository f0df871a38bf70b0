"""numpy restatement of the a-posteriori (MOOD) subcell limiter -- SubcellLimiter.step_a_posteriori / run and the two kernels behind them
(exa_lim_snapshot, exa_lim_detect) -- for tests/test_limiter_a_posteriori.py and scripts/make_limiter_mood_golden.py.  Test
infrastructure: built on the oracle's ADER-DG step, projection / reconstruction operators and FV patch update, never imported by the
product.

Euler layout: density first, energy last, min(3, nv - 2) momenta behind the density, gamma = 1.4."""
import numpy as np

import oracle
from oracle import aderdg_numpy as A
from oracle.dg_operators import operators
from oracle.limiter_numpy import apply_all_axes, projection_matrix, reconstruction_matrix

G = 1.4
D0, EPS, FLOOR = 1e-4, 1e-3, 1e-12


def _dim(u):
    return (u.ndim - 1) // 2


def pressure(u):
    nm = min(3, u.shape[-1] - 2)
    ke = sum(u[..., 1 + a] ** 2 for a in range(nm)) if nm else 0.0
    with np.errstate(all="ignore"):
        return 0.4 * (u[..., -1] - 0.5 * ke / u[..., 0])


def cell_bounds(u):
    """bounds[grid.., 4] = min rho, max rho, min E, max E over the nodes of every cell (what exa_lim_snapshot writes)"""
    dim = _dim(u)
    nodes = tuple(range(dim, 2 * dim))
    return np.stack([u[..., 0].min(nodes), u[..., 0].max(nodes), u[..., -1].min(nodes), u[..., -1].max(nodes)], axis=-1)


def neighbourhood(bounds, no_neighbour=(), ghost=None):
    """lo[grid.., 2], hi[grid.., 2] (rho, E): minimum / maximum of the bounds over the cell and its 2*dim face neighbours.  Periodic wrap;
    (d, side) in no_neighbour: a domain face with a boundary condition, the cell's own bounds; ghost[(d, side)] = [transverse cells.., 4]:
    the neighbour block's bounds across that block face."""
    dim = bounds.ndim - 1
    mins, maxs = bounds[..., 0::2], bounds[..., 1::2]
    lo, hi = mins.copy(), maxs.copy()
    for d in range(dim):
        for side, shift in ((0, 1), (1, -1)):                 # side 0: the neighbour at c_d - 1
            nl, nh = np.roll(mins, shift, d), np.roll(maxs, shift, d)
            edge = [slice(None)] * dim
            edge[d] = 0 if side == 0 else -1
            edge = tuple(edge)
            if (d, side) in no_neighbour:
                nl[edge], nh[edge] = mins[edge], maxs[edge]
            elif ghost is not None and (d, side) in ghost:
                g = np.asarray(ghost[(d, side)]).reshape(mins[edge].shape[:-1] + (4,))
                nl[edge], nh[edge] = g[..., 0::2], g[..., 1::2]
            lo, hi = np.minimum(lo, nl), np.maximum(hi, nh)
    return lo, hi


def _rel(a, b):
    """relative distance of a decision quantity from its threshold"""
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)


def detect(cand, bounds, d0=D0, eps=EPS, floor=FLOOR, no_neighbour=(), ghost=None):
    """(mask[grid..], margin[grid..]) of the candidate against the old state's bounds: troubled if (a) a value is not finite or rho <= floor or
    p <= floor at a node, or (b) the nodal range of rho or E leaves [lo - delta, hi + delta], delta = max(d0, eps (hi - lo)).
    margin: the smallest relative distance of a decision quantity of the cell from its threshold (inf for a cell with a non-finite value:
    finiteness has no threshold).  The pressure's distance is taken relative to the size of its terms, 0.4 (|E| + |m|^2 / (2 |rho|)): it is
    the one quantity whose rounding may differ between two evaluations."""
    dim = _dim(cand)
    nodes = tuple(range(dim, 2 * dim))
    with np.errstate(all="ignore"):
        rho, E, p = cand[..., 0], cand[..., -1], pressure(cand)
        fin = np.isfinite(cand).all(-1).reshape(cand.shape[:dim] + (-1,)).all(-1)
        bad = ~fin | ~(rho.min(nodes) > floor) | ~(p.min(nodes) > floor)
        margin = _rel(rho, floor).min(nodes)
        terms = 0.4 * (np.abs(E) + np.abs(E - p / 0.4))
        margin = np.minimum(margin, (np.abs(p - floor) / np.maximum(terms, 1e-300)).min(nodes))
        lo, hi = neighbourhood(bounds, no_neighbour, ghost)
        for k, q in enumerate((rho, E)):
            l, h = lo[..., k], hi[..., k]
            delta = np.maximum(d0, eps * (h - l))
            qmax, qmin = q.max(nodes), q.min(nodes)
            bad |= ~(qmax <= h + delta) | ~(qmin >= l - delta)
            margin = np.minimum(margin, np.minimum(_rel(qmax, h + delta), _rel(qmin, l - delta)))
        margin = np.where(fin, margin, np.inf)
    return bad, margin


def detect_a_priori(u, w, dmp_tol=0.5, floor=1e-12):
    """SubcellLimiter.detect() restated: the indicator on the state BEFORE the step (cell means of the face neighbourhood, density only)"""
    dim = _dim(u)
    nodes = tuple(range(dim, 2 * dim))
    rho, p = u[..., 0], pressure(u)
    bad = (rho.min(nodes) <= floor) | (p.min(nodes) <= floor) | ~np.isfinite(u).all(-1).reshape(u.shape[:dim] + (-1,)).all(-1)
    mean = rho
    for _ in range(dim):
        mean = np.tensordot(mean, w, axes=([dim], [0]))
    lo, hi = mean.copy(), mean.copy()
    for d in range(dim):
        up, dn = np.roll(mean, -1, d), np.roll(mean, 1, d)
        lo, hi = np.minimum(lo, np.minimum(up, dn)), np.maximum(hi, np.maximum(up, dn))
    span = np.maximum(hi - lo, floor)
    return bad | (rho.max(nodes) > hi + dmp_tol * span) | (rho.min(nodes) < lo - dmp_tol * span)


def fv_update(dim, nv=5):
    def fv(patch, dt, h):
        return oracle.fv_corrected(patch[None], dt, h, dim, patch.shape[0] - 2, 1, nv, 0, 1, oracle.PDE_EULER)[0]
    return fv


def replace_troubled(u, cand, mask, dt, dx, ops):
    """cand with the troubled cells replaced by the FV patch update of the projected u (oracle.limiter_numpy.limited_step with the
    candidate given instead of computed; periodic grid)."""
    dim = _dim(u)
    N = ops["N"]
    Ns = 2 * N - 1
    P = projection_matrix(ops["xi"], Ns)
    R = reconstruction_matrix(P, ops["w"])
    fv = fv_update(dim, u.shape[-1])
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


def step(u, dt, dx, ops, pde=None, d0=D0, eps=EPS, floor=FLOOR):
    """One a-posteriori limited step on a periodic grid: (u_new, mask)."""
    pde = pde or A.Euler()
    with np.errstate(all="ignore"):
        cand = A.step(u, dt, dx, ops, pde)
        mask, _ = detect(cand, cell_bounds(u), d0, eps, floor)
        return replace_troubled(u, cand, mask, dt, dx, ops), mask


# ---- the periodic double Sod tube along x ------------------------------------------------------------------------
def exact_sod(xi):
    """Sod (1, 0, 1 | 0.125, 0, 0.1): density at the similarity coordinate xi = (x - x0) / t"""
    rl, pl, rr, pr = 1.0, 1.0, 0.125, 0.1
    cl, cr = np.sqrt(G * pl / rl), np.sqrt(G * pr / rr)

    def f(p, rk, pk, ck):
        if p > pk:
            a, b = 2 / ((G + 1) * rk), (G - 1) / (G + 1) * pk
            return (p - pk) * np.sqrt(a / (p + b))
        return 2 * ck / (G - 1) * ((p / pk) ** ((G - 1) / (2 * G)) - 1)
    lo, hi = 1e-6, 1.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if f(mid, rl, pl, cl) + f(mid, rr, pr, cr) > 0:
            hi = mid
        else:
            lo = mid
    ps = 0.5 * (lo + hi)
    us = 0.5 * (f(ps, rr, pr, cr) - f(ps, rl, pl, cl))
    rsl = rl * (ps / pl) ** (1 / G)
    csl = cl * (ps / pl) ** ((G - 1) / (2 * G))
    rsr = rr * ((ps / pr + (G - 1) / (G + 1)) / ((G - 1) / (G + 1) * ps / pr + 1))
    S = cr * np.sqrt((G + 1) / (2 * G) * ps / pr + (G - 1) / (2 * G))
    fan = rl * (2 / (G + 1) + (G - 1) / ((G + 1) * cl) * (0 - xi)) ** (2 / (G - 1))
    return np.where(xi < -cl, rl, np.where(xi < us - csl, fan, np.where(xi < us, rsl, np.where(xi < S, rsr, rr))))


def exact_double(x, t):
    """left state inside (0.25, 0.75), right state outside, periodic on [0, 1): valid while the waves of the two jumps have not met"""
    with np.errstate(all="ignore"):
        return np.where(x < 0.5, exact_sod(-(x - 0.25) / t), exact_sod((x - 0.75) / t))


def tube_initial(N, nx, dim):
    """u[nx, 1, (1,) N.., 5]: cell-wise constant data, the jumps sit on cell faces"""
    nc = (nx,) + (1,) * (dim - 1)
    cx = (np.arange(nx) + 0.5) / nx
    inside = ((cx > 0.25) & (cx < 0.75)).reshape((nx,) + (1,) * (2 * dim - 1))
    u = np.zeros(nc + (N,) * dim + (5,))
    u[..., 0] = np.where(inside, 1.0, 0.125)
    u[..., 4] = np.where(inside, 1.0, 0.1) / 0.4
    return u


def totals(u, w):
    """integral of every variable over the grid in units of the cell volume"""
    dim = _dim(u)
    v = u
    for _ in range(dim):
        v = np.tensordot(v, w, axes=([dim], [0]))
    return v.reshape(-1, u.shape[-1]).sum(0)


def tube_l1(u, xi, w, t):
    """L1 error of the density against the exact solution along x (the solution does not depend on the other axes: their first node)"""
    dim = _dim(u)
    nx = u.shape[0]
    line = u[(slice(None),) + (0,) * (dim - 1) + (slice(None),) + (0,) * (dim - 1) + (0,)]
    xn = (np.arange(nx)[:, None] + np.asarray(xi)[None, :]) / nx
    return float((np.abs(line - exact_double(xn, t)) * np.asarray(w)[None, :]).sum() / nx)


def defects(m0, m1):
    return [float(abs(a - b) / max(abs(a), 1.0)) for a, b in zip(m0, m1)]


def run_tube(N, nx, dim, t_end=0.1, cfl=0.4, a_priori=False, max_steps=100000):
    """The double tube on nx x 1 (x 1) cells with the CFL step of SubcellLimiter.run.  Returns steps, l1, min_rho, min_p (over every
    step's result), max_troubled (cells in one step), cons (relative defect of every conserved total) -- or, if the run leaves the
    admissible states, what it had until then and "failed"."""
    ops = operators(N)
    w = ops["w"]
    dx = [1.0 / nx] * dim
    u = tube_initial(N, nx, dim)
    pde = A.Euler()
    m0 = totals(u, w)
    t, steps, worst, min_rho, min_p = 0.0, 0, 0, np.inf, np.inf
    out = dict(N=N, nx=nx, dim=dim)
    while t < t_end * (1 - 1e-14) and steps < max_steps:
        with np.errstate(all="ignore"):
            lam = max(np.max(pde.maxeig(u, d)) for d in range(dim))
        if not np.isfinite(lam):
            out["failed"] = "lambda_max = %r at step %d" % (lam, steps)
            break
        dt = min(cfl * dx[0] / ((2 * N - 1) * dim * lam), t_end - t)
        if a_priori:
            mask = detect_a_priori(u, w)
            with np.errstate(all="ignore"):
                u = replace_troubled(u, A.step(u, dt, dx, ops, pde), mask, dt, dx, ops)
        else:
            u, mask = step(u, dt, dx, ops, pde)
        t += dt
        steps += 1
        worst = max(worst, int(mask.sum()))
        if not np.isfinite(u).all():
            out["failed"] = "non-finite u after step %d" % steps
            break
        min_rho, min_p = min(min_rho, float(u[..., 0].min())), min(min_p, float(pressure(u).min()))
    out.update(steps=steps, min_rho=min_rho, min_p=min_p, max_troubled=worst)
    if "failed" not in out:
        out.update(l1=tube_l1(u, ops["xi"], w, t_end), cons=defects(m0, totals(u, w)))
    return out

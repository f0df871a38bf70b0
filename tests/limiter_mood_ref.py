"""numpy restatement of the a-posteriori (MOOD) subcell limiter -- SubcellLimiter.step_a_posteriori / run and the two kernels behind them
(exa_lim_snapshot, exa_lim_detect) -- for tests/test_limiter_a_posteriori.py and scripts/make_limiter_mood_golden.py: the general limiter of
tests/limiter_ref.py with the Euler criterion and the compiled oracle's FV patch update, and the double Sod tube.  Test infrastructure,
never imported by the product.

Euler layout: density first, energy last, min(3, nv - 2) momenta behind the density, gamma = 1.4."""
import numpy as np

import oracle
from oracle import aderdg_numpy as A
from oracle.dg_operators import operators  # noqa: F401  (the tests take it from here)
from oracle.limiter_numpy import replace_troubled as _replace_troubled
from tests import limiter_ref as L
from tests.limiter_ref import _dim

G = 1.4
D0, EPS, FLOOR = L.D0, L.EPS, L.FLOOR


def pressure(u):
    nm = min(3, u.shape[-1] - 2)
    ke = sum(u[..., 1 + a] ** 2 for a in range(nm)) if nm else 0.0
    with np.errstate(all="ignore"):
        return 0.4 * (u[..., -1] - 0.5 * ke / u[..., 0])


def admissible(u):
    """the Euler criterion for limiter_ref.detect: [rho, (p, size of p's terms)].  The pressure's distance from the floor is taken relative to
    0.4 (|E| + |m|^2 / (2 |rho|)): it is the one quantity whose rounding may differ between two evaluations."""
    E, p = u[..., -1], pressure(u)
    return [u[..., 0], (p, 0.4 * (np.abs(E) + np.abs(E - p / 0.4)))]


def _dmp(u):
    """the watched variables: density and energy"""
    return (0, u.shape[-1] - 1)


def cell_bounds(u):
    """bounds[grid.., 4] = min rho, max rho, min E, max E over the nodes of every cell (what exa_lim_snapshot writes)"""
    return L.cell_bounds(u, _dmp(u))


def detect(cand, bounds, d0=D0, eps=EPS, floor=FLOOR, no_neighbour=(), ghost=None):
    """limiter_ref.detect with the Euler criterion: troubled if a value is not finite, rho <= floor or p <= floor at a node, or the nodal
    range of rho or E leaves the relaxed range of the old state's bounds"""
    return L.detect(cand, bounds, admissible, _dmp(cand), d0, eps, floor, no_neighbour, ghost)


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
    """cand with the troubled cells replaced by the compiled oracle's FV patch update of the projected u (periodic grid)"""
    return _replace_troubled(u, cand, mask, dt, dx, ops, fv_update(_dim(u), u.shape[-1]))


def step(u, dt, dx, ops, pde=None, d0=D0, eps=EPS, floor=FLOOR):
    """One a-posteriori limited step on a periodic grid: (u_new, mask)."""
    return L.step(u, dt, dx, ops, pde or A.Euler(), admissible, _dmp(u), fv_update(_dim(u), u.shape[-1]), d0, eps, floor)


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


def track_minima(out):
    """the callback of limiter_ref.run that keeps min_rho, min_p over every step's result in out"""
    out.update(min_rho=np.inf, min_p=np.inf)

    def track(u):
        out.update(min_rho=min(out["min_rho"], float(u[..., 0].min())), min_p=min(out["min_p"], float(pressure(u).min())))
    return track


def run_tube(N, nx, dim, t_end=0.1, cfl=0.4, a_priori=False, max_steps=100000):
    """The double tube on nx x 1 (x 1) cells with the CFL step of SubcellLimiter.run.  Returns steps, l1, min_rho, min_p (over every
    step's result), max_troubled (cells in one step), cons (relative defect of every conserved total) -- or, if the run leaves the
    admissible states, what it had until then and "failed"."""
    u0 = tube_initial(N, nx, dim)
    pde = A.Euler()

    def one(u, dt, dx, ops):
        if not a_priori:
            return step(u, dt, dx, ops, pde)
        mask = detect_a_priori(u, ops["w"])
        with np.errstate(all="ignore"):
            return replace_troubled(u, A.step(u, dt, dx, ops, pde), mask, dt, dx, ops), mask
    out = dict(N=N, nx=nx, dim=dim)
    u, ops = L.run(u0, pde, N, nx, t_end, cfl, max_steps, one, track_minima(out), out)
    if "failed" not in out:
        out.update(l1=tube_l1(u, ops["xi"], ops["w"], t_end), cons=defects(totals(u0, ops["w"]), totals(u, ops["w"])))
    return out

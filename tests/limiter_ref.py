"""numpy restatement of the a-posteriori (MOOD) subcell limiter, parameterised as the kernel is (exa_lim_detect.hpp): by what "admissible"
means and by the variables the relaxed discrete maximum principle (DMP) watches.  tests/limiter_mood_ref.py (the Euler layout),
tests/limiter_admissible_ref.py (a term set's own criterion) and tests/limiter_conservative_ref.py (the conservative interface) are
instances of it.  Test infrastructure, built on the oracle's ADER-DG step and oracle/limiter_numpy.py; never imported by the product."""
import numpy as np

from oracle import aderdg_numpy as A
from oracle.dg_operators import operators
from oracle.limiter_numpy import replace_troubled

D0, EPS, FLOOR = 1e-4, 1e-3, 1e-12


def _dim(u):
    return (u.ndim - 1) // 2


def cell_bounds(u, dmp):
    """bounds[grid.., 2 K] = min, max of every watched variable over the nodes of every cell (what exa_lim_snapshot writes)"""
    dim = _dim(u)
    nodes = tuple(range(dim, 2 * dim))
    cols = []
    for v in dmp:
        cols += [u[..., v].min(nodes), u[..., v].max(nodes)]
    return np.stack(cols, axis=-1) if cols else np.zeros(u.shape[:dim] + (0,))


def neighbourhood(bounds, no_neighbour=(), ghost=None):
    """lo[grid.., K], hi[grid.., K]: minimum / maximum of the bounds [grid.., 2 K] over the cell and its 2*dim face neighbours.  Periodic wrap;
    (d, side) in no_neighbour: a domain face with a boundary condition, the cell's own bounds; ghost[(d, side)] = [transverse cells.., 2 K]:
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
                g = np.asarray(ghost[(d, side)]).reshape(mins[edge].shape[:-1] + (bounds.shape[-1],))
                nl[edge], nh[edge] = g[..., 0::2], g[..., 1::2]
            lo, hi = np.minimum(lo, nl), np.maximum(hi, nh)
    return lo, hi


def _rel(a, b):
    """relative distance of a decision quantity from its threshold"""
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)


_smallest = [np.inf]


def reset_margin():
    _smallest[0] = np.inf


def smallest_margin():
    """the smallest relative margin of every comparison detect() made since reset_margin()"""
    return _smallest[0]


def detect(cand, bounds, admissible, dmp, d0=D0, eps=EPS, floor=FLOOR, no_neighbour=(), ghost=None):
    """(mask[grid..], margin[grid..]): troubled if (a) a value is not finite or not g_k > floor at a node for one of admissible(cand)'s
    values, or (b) the nodal range of a watched variable leaves [lo - delta, hi + delta], delta = max(d0, eps (hi - lo)).  admissible:
    q[..., nv] -> list of g_k or of (g_k, scale_k), or None; scale_k is the size rounding errors of two evaluations of g_k are proportional
    to.  margin: the smallest relative distance of a decision quantity of the cell from its threshold (g_k: relative to scale_k; inf for a
    cell with a non-finite value: finiteness has no threshold)."""
    dim = _dim(cand)
    nodes = tuple(range(dim, 2 * dim))
    grid = cand.shape[:dim]
    with np.errstate(all="ignore"):
        fin = np.isfinite(cand).all(-1).reshape(grid + (-1,)).all(-1)
        bad = ~fin
        margin = np.full(grid, np.inf)
        for item in (admissible(cand) if admissible is not None else []):
            g, scale = item if isinstance(item, tuple) else (item, None)
            bad = bad | ~(g.min(nodes) > floor) | np.isnan(g).reshape(grid + (-1,)).any(-1)
            rel = _rel(g, floor) if scale is None else np.abs(g - floor) / np.maximum(scale, 1e-300)
            margin = np.minimum(margin, rel.min(nodes))
        if len(dmp):
            lo, hi = neighbourhood(bounds, no_neighbour, ghost)
            for k, v in enumerate(dmp):
                q = cand[..., v]
                l, h = lo[..., k], hi[..., k]
                delta = np.maximum(d0, eps * (h - l))
                qmax, qmin = q.max(nodes), q.min(nodes)
                bad = bad | ~(qmax <= h + delta) | ~(qmin >= l - delta)
                margin = np.minimum(margin, np.minimum(_rel(qmax, h + delta), _rel(qmin, l - delta)))
        margin = np.where(fin, margin, np.inf)
    _smallest[0] = min(_smallest[0], float(margin.min()))
    return bad, margin


def step(u, dt, dx, ops, pde, admissible, dmp, fv, d0=D0, eps=EPS, floor=FLOOR):
    """One a-posteriori limited step on a periodic grid: (u_new, mask).  fv(patch, dt, h) -> patch: the FV update of the troubled cells."""
    with np.errstate(all="ignore"):
        cand = A.step(u, dt, dx, ops, pde)
        mask, _ = detect(cand, cell_bounds(u, dmp), admissible, dmp, d0, eps, floor)
        return replace_troubled(u, cand, mask, dt, dx, ops, fv), mask


def run(u, pde, N, nx, t_end, cfl, max_steps, step, track, out):
    """The CFL loop of SubcellLimiter.run on nx x 1 (x 1) cells of size 1 / nx.  step(u, dt, dx, ops) -> (u_new, mask); track(u) after every
    step whose result is finite: what the problem follows over the steps.  Returns (u, ops); out receives steps and max_troubled (cells in
    one step's mask) -- and, if the run leaves the admissible states, "failed"."""
    dim = _dim(u)
    ops = operators(N)
    dx = [1.0 / nx] * dim
    t, steps, worst = 0.0, 0, 0
    while t < t_end * (1 - 1e-14) and steps < max_steps:
        with np.errstate(all="ignore"):
            lam = max(np.max(pde.maxeig(u, d)) for d in range(dim))
        if not np.isfinite(lam):
            out["failed"] = "lambda_max = %r at step %d" % (lam, steps)
            break
        dt = min(cfl * dx[0] / ((2 * N - 1) * dim * lam), t_end - t)
        u, mask = step(u, dt, dx, ops)
        t += dt
        steps += 1
        worst = max(worst, int(mask.sum()))
        if not np.isfinite(u).all():
            out["failed"] = "non-finite u after step %d" % steps
            break
        track(u)
    out.update(steps=steps, max_troubled=worst)
    return u, ops

"""numpy restatement of the a-posteriori (MOOD) subcell limiter for a term set that says itself what "admissible" means and which variables
the relaxed discrete maximum principle watches (pde_codegen.SympyPDE(admissible=..., dmp=...); exa_lim_detect.hpp) -- for
tests/test_limiter_admissible.py and scripts/make_limiter_admissible_golden.py: the general limiter of tests/limiter_ref.py (cell_bounds,
neighbourhood, detect and its margin bookkeeping are that module's) with a criterion from SymPy expressions, a Rusanov update in numpy, and
the shallow-water dam break.  Test infrastructure; never imported by the product."""
import numpy as np
import sympy

from tests import limiter_mood_ref as M
from tests import limiter_ref as L
from tests.limiter_ref import cell_bounds, detect, neighbourhood, reset_margin, smallest_margin  # noqa: F401  (the general limiter is this module's)

D0, EPS, FLOOR = L.D0, L.EPS, L.FLOOR
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


def step(u, dt, dx, ops, pde, admissible, dmp, d0=D0, eps=EPS, floor=FLOOR):
    """One a-posteriori limited step on a periodic grid: (u_new, mask)."""
    return L.step(u, dt, dx, ops, pde, admissible, dmp, fv_rusanov(pde, L._dim(u)), d0, eps, floor)


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
    dim = L._dim(u)
    v = np.abs(u[..., 0] - u0[..., 0])
    for _ in range(dim):
        v = np.tensordot(v, w, axes=([dim], [0]))
    return float(v.sum())


def run_dam_break(N, nx, dim=2, t_end=0.05, cfl=0.4, max_steps=100000):
    """The double dam break on nx x 1 cells with the CFL step of SubcellLimiter.run, criterion [h], dmp = (0,).  Returns steps, min_h (over
    every step's result), max_troubled (cells in one step), change = depth_change against the initial state, mass (relative defect of the
    total depth) -- or, if the run leaves the admissible states, what it had until then and "failed"."""
    u0 = dam_initial(N, nx, dim)
    pde = ShallowWater()
    out = dict(N=N, nx=nx, dim=dim, cfl=cfl, t_end=t_end, min_h=np.inf)

    def track(u):
        out["min_h"] = min(out["min_h"], float(u[..., 0].min()))
    u, ops = L.run(u0.copy(), pde, N, nx, t_end, cfl, max_steps, lambda u, dt, dx, ops: step(u, dt, dx, ops, pde, swe_admissible, (0,)), track, out)
    if "failed" not in out:
        w = ops["w"]
        out.update(change=depth_change(u, u0, w), mass=M.defects(M.totals(u0, w)[:1], M.totals(u, w)[:1])[0])
    return out

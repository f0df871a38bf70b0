"""The periodic double Sod shock tube of examples/sod_tube_limited.py with both patch updates of the troubled cells: the first-order
Rusanov update (SubcellLimiter's default) and the second-order MUSCL-Hancock update (fv_mode=FV_MUSCL_HANCOCK: patches with halo 2, face
halos two layers deep, edge entries from the diagonal cells).

The limited ADER-DG run is worst wherever the solution is first-order FV -- the few cells at the shocks and contacts -- so the error of
the whole run falls with the order of the update those cells take.  Prints, for either mode, the L1 error of the density against the
exact Riemann solution, the smallest density and pressure over the run and the number of steps.

usage: python examples/sod_tube_limited_second_order.py [cells along x = 32] [order N = 4] [dim = 2] [t_end = 0.1]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

G = 1.4


def exact_sod(xi):
    """Sod (1, 0, 1 | 0.125, 0, 0.1): density at the similarity coordinate xi = (x - x0) / t"""
    rl, pl, rr, pr = 1.0, 1.0, 0.125, 0.1
    cl, cr = np.sqrt(G * pl / rl), np.sqrt(G * pr / rr)

    def f(p, rk, pk, ck):                                      # velocity change across the wave towards side k at star pressure p
        if p > pk:
            a, b = 2 / ((G + 1) * rk), (G - 1) / (G + 1) * pk
            return (p - pk) * np.sqrt(a / (p + b))
        return 2 * ck / (G - 1) * ((p / pk) ** ((G - 1) / (2 * G)) - 1)
    lo, hi = 1e-6, 1.0
    for _ in range(200):                                       # bisection for the star pressure
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


def run(nx, N, dim, t_end, fv_mode, cfl=0.4):
    from exahype_amd import solvers as exa
    nc = (nx,) + (1,) * (dim - 1)
    s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / nx] * dim)
    lim = exa.SubcellLimiter(s, capacity=16, fv_mode=fv_mode)  # a handful of cells are troubled per step; more than 16 would raise
    ops = s.operators()
    inside = ((np.arange(nx) + 0.5) / nx > 0.25) & ((np.arange(nx) + 0.5) / nx < 0.75)
    inside = inside.reshape((nx,) + (1,) * (2 * dim - 1))
    u = np.zeros(nc + (N,) * dim + (5,))
    u[..., 0] = np.where(inside, 1.0, 0.125)
    u[..., 4] = np.where(inside, 1.0, 0.1) / (G - 1)
    s.upload(u)
    steps = lim.run(t_end, cfl=cfl, track=True)
    u = lim.download()
    line = u[(slice(None),) + (0,) * (dim - 1) + (slice(None),) + (0,) * (dim - 1) + (0,)]          # rho along x
    x = (np.arange(nx)[:, None] + ops["xi"][None, :]) / nx
    l1 = float((np.abs(line - exact_double(x, t_end)) * ops["w"][None, :]).sum() / nx)
    st = {k: v.item() for k, v in lim.stats.items()}
    return dict(l1=l1, steps=steps, min_rho=st["min_rho"], min_p=st["min_p"], max_troubled=st["max_troubled"])


def main(nx=32, N=4, dim=2, t_end=0.1):
    from exahype_amd import solvers as exa
    out = {}
    for name, mode in (("rusanov", exa.FV_RUSANOV), ("muscl_hancock", exa.FV_MUSCL_HANCOCK)):
        r = out[name] = run(nx, N, dim, t_end, mode)
        print("%-13s %d steps, at most %d troubled cells in a step, min rho = %.6f, min p = %.6f, L1(rho) = %.8f"
              % (name, r["steps"], r["max_troubled"], r["min_rho"], r["min_p"], r["l1"]))
    print("L1(rho) second order / first order = %.4f" % (out["muscl_hancock"]["l1"] / out["rusanov"]["l1"]))
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 32, int(a[1]) if len(a) > 1 else 4, int(a[2]) if len(a) > 2 else 2, float(a[3]) if len(a) > 3 else 0.1)

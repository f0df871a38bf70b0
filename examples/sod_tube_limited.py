"""A periodic double Sod shock tube through the a-posteriori limited ADER-DG scheme: `SubcellLimiter.run`.

The left state (rho, u, p) = (1, 0, 1) fills x in (0.25, 0.75), the right state (0.125, 0, 0.1) the rest of the periodic unit interval:
two mirrored Sod tubes whose waves have not met at t = 0.1.  Every step the DG candidate is checked on the device against the state it
started from (finite, positive, relaxed discrete maximum principle) and the few cells at the shocks and contacts are redone from that
state with the FV Rusanov patch update on 2p+1 subcells per axis.  Prints the L1 error of the density against the exact Riemann
solution, the smallest density and pressure of the run and the conservation defects.

--conservative makes the DG / FV interface conservative (three rounds of "correct, re-detect, repeat": the untroubled neighbours of the
redone cells trade the DG face flux for the FV one): the defects of mass and energy fall from about 1e-3 to rounding level.

usage: python examples/sod_tube_limited.py [cells along x = 32] [order N = 4] [dim = 2] [t_end = 0.1] [--conservative]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from exahype_amd import solvers as exa

G = 1.4


def sod_density(xi):
    """density of the Sod problem (1, 0, 1 | 0.125, 0, 0.1) at the similarity coordinate xi = (x - x0) / t"""
    rl, pl, rr, pr = 1.0, 1.0, 0.125, 0.1
    cl, cr = np.sqrt(G * pl / rl), np.sqrt(G * pr / rr)

    def f(p, rk, pk, ck):                                      # velocity change across the wave towards side k at star pressure p
        if p > pk:
            return (p - pk) * np.sqrt(2 / ((G + 1) * rk) / (p + (G - 1) / (G + 1) * pk))
        return 2 * ck / (G - 1) * ((p / pk) ** ((G - 1) / (2 * G)) - 1)
    lo, hi = 1e-6, 1.0
    for _ in range(200):                                       # bisection for the star pressure
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if f(mid, rl, pl, cl) + f(mid, rr, pr, cr) > 0 else (mid, hi)
    ps = 0.5 * (lo + hi)
    us = 0.5 * (f(ps, rr, pr, cr) - f(ps, rl, pl, cl))
    rsl = rl * (ps / pl) ** (1 / G)
    csl = cl * (ps / pl) ** ((G - 1) / (2 * G))
    mu = (G - 1) / (G + 1)
    rsr = rr * (ps / pr + mu) / (mu * ps / pr + 1)
    shock = cr * np.sqrt((G + 1) / (2 * G) * ps / pr + (G - 1) / (2 * G))
    with np.errstate(all="ignore"):
        fan = rl * (2 / (G + 1) - mu / cl * xi) ** (2 / (G - 1))
    return np.where(xi < -cl, rl, np.where(xi < us - csl, fan, np.where(xi < us, rsl, np.where(xi < shock, rsr, rr))))


def exact_density(x, t):
    return np.where(x < 0.5, sod_density(-(x - 0.25) / t), sod_density((x - 0.75) / t))


def totals(u, w, dim):
    for _ in range(dim):
        u = np.tensordot(u, w, axes=([dim], [0]))
    return u.reshape(-1, u.shape[-1]).sum(0)


def main(nx=32, N=4, dim=2, t_end=0.1, cfl=0.4, conservative=False):
    nc = (nx,) + (1,) * (dim - 1)
    s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / nx] * dim)
    lim = exa.SubcellLimiter(s, capacity=16)                   # a handful of cells are troubled per step; more than 16 would raise
    ops = s.operators()
    inside = ((np.arange(nx) + 0.5) / nx > 0.25) & ((np.arange(nx) + 0.5) / nx < 0.75)
    inside = inside.reshape((nx,) + (1,) * (2 * dim - 1))
    u = np.zeros(nc + (N,) * dim + (5,))
    u[..., 0] = np.where(inside, 1.0, 0.125)
    u[..., 4] = np.where(inside, 1.0, 0.1) / (G - 1)
    s.upload(u)
    m0 = totals(u, ops["w"], dim)
    steps = lim.run(t_end, cfl=cfl, track=True, conservative=True) if conservative else lim.run(t_end, cfl=cfl, track=True)
    u = lim.download()
    m1 = totals(u, ops["w"], dim)
    line = u[(slice(None),) + (0,) * (dim - 1) + (slice(None),) + (0,) * (dim - 1) + (0,)]          # rho along x
    x = (np.arange(nx)[:, None] + ops["xi"][None, :]) / nx
    l1 = float((np.abs(line - exact_density(x, t_end)) * ops["w"][None, :]).sum() / nx)
    st = {k: v.item() for k, v in lim.stats.items()}
    print("%d steps to t = %.4f on %d cells of order %d (%d-D); at most %d troubled cells in a step" % (steps, s.time, nx, N - 1, dim, st["max_troubled"]))
    print("min rho = %.6f, min p = %.6f over the run; relative defect of (rho, m, E): %s" %
          (st["min_rho"], st["min_p"], " ".join("%.2e" % (abs(a - b) / max(abs(a), 1.0)) for a, b in zip(m0, m1))))
    if conservative:
        print("conservative interface, 3 rounds: %d cells left unresolved over the run" % st["unresolved"])
    print("L1(rho) = %.8f" % l1)
    return l1


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x != "--conservative"]
    main(int(a[0]) if len(a) > 0 else 32, int(a[1]) if len(a) > 1 else 4, int(a[2]) if len(a) > 2 else 2, float(a[3]) if len(a) > 3 else 0.1, conservative="--conservative" in sys.argv[1:])

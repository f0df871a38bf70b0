"""A periodic double dam break for the shallow-water equations through the a-posteriori limited ADER-DG scheme: `SubcellLimiter.run` with
a term set that brings its own admissibility criterion.

The system (h, hu, hv), g = 9.81, is given as SymPy expressions (`SympyPDE`); `admissible=lambda q: [q[0]]` says that a state is admissible
iff the depth is positive and `dmp=(0,)` that the relaxed discrete maximum principle watches the depth.  Without the two keywords the
detector would read the three variables in the Euler layout -- hv as an energy -- and mark every cell with hv < 0.  The depth is 1 outside
and 0.1 inside x in (0.25, 0.75) of the periodic unit interval, at rest: two mirrored dam breaks whose waves have not met at t = 0.05.
Prints the steps, the smallest depth of the run and the largest number of troubled cells in a step.

With a fourth argument `conservative` the term set is generated with `conservative_interface=True` and the run uses the limiter's
conservative DG / FV interface (`run(conservative=True)`, three rounds): the default run loses most of a percent of the water on the faces
between troubled and untroubled cells, this one keeps the totals of h, hu and hv to rounding.  It then also prints the largest relative
defect of the three totals and the number of cells one more detection would still have marked.

usage: python examples/dam_break_limited.py [cells along x = 32] [order N = 4] [t_end = 0.05] [conservative]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import sympy

G = 9.81


def shallow_water(conservative_interface=False):
    from exahype_amd.pde_codegen import SympyPDE

    def flux(q, d):
        h, hu, hv = q
        un = (hu, hv)[d] / h if d < 2 else 0
        p = sympy.Rational(1, 2) * G * h * h
        f = [h * un, hu * un, hv * un]
        if d < 2:
            f[1 + d] = f[1 + d] + p
        return f

    def eig(q, d):
        h, hu, hv = q
        un = (hu, hv)[d] / h if d < 2 else 0
        return sympy.Abs(un) + sympy.sqrt(G * h)
    return SympyPDE(3, flux, eig, max_dim=2, name="shallow_water", admissible=lambda q: [q[0]], dmp=(0,),
                    **({"conservative_interface": True} if conservative_interface else {}))


def main(nx=32, N=4, t_end=0.05, cfl=0.4, conservative=False):
    from exahype_amd import solvers as exa
    pde = shallow_water(conservative_interface=conservative)
    s = exa.AderDgSolver(2, N, (nx, 1), pde=pde.register(), n_vars=3, dx=[1.0 / nx] * 2)
    lim = exa.SubcellLimiter(s, capacity=16)                   # a handful of cells are troubled per step; more than 16 would raise
    cx = (np.arange(nx) + 0.5) / nx
    inside = ((cx > 0.25) & (cx < 0.75)).reshape(nx, 1, 1, 1)
    u = np.zeros((nx, 1, N, N, 3))
    u[..., 0] = np.where(inside, 0.1, 1.0)
    s.upload(u)
    steps = lim.run(t_end, cfl=cfl, track=True, **({"conservative": True, "rounds": 3} if conservative else {}))
    st = lim.stats
    print("%d steps to t = %.4f on %d cells of order %d; the depth stayed above %.6f" % (steps, s.time, nx, N - 1, st["min_admissible"][0].item()))
    last = "steps=%d min_h=%.8f max_troubled=%d" % (steps, st["min_admissible"][0].item(), st["max_troubled"].item())
    if conservative:
        w = np.asarray(s.operators()["w"])
        total = lambda a: np.einsum("xyijv,i,j->v", a, w, w)
        m0, m1 = total(u), total(lim.download())
        last += " mass_defect=%.3e unresolved=%d" % (max(abs(a - b) / max(abs(a), 1.0) for a, b in zip(m0, m1)), st["unresolved"].item())
    print(last)


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 32, int(a[1]) if len(a) > 1 else 4, float(a[2]) if len(a) > 2 else 0.05,
         conservative=len(a) > 3 and a[3] == "conservative")

#!/usr/bin/env python3
"""Times the two kernels of the limiter's conservative DG / FV interface for the built-in Euler set and for the generated Euler set with
SympyPDE(conservative_interface=True), one after the other in one process (HIP events, median after warm-up), one shape per process:

    python scripts/quick_bench_limiter_conservative_user.py N CELLS_PER_AXIS [reps = 5]     (3-D; run each shape under its own `timeout`)

  exa_lim_face_flux           over the capacity-sized slot list, the troubled cells of the first round in it
  exa_lim_interface_correct   six launches
State and mask: those of scripts/quick_bench_limiter_conservative.py (a smooth density wave with node-wise noise in 5 % of the cells; the
first round's detection of the built-in criterion decides the mask for both term sets, so both time the same cells)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sympy
import torch

from exahype_amd import solvers as exa
from exahype_amd.pde_codegen import SympyPDE
from quick_bench_limiter_conservative import timed


def euler_conservative():
    def prim(q):
        irho = 1 / q[0]
        return irho, sympy.Float(0.4) * (q[4] - sympy.Rational(1, 2) * irho * (q[1] ** 2 + q[2] ** 2 + q[3] ** 2))

    def flux(q, d):
        irho, p = prim(q)
        c = irho * q[d + 1]
        f = [c * q[0], c * q[1], c * q[2], c * q[3], c * q[4] + c * p]
        f[d + 1] = f[d + 1] + p
        return f

    def eig(q, d):
        irho, p = prim(q)
        return sympy.Abs(q[d + 1] * irho) + sympy.sqrt(sympy.Float(1.4) * p * irho)
    return SympyPDE(5, flux, eig, max_dim=3, name="euler_from_sympy",
                    admissible=lambda q: [q[0], sympy.Float(0.4) * (q[4] - (q[1] ** 2 + q[2] ** 2 + q[3] ** 2) / (2 * q[0]))], dmp=(0, 4),
                    conservative_interface=True)


def one(label, N, n, reps, mask, **kw):
    """(face flux ms, interface correct ms, the first round's mask) for one term set"""
    dim, nc = 3, (n, n, n)
    s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / n] * dim, **kw)
    lim = exa.SubcellLimiter(s, capacity=int(0.2 * n ** 3))
    g = torch.Generator(device=s.dev).manual_seed(1)
    X = s.node_positions().reshape(s.u.shape[:-1] + (3,))
    rho = 1.0 + 0.2 * torch.sin(2 * torch.pi * X.sum(-1))
    rough = (torch.rand(nc, generator=g, device=s.dev) < 0.05).reshape(nc + (1, 1, 1))
    rho = rho * (1 + 0.3 * rough * (torch.rand(rho.shape, generator=g, device=s.dev) - 0.5))
    u = s.u
    u[..., 0] = rho
    for a in range(3):
        u[..., 1 + a] = 0.1 * (a + 1) * rho
    u[..., 4] = 1.0 / 0.4 + 0.5 * rho * 0.14
    del X, rho
    dt = 0.4 / n / ((2 * N - 1) * dim * float(s.max_eigenvalue()[0]))
    lim._mood_setup()
    lim._conservative_setup("step")
    lim._snapshot(s.u, lim._u_old)
    s.step(dt)
    m = lim._detect(s.u, 1e-4, 1e-3, 1e-12).clone() if mask is None else mask.to(s.dev)
    lim._compact(m.reshape(-1))
    lim._project(m.reshape(-1), lim._u_old, 0.0)
    lim._face_flux()
    lim.check(wait=True)
    t_ff, _ = timed(lim._face_flux, reps)
    lim._interface_correct(m, dt)
    t_ic, _ = timed(lambda: lim._interface_correct(m, dt), reps)
    print("%-34s exa_lim_face_flux %7.3f ms over %d slots (%d troubled)   exa_lim_interface_correct %7.3f ms (six launches)"
          % (label, t_ff, lim.capacity, int(m.sum()), t_ic), flush=True)
    return t_ff, t_ic, m.cpu()


def main(N, n, reps=5):
    print("3-D N = %d, %d^3 cells" % (N, n), flush=True)
    b_ff, b_ic, mask = one("built-in Euler", N, n, reps, None)
    torch.cuda.empty_cache()
    pde = euler_conservative()
    g_ff, g_ic, _ = one("generated Euler (keyword)", N, n, reps, mask, pde=pde.register(), n_vars=5)
    print("generated / built-in: face flux %.3f, interface correct %.3f, both kernels %.3f (margin of a generated set: 1.10)"
          % (g_ff / b_ff, g_ic / b_ic, (g_ff + g_ic) / (b_ff + b_ic)))


if __name__ == "__main__":
    a = sys.argv
    main(int(a[1]), int(a[2]), int(a[3]) if len(a) > 3 else 5)

#!/usr/bin/env python3
"""Times the a-posteriori detector of a GENERATED term set with its own criterion against the built-in one, HIP events after warm-up, on
one shape per process:

    python scripts/quick_bench_limiter_admissible.py N CELLS_PER_AXIS [reps = 5]        (3-D; run each shape under its own `timeout`)

  exa_lim_snapshot, exa_lim_detect   built-in Euler plan, then Euler from SymPy expressions with admissible = [rho, p], dmp = (0, 4):
                                     the same bytes through the same kernel shape (exa_lim_detect.hpp), the criterion folded at compile time
  step_a_posteriori                  default mode, built-in term set (must not move when the detector's code moves)
State: that of scripts/quick_bench_limiter_mood.py -- a smooth density wave with node-wise noise in 5 % of the cells."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sympy
import torch

from exahype_amd import solvers as exa
from exahype_amd.pde_codegen import SympyPDE

COPY_RATE = 6.29e12


def euler_with_criterion():
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
                    admissible=lambda q: [q[0], sympy.Float(0.4) * (q[4] - (q[1] ** 2 + q[2] ** 2 + q[3] ** 2) / (2 * q[0]))], dmp=(0, 4))


def timed(fn, reps, before=None):
    ms = []
    for _ in range(reps):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def fill(s, n):
    g = torch.Generator(device=s.dev).manual_seed(1)
    nc = (n, n, n)
    X = s.node_positions().reshape(s.u.shape[:-1] + (3,))
    rho = 1.0 + 0.2 * torch.sin(2 * torch.pi * X.sum(-1))
    rough = (torch.rand(nc, generator=g, device=s.dev) < 0.05).reshape(nc + (1, 1, 1))
    rho = rho * (1 + 0.3 * rough * (torch.rand(rho.shape, generator=g, device=s.dev) - 0.5))
    u = s.u
    u[..., 0] = rho
    for a in range(3):
        u[..., 1 + a] = 0.1 * (a + 1) * rho
    u[..., 4] = 1.0 / 0.4 + 0.5 * rho * 0.14


def detector_times(s, lim, reps, label):
    ubytes = s.u.numel() * 8
    lim._mood_setup()
    for _ in range(2):
        lim._snapshot(s.u, lim._u_old)
        lim._detect(s.u, 1e-4, 1e-3, 1e-12)
    t_snap, _ = timed(lambda: lim._snapshot(s.u, lim._u_old), reps)
    t_det, _ = timed(lambda: lim._detect(s.u, 1e-4, 1e-3, 1e-12), reps)
    mask = lim._mask.clone()
    for name, t, nbytes in (("exa_lim_snapshot (copy + bounds)", t_snap, 2 * ubytes), ("exa_lim_detect", t_det, ubytes)):
        print("%-10s %-34s %8.3f ms  %6.2f TB/s  %5.1f %% of the copy rate" % (label, name, t, nbytes / t / 1e9, 100 * nbytes / (t * 1e-3) / COPY_RATE))
    return t_snap, t_det, mask, lim._bounds.clone()


def main(N, n, reps=5):
    dim, nc = 3, (n, n, n)
    ncell = n ** 3
    s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / n] * dim)
    lim = exa.SubcellLimiter(s, capacity=int(0.2 * ncell))
    fill(s, n)
    print("3-D N = %d, %d^3 cells, u = %.2f GB, median of %d" % (N, n, s.u.numel() * 8 / 1e9, reps))
    bs, bd, bmask, bbounds = detector_times(s, lim, reps, "built-in")
    u0 = s.u.clone()
    dt = 0.4 / n / ((2 * N - 1) * dim * float(s.max_eigenvalue()[0]))
    restore = lambda: (s._u.copy_(u0), setattr(s, "time", 0.0))
    n_tr = int(lim.step_a_posteriori(dt))
    lim.check(wait=True)
    t_post, _ = timed(lambda: lim.step_a_posteriori(dt), max(3, reps // 2), before=restore)
    lim.check(wait=True)
    print("built-in   step_a_posteriori(dt) %.3f ms, %d of %d cells troubled" % (t_post, n_tr, ncell))
    del s, lim, u0
    torch.cuda.empty_cache()

    g = exa.AderDgSolver(dim, N, nc, pde=euler_with_criterion().register(), n_vars=5, dx=[1.0 / n] * dim)
    glim = exa.SubcellLimiter(g, capacity=16)
    fill(g, n)
    gs, gd, gmask, gbounds = detector_times(g, glim, reps, "generated")
    print("masks equal: %s, bounds equal: %s" % (bool(torch.equal(bmask, gmask)), bool(torch.equal(bbounds, gbounds))))
    print("generated / built-in: snapshot %.3f, detect %.3f" % (gs / bs, gd / bd))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 5)

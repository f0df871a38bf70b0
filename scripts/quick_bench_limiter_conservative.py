#!/usr/bin/env python3
"""Times the a-posteriori limited step without and with the conservative DG / FV interface (HIP events, after warm-up), one shape per process:

    python scripts/quick_bench_limiter_conservative.py N CELLS_PER_AXIS [reps = 5] [rounds = 3]     (3-D, Euler; run each shape under its own `timeout`)

  step_a_posteriori(dt)                                  the default: what the parent commit runs too (same script part, comparable)
  step_a_posteriori(dt, conservative=True, rounds=R)     R rounds of detect / project / face flux / FV update / reconstruct / correct
  exa_lim_face_flux, exa_lim_interface_correct           the two new kernels alone, on the troubled cells of the first round
State: the one of scripts/quick_bench_limiter_mood.py -- a smooth density wave with node-wise noise in 5 % of the cells (Bernoulli-seeded)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from exahype_amd import solvers as exa


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


def main(N, n, reps=5, rounds=3):
    dim, nc = 3, (n, n, n)
    s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / n] * dim)
    ncell = n ** 3
    lim = exa.SubcellLimiter(s, capacity=int(0.2 * ncell))
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
    u0 = u.clone()
    dt = 0.4 / n / ((2 * N - 1) * dim * float(s.max_eigenvalue()[0]))
    restore = lambda: (s._u.copy_(u0), setattr(s, "time", 0.0))
    print("3-D N = %d, %d^3 cells, u = %.2f GB, dt = %.3e" % (N, n, u.numel() * 8 / 1e9, dt))

    restore()
    n_tr = int(lim.step_a_posteriori(dt))                   # warm-up
    lim.check(wait=True)
    t_plain, t_plain_min = timed(lambda: lim.step_a_posteriori(dt), reps, before=restore)
    print("troubled cells: %d of %d (%.1f %%)" % (n_tr, ncell, 100.0 * n_tr / ncell))
    print("step_a_posteriori(dt)                              median %.3f ms  min %.3f ms" % (t_plain, t_plain_min))
    if not hasattr(lim, "_conservative_setup"):
        return                                              # (a commit without the conservative interface: the line above is the comparison)
    restore()
    n_cum = int(lim.step_a_posteriori(dt, conservative=True, rounds=rounds))
    lim.check(wait=True)
    t_cons, t_cons_min = timed(lambda: lim.step_a_posteriori(dt, conservative=True, rounds=rounds), reps, before=restore)
    print("step_a_posteriori(dt, conservative=True, rounds=%d) median %.3f ms  min %.3f ms  (+%.3f ms = %.1f %%); cumulative mask %d cells"
          % (rounds, t_cons, t_cons_min, t_cons - t_plain, 100 * (t_cons - t_plain) / t_plain, n_cum))
    # the two kernels alone, on the first round's troubled cells
    restore()
    lim._snapshot(s.u, lim._u_old)
    s.step(dt)
    m = lim._detect(s.u, 1e-4, 1e-3, 1e-12).clone()
    lim._compact(m.reshape(-1))
    lim._project(m.reshape(-1), lim._u_old, 0.0)
    lim._face_flux()
    t_ff, _ = timed(lim._face_flux, reps)
    lim._interface_correct(m, dt)
    t_ic, _ = timed(lambda: lim._interface_correct(m, dt), reps)
    print("exa_lim_face_flux          %8.3f ms over %d slots (%d troubled)" % (t_ff, lim.capacity, int(m.sum())))
    print("exa_lim_interface_correct  %8.3f ms (six launches)" % t_ic)


if __name__ == "__main__":
    a = sys.argv
    main(int(a[1]), int(a[2]), int(a[3]) if len(a) > 3 else 5, int(a[4]) if len(a) > 4 else 3)

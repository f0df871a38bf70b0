#!/usr/bin/env python3
"""Times the a-posteriori limiter's two kernels and its step with HIP events, after warm-up, on one shape per process:

    python scripts/quick_bench_limiter_mood.py N CELLS_PER_AXIS [reps = 5]        (3-D, Euler; run each shape under its own `timeout`)

  exa_lim_snapshot, exa_lim_detect      bytes moved / time against the measured copy rate of 6.29 TB/s
  SubcellLimiter.detect()               the a-priori indicator in torch ops on the same state
  step_a_posteriori against step(mask)  the same troubled cells; overhead in ms and as a share of the step
State: a smooth density wave with node-wise noise in 5 % of the cells, so that the candidate of a CFL-0.4 step is troubled there."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from exahype_amd import solvers as exa

COPY_RATE = 6.29e12


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


def main(N, n, reps=5):
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
    ubytes = u.numel() * 8
    print("3-D N = %d, %d^3 cells, u = %.2f GB, dt = %.3e" % (N, n, ubytes / 1e9, dt))

    lim._mood_setup()
    for _ in range(2):
        lim._snapshot(s.u, lim._u_old)
        lim._detect(s.u, 1e-4, 1e-3, 1e-12)
    t_snap, _ = timed(lambda: lim._snapshot(s.u, lim._u_old), reps)
    t_bnd, _ = timed(lambda: lim._snapshot(s.u, None), reps)
    t_det, _ = timed(lambda: lim._detect(s.u, 1e-4, 1e-3, 1e-12), reps)
    lim.detect()
    t_torch, _ = timed(lambda: lim.detect(), reps)
    for name, t, nbytes in (("exa_lim_snapshot (copy + bounds)", t_snap, 2 * ubytes), ("exa_lim_snapshot (bounds only)", t_bnd, ubytes),
                            ("exa_lim_detect", t_det, ubytes)):
        print("%-34s %8.3f ms  %6.2f TB/s  %5.1f %% of the copy rate" % (name, t, nbytes / t / 1e9, 100 * nbytes / (t * 1e-3) / COPY_RATE))
    print("%-34s %8.3f ms" % ("SubcellLimiter.detect() (torch ops)", t_torch))
    print("snapshot + detect = %.3f ms = %.2f x the torch detect()" % (t_snap + t_det, (t_snap + t_det) / t_torch))

    restore()
    n_tr = int(lim.step_a_posteriori(dt))                   # warm-up; its mask serves step()
    mask = lim._mask.clone()
    lim.check(wait=True)
    t_post, _ = timed(lambda: lim.step_a_posteriori(dt), max(3, reps // 2), before=restore)
    restore()
    lim.step(dt, mask)
    t_step, _ = timed(lambda: lim.step(dt, mask), max(3, reps // 2), before=restore)
    lim.check(wait=True)
    print("troubled cells: %d of %d (%.1f %%)" % (n_tr, ncell, 100.0 * n_tr / ncell))
    print("step(dt, mask) %.3f ms; step_a_posteriori(dt) %.3f ms; overhead %.3f ms = %.1f %% of the step" %
          (t_step, t_post, t_post - t_step, 100 * (t_post - t_step) / t_step))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 5)

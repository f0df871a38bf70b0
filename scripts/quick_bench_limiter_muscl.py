#!/usr/bin/env python3
"""Times the limiter's patch pipeline in both modes with HIP events, after warm-up: the first-order path (patches with halo 1, the yardstick of
the same session) against the second-order one (SubcellLimiter(fv_mode=FV_MUSCL_HANCOCK): patches with halo 2).

    python scripts/quick_bench_limiter_muscl.py [reps = 5] [out = profiles/limiter_muscl.txt]

Shapes: 2-D N = 8 on 256 x 256 cells and 3-D N = 5 on 32^3 cells (Euler), 5 % of the cells troubled (a fixed Bernoulli mask).  Per launch,
the two modes alternating: the projection, the FV patch update and the reconstruction over the capacity-sized patch list; then a whole
step(dt, mask).  A sample is one event pair around K_LAUNCH back-to-back launches (K_STEP steps), so that the window is milliseconds and not one
launch's overhead; the figure is the window over the count.  Median of `reps` samples after warm-up; the ratio is second order / first order.  The table goes to stdout and to `out`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from exahype_amd import solvers as exa

SHAPES = [(2, 8, 256), (3, 5, 32)]          # (dim, N, cells per axis)
K_LAUNCH, K_STEP = 50, 5                     # launches / steps inside one timed window


def timed(fn, before=None, k=1):
    """ms per call of fn over k back-to-back calls between one pair of events"""
    if before is not None:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def shape_rows(dim, N, n, reps):
    nc = (n,) * dim
    ncell = n ** dim
    g = torch.Generator(device="cuda").manual_seed(7)
    mask = torch.rand(nc, generator=g, device="cuda") < 0.05
    n_tr = int(mask.sum())
    cap = int(1.2 * n_tr)
    sol, lim = {}, {}
    for mode in (exa.FV_RUSANOV, exa.FV_MUSCL_HANCOCK):
        s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / n] * dim)
        X = s.node_positions().reshape(s.u.shape[:-1] + (3,))
        rho = 1.0 + 0.2 * torch.sin(2 * torch.pi * X[..., :dim].sum(-1))
        u = s.u
        u[..., 0] = rho
        for a in range(dim):
            u[..., 1 + a] = 0.1 * (a + 1) * rho
        u[..., 4] = 1.0 / 0.4 + 0.5 * rho * 0.14
        sol[mode], lim[mode] = s, exa.SubcellLimiter(s, capacity=cap, fv_mode=mode)
    s0 = sol[exa.FV_RUSANOV]
    u0 = s0.u.clone()
    dt = 0.4 / n / ((2 * N - 1) * dim * float(s0.max_eigenvalue()[0]))
    m = mask.reshape(-1)
    stages = {}
    for mode in lim:
        L, s = lim[mode], sol[mode]
        L._compact(m)
        restore = lambda s=s: (s._u.copy_(u0), setattr(s, "time", 0.0))             # noqa: E731
        stages[mode] = [
            ("projection", lambda L=L, s=s: L._project(m, s.u, 0.0), restore),
            # (the update runs in place: the window starts from freshly projected patches and repeats the update on what it left -- the halos stay)
            ("FV patch update", lambda L=L, s=s: L._fv.time_step(L._patches.reshape(-1), dt, s.dx[0] / L.Ns, slot=L._cells), lambda L=L, s=s: L._project(m, s.u, 0.0)),
            ("reconstruction", lambda L=L, s=s: _reconstruct(L, s), None),
            ("step(dt, mask)", lambda L=L: L.step(dt, mask), restore),
        ]
    rows = []
    names = [name for name, _, _ in stages[exa.FV_RUSANOV]]
    for k, name in enumerate(names):
        count = K_STEP if name.startswith("step") else K_LAUNCH
        ms = {mode: [] for mode in lim}
        for mode in lim:                                       # warm-up
            for _ in range(2):
                timed(stages[mode][k][1], stages[mode][k][2])
        for _ in range(reps):                                  # the two modes alternate
            for mode in lim:
                ms[mode].append(timed(stages[mode][k][1], stages[mode][k][2], count))
        t1, t2 = median(ms[exa.FV_RUSANOV]), median(ms[exa.FV_MUSCL_HANCOCK])
        rows.append((name, t1, t2))
    for L in lim.values():
        L.check(wait=True)
    head = "%d-D N = %d, %d^%d cells, %d troubled (%.1f %%), capacity %d, patch %d | %d doubles" % (
        dim, N, n, dim, n_tr, 100.0 * n_tr / ncell, cap, lim[exa.FV_RUSANOV].patch_doubles, lim[exa.FV_MUSCL_HANCOCK].patch_doubles)
    return head, rows


def _reconstruct(L, s):
    import ctypes as C
    ptr = lambda t: C.c_void_p(t.data_ptr())                   # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if L.fv_halo == 2:
        exa.check(s.lib.exa_lim_reconstruct_patches_halo(s._plan, ptr(L._patches), ptr(L._cells), L.capacity, ptr(s.u), 2, stream))
    else:
        exa.check(s.lib.exa_dg_reconstruct_patches(s._plan, ptr(L._patches), ptr(L._cells), L.capacity, ptr(s.u), stream))


def main(reps=5, out=None):
    lines = ["limiter patch pipeline, first order (halo 1) against second order (halo 2); ms per launch: median of %d windows of %d launches (%d steps) "
             "after warm-up" % (reps, K_LAUNCH, K_STEP)]
    for dim, N, n in SHAPES:
        head, rows = shape_rows(dim, N, n, reps)
        lines += ["", head, "%-18s %12s %12s %8s" % ("", "halo 1", "halo 2", "ratio")]
        lines += ["%-18s %12.3f %12.3f %8.2f" % (name, t1, t2, t2 / t1) for name, t1, t2 in rows]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, sys.argv[2] if len(sys.argv) > 2 else os.path.join("profiles", "limiter_muscl.txt"))

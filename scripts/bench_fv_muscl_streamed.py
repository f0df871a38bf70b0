"""Time of the plane-streaming MUSCL-Hancock patch update (fv_muscl_stream_kernel; FVRusanovKernel(stream_planes=...)) beside the resident kernel
and the Rusanov mode (profiles/fv_muscl_streamed.txt), taken the way scripts/quick_bench_fv_muscl.py takes its numbers.

    python scripts/bench_fv_muscl_streamed.py [repeats = 5] [--resident-only] [--limited] [--tree DIR]

Euler, H = 2, 5 variables, dt / h = 0.01; per form the median of `repeats` launches timed by device events after two warm-up launches, the forms
alternating inside every repeat, all in one process and each on its own copy of the same array.

  1. 3-D P = 8, 32 768 patches: the resident kernel against FV_STREAM_ALWAYS (and the Rusanov mode).
  2. 3-D P = 11 and P = 15 at the same number of interior volumes (12 605 and 4 971 patches for 16.8 M volumes): FV_STREAM_IF_NEEDED against the
     Rusanov mode on the same arrays; ns per interior volume beside the P = 8 figures.
  --limited   3. a limited step shaped like configuration 4 (3-D Euler N = 8, 32^3 cells, Bernoulli(0.05) mask): SubcellLimiter with
              fv_mode=FV_RUSANOV against FV_MUSCL_HANCOCK + FV_STREAM_IF_NEEDED on the same mask, and the plain DG step.
  --resident-only  the resident P = 8 kernel alone; with --tree DIR exahype_amd is imported from another checkout (built there): how the
              instantiation of the commit before is timed against this one's, in alternating processes.
"""
import os
import sys

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
RESIDENT_ONLY = "--resident-only" in sys.argv
LIMITED = "--limited" in sys.argv
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    ARGS.remove(TREE)
sys.path.insert(0, TREE)
import numpy as np
import torch

from exahype_amd import solvers as exa

DT, H_VOLUME, HALO, M = 1e-3, 0.1, 2, 5
VOLUMES = 32768 * 8 ** 3


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def euler_patches(n, P):
    S = P + 2 * HALO
    g = torch.Generator(device="cuda").manual_seed(7)
    Q = torch.rand((n,) + (S,) * 3 + (M,), dtype=torch.float64, device="cuda", generator=g)
    Q[..., 0] += 1.0                                              # density in [1, 2]
    Q[..., 1:4] -= 0.5                                            # momenta in [-1/2, 1/2]
    Q[..., 4] += 2.5                                              # energy in [2.5, 3.5]: p > 0.8
    return Q


def alternate(forms, repeats):
    """forms: [(label, callable)] -> {label: [ms]} with the forms alternating inside every repeat, two warm-up rounds"""
    ms = {label: [] for label, _ in forms}
    for k in range(repeats + 2):
        for label, fn in forms:
            t = timed(fn)
            if k >= 2:
                ms[label].append(t)
    return ms


def patch_shape(P, n, forms, repeats):
    Q0 = euler_patches(n, P)
    runs, arrays = [], []
    for label, mode, sp in forms:
        kw = {} if sp is None else {"stream_planes": sp}
        kern = exa.FVRusanovKernel(3, P, HALO, M, 0, n, exa.PDE_EULER, mode, **kw)
        Q = Q0.clone()
        arrays.append((label, Q))
        form = "streamed" if getattr(kern, "streamed", False) else "resident"
        runs.append(("%s (%s)" % (label, form) if mode == exa.FV_MUSCL_HANCOCK else label, (lambda k=kern, q=Q: k.time_step(q, DT, H_VOLUME))))
    ms = alternate(runs, repeats)
    print("3-D P = %d, %d patches (%d interior volumes), H = 2, Euler 5 + 0; median of %d after 2 warm-up launches" % (P, n, n * P ** 3, repeats))
    for (label, _), (_, Q) in zip(runs, arrays):
        assert bool(torch.isfinite(Q).all()), label
        med = float(np.median(ms[label]))
        print("  %-26s %8.4f ms per launch (min %.4f, max %.4f)   %.4f ns per interior volume"
              % (label, med, min(ms[label]), max(ms[label]), med * 1e6 / (n * P ** 3)))
    del arrays, runs
    torch.cuda.empty_cache()


def limited(repeats):
    import bench
    N, n = 8, 32
    dx = [1.0 / n] * 3
    rows = []
    for label, kw in (("plain DG step", None), ("limited, FV_RUSANOV", dict(fv_mode=exa.FV_RUSANOV)),
                      ("limited, FV_MUSCL_HANCOCK streamed", dict(fv_mode=exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_IF_NEEDED))):
        s = exa.AderDgSolver(3, N, (n,) * 3, dx=dx)
        lam = bench.synthetic_state(s, [0, 0, 0], [1, 1, 1], seed=4)      # the benchmark's density wave
        mask = torch.rand((n,) * 3, generator=torch.Generator(device=s.dev).manual_seed(4), device=s.dev) < 0.05
        dt = 0.1 * dx[0] / (15 * 3 * lam)
        if kw is None:
            rows.append((label, s, None, (lambda s=s: s.step(dt))))
        else:
            lim = exa.SubcellLimiter(s, capacity=int(0.08 * n ** 3) + 16, **kw)
            rows.append((label, s, lim, (lambda lim=lim, mask=mask: lim.step(dt, mask))))
    ms = alternate([(label, fn) for label, _, _, fn in rows], repeats)
    print("limited step, 3-D Euler N = 8, %d^3 cells, Bernoulli(0.05) mask (%d troubled cells, patches of 15^3 volumes); median of %d after 2 warm-up steps"
          % (n, int(mask.sum()), repeats))
    for label, s, lim, _ in rows:
        if lim is not None:
            lim.check(wait=True)
        assert bool(torch.isfinite(s.u).all()), label
        print("  %-36s %8.3f ms per step (min %.3f, max %.3f)" % (label, float(np.median(ms[label])), min(ms[label]), max(ms[label])))


def main(repeats=5):
    if not torch.cuda.is_available():
        raise SystemExit("bench_fv_muscl_streamed.py measures on a GPU: none is available")
    print("exahype_amd from %s" % os.path.dirname(os.path.abspath(exa.__file__)))
    if RESIDENT_ONLY:
        patch_shape(8, 32768, [("muscl-hancock", exa.FV_MUSCL_HANCOCK, None)], repeats)
        return
    if LIMITED:
        limited(repeats)
        return
    patch_shape(8, 32768, [("rusanov", exa.FV_RUSANOV, None), ("muscl-hancock", exa.FV_MUSCL_HANCOCK, exa.FV_STREAM_NEVER),
                           ("muscl-hancock, ALWAYS", exa.FV_MUSCL_HANCOCK, exa.FV_STREAM_ALWAYS)], repeats)
    for P in (11, 15):
        patch_shape(P, VOLUMES // P ** 3, [("rusanov", exa.FV_RUSANOV, None), ("muscl-hancock", exa.FV_MUSCL_HANCOCK, exa.FV_STREAM_IF_NEEDED)], repeats)


if __name__ == "__main__":
    main(*(int(a) for a in ARGS[:1]))

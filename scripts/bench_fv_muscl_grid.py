"""Time per step of the MUSCL-Hancock patch grid in its three forms, in one process (profiles/fv_muscl_grid_one_launch.txt).

    python scripts/bench_fv_muscl_grid.py [repeats = 9] [warm-up = 3]

Forms:  one launch   FVPatchGrid(fused=FUSED_EDGES).step -- exa_fv_grid_step_muscl_device on halo-less arrays (halo gather, update and the next
                     step's CFL scan in one kernel)
        two passes   FVPatchGrid(fused=False).step -- the halo fill by torch ops on the array with halo, then the in-place update
        bare kernel  FVRusanovKernel.time_step on that array with halo, halos as they are: the update alone
and, as a step of run() costs it, `max_eigenvalue()` (the host read of the CFL scan) + step for the first two: the one-launch form finds the
scan where its last step left it, the two-pass form launches one.

Shapes: 2-D P = 4 on a 1024 x 1024 grid (2^20 patches) and 3-D P = 8 on a 32 x 32 x 32 grid (32 768 patches), H = 2, 5 variables, Euler, periodic.
Per form the median of `repeats` steps timed by device events after `warm-up` untimed ones; the forms alternate inside a repeat, so a drift of
the machine reaches all of them alike.  The step is small (dt / h = 0.01): the states stay admissible over all repeats.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from exahype_amd import solvers as exa

SHAPES = ((2, (1024, 1024), 4), (3, (32, 32, 32), 8))
DT, H_VOLUME = 1e-3, 0.1


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def main(repeats=9, warmup=3):
    if not torch.cuda.is_available():
        raise SystemExit("bench_fv_muscl_grid.py measures on a GPU: none is available")
    m = V = 5
    for dim, grid, P in SHAPES:
        n = int(np.prod(grid))
        gen = torch.Generator(device="cuda").manual_seed(7)
        U0 = torch.rand(grid + (P,) * dim + (V,), dtype=torch.float64, device="cuda", generator=gen)
        U0[..., 0] += 1.0                                         # density in [1, 2]
        U0[..., 1:4] -= 0.5                                       # momenta in [-1/2, 1/2]
        U0[..., 4] += 2.5                                         # energy in [2.5, 3.5]: p > 0.8
        length = H_VOLUME * grid[0] * P
        one = exa.FVPatchGrid(dim, grid, P, 2, m, V - m, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, length=length, fused=exa.FUSED_EDGES)
        two = exa.FVPatchGrid(dim, grid, P, 2, m, V - m, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, length=length, fused=False)
        one.set_interior(U0)
        two.set_interior(U0)
        one.step(DT)
        two.step(DT)
        same = bool(torch.equal(one.interior_device(), two.interior_device()))
        bare_q = two.with_halo()

        def run_step(g):
            g.max_eigenvalue()
            g.step(DT)
        forms = (("one launch", lambda: one.step(DT)), ("two passes", lambda: two.step(DT)),
                 ("bare kernel", lambda: two.kernel.time_step(bare_q, DT, two.h)),
                 ("one launch + scan", lambda: run_step(one)), ("two passes + scan", lambda: run_step(two)))
        ms = {name: [] for name, _ in forms}
        for k in range(warmup + repeats):
            for name, fn in forms:
                t = timed(fn)
                if k >= warmup:
                    ms[name].append(t)
        assert bool(torch.isfinite(one.interior_device()).all()) and bool(torch.isfinite(two.interior_device()).all())
        med = {name: float(np.median(v)) for name, v in ms.items()}
        print("%d-D P = %d, grid %s (%d patches), H = 2, V = %d, Euler, periodic; median of %d after %d warm-up steps; first step bit-equal in both forms: %s"
              % (dim, P, "x".join(str(g) for g in grid), n, V, repeats, warmup, same))
        for name, _ in forms:
            print("  %-18s %8.4f ms per step   (min %.4f, max %.4f)" % (name, med[name], min(ms[name]), max(ms[name])))
        print("  one launch / two passes = %.3f; one launch / bare kernel = %.3f; with the CFL scan of run(): one launch / two passes = %.3f"
              % (med["one launch"] / med["two passes"], med["one launch"] / med["bare kernel"], med["one launch + scan"] / med["two passes + scan"]))
        del one, two, bare_q, U0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))

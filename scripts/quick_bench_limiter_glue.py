#!/usr/bin/env python3
"""Times the limiter glue kernels at the variable counts no bench.py config covers, HIP events after warm-up, on one shape per process:

    python scripts/quick_bench_limiter_glue.py DIM N CELLS_PER_AXIS NV [reps = 5]        (run each shape under its own `timeout`)

  exa_dg_project_patches        the troubled cells of a fixed Bernoulli(0.05) cell list -> patches with halo 1
  exa_lim_face_layers           all 2 DIM block faces, every cell of the boundary layer (need = NULL)
  exa_dg_reconstruct_patches    the same patches -> the cells of the list
NV = 1: the built-in advection; NV = 2: the generated term set `reaction_advection` of tests/test_user_pde.py; NV = 5: Euler.  The shapes
of profiles/limiter_unit_refactor.txt: 3 8 64 (cfg 4's) and 2 4 512.  A sample is one event pair around K back-to-back launches; the
figure is the window over K, the median of `reps` windows.  One line per kernel; EXA_LIB selects another build of the library."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from exahype_amd import solvers as exa

K = 20                                        # launches inside one timed window


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(K):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / K


def median(fn, reps):
    window(fn)                                # warm-up
    ms = sorted(window(fn) for _ in range(reps))
    return ms[len(ms) // 2]


def main(dim, N, n, nv, reps=5):
    nc = (n,) * dim
    if nv == 5:
        s = exa.AderDgSolver(dim, N, nc)
    elif nv == 1:
        s = exa.AderDgSolver(dim, N, nc, pde=exa.PDE_ADVECTION, n_vars=1)
    else:
        from tests.test_user_pde import reaction_advection
        assert nv == 2
        s = exa.AderDgSolver(dim, N, nc, pde=reaction_advection().register(), n_vars=2)
    g = torch.Generator(device="cuda").manual_seed(7)
    s.u.copy_(torch.rand(s.u.shape, generator=g, device="cuda", dtype=torch.float64) + 1.0)
    cells = torch.nonzero(torch.rand(n ** dim, generator=g, device="cuda") < 0.05).reshape(-1).contiguous()
    ncell = int(cells.numel())
    ptr = lambda t: C.c_void_p(t.data_ptr())                       # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    patches = torch.zeros(ncell * s.lib.exa_lim_patch_count(s._plan), dtype=torch.float64, device="cuda")
    layers = [torch.zeros(s.lib.exa_lim_face_layer_count(s._plan, d), dtype=torch.float64, device="cuda") for d in range(dim)]

    def project():
        exa.check(s.lib.exa_dg_project_patches(s._plan, ptr(s.u), ptr(cells), ncell, ptr(patches), stream))

    def face_layers():
        for d in range(dim):
            for side in (0, 1):
                exa.check(s.lib.exa_lim_face_layers(s._plan, ptr(s.u), d, side, None, ptr(layers[d]), stream))

    def reconstruct():
        exa.check(s.lib.exa_dg_reconstruct_patches(s._plan, ptr(patches), ptr(cells), ncell, ptr(s.u), stream))

    head = "%d-D N = %d, %d^%d cells, nv = %d, %d cells listed" % (dim, N, n, dim, nv, ncell)
    for name, fn in (("exa_dg_project_patches", project), ("exa_lim_face_layers (all faces)", face_layers), ("exa_dg_reconstruct_patches", reconstruct)):
        print("%s | %-32s %9.4f ms" % (head, name, median(fn, reps)), flush=True)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(*a)

"""Time per launch of the MUSCL-Hancock patch update beside the Rusanov mode on the same arrays (profiles/fv_muscl_hancock.txt).

    python scripts/quick_bench_fv_muscl.py [repeats = 5]

Shapes: 2-D P = 4 with 2^20 patches and 3-D P = 8 with 32 768 patches, H = 2, 5 variables, Euler.  Per shape: the median of `repeats` timed
launches after a warm-up, for both modes in one process; the algorithmic bytes 8 (S^dim V + P^dim n_real) per patch (the array read once,
the interior's evolved variables written once) against the 6.29 TB/s copy rate; the ratio of the two modes.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from exahype_amd import solvers as exa

COPY_RATE = 6.29e12
SHAPES = ((2, 4, 1 << 20), (3, 8, 32768))


def median_ms(kern, Q, dt, h, repeats):
    ms = []
    for k in range(repeats + 2):                                  # two warm-up launches
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        kern.time_step(Q, dt, h)
        stop.record()
        stop.synchronize()
        if k >= 2:
            ms.append(start.elapsed_time(stop))
    return float(np.median(ms))


def main(repeats=5):
    H, m, V = 2, 5, 5
    for dim, P, n in SHAPES:
        S = P + 2 * H
        g = torch.Generator(device="cuda").manual_seed(7)
        Q0 = torch.rand((n,) + (S,) * dim + (V,), dtype=torch.float64, device="cuda", generator=g)
        Q0[..., 0] += 1.0                                         # density in [1, 2]
        Q0[..., 1:4] -= 0.5                                       # momenta in [-1/2, 1/2]
        Q0[..., 4] += 2.5                                         # energy in [2.5, 3.5]: p > 0.8
        dt, h = 1e-3, 0.1
        bytes_pp = 8 * (S ** dim * V + P ** dim * m)
        t = {}
        for name, mode in (("rusanov", exa.FV_RUSANOV), ("muscl-hancock", exa.FV_MUSCL_HANCOCK)):
            kern = exa.FVRusanovKernel(dim, P, H, m, V - m, n, exa.PDE_EULER, mode)
            Q = Q0.clone()
            t[name] = median_ms(kern, Q, dt, h, repeats)
            assert bool(torch.isfinite(Q).all())
            at_copy = n * bytes_pp / COPY_RATE * 1e3
            print("%d-D P = %d, %d patches, %-13s: %.4f ms per launch; algorithmic %.1f MB -> %.4f ms at 6.29 TB/s (%.2f of it)"
                  % (dim, P, n, name, t[name], n * bytes_pp / 1e6, at_copy, at_copy / t[name]))
        print("%d-D P = %d: muscl-hancock / rusanov = %.2f" % (dim, P, t["muscl-hancock"] / t["rusanov"]))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5)

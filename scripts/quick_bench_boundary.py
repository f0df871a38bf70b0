"""Cost of domain boundaries on the bench.py default configuration (3-D Euler, p = 5, 128^3 cells): the periodic step against walls on all
six faces and against a time-dependent Dirichlet datum on all six faces -- development aid.  usage: quick_bench_boundary.py [cells] [steps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from exahype_amd import solvers as exa  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
N = 6


def datum(X, t):
    rho = 1.0 + 0.1 * torch.sin(6.0 * X[:, 0] + 4.0 * X[:, 1] - 2.0 * X[:, 2] - t)
    z = torch.zeros_like(rho)
    return torch.stack([rho, 0.1 * rho, z, z, 2.5 + 0.005 * rho], -1)


FACES = [(a, s) for a in range(3) for s in range(2)]
CASES = [("periodic", None), ("walls", {f: exa.Wall() for f in FACES}), ("dirichlet_f", {f: exa.Dirichlet(datum) for f in FACES})]
res = {}
for name, bc in CASES + CASES[:1]:                 # (the periodic step once more at the end: drift of the clocks)
    s = exa.AderDgSolver(3, N, (n, n, n), boundary=bc)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    s.u.copy_(torch.rand(s.u.shape, generator=g, device="cuda", dtype=torch.float64) * 0.1)
    s.u[..., 0] += 1.0
    s.u[..., 4] += 2.5
    dt = 1e-5
    for _ in range(2):
        s.step(dt)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        s.step(dt)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    res.setdefault(name, []).append(ms)
    pts = sum(int(buf.shape[0]) * s.nf * N for _, _, b, _, buf in s._bc if isinstance(b, exa.Dirichlet)) if bc else 0
    print(f"{n}^3 p=5 {name}: {ms:.2f} ms/step  finite={bool(torch.isfinite(s.u).all())}  f points/step={pts}", flush=True)
    del s
    torch.cuda.empty_cache()
base = min(res["periodic"])
for name in ("walls", "dirichlet_f"):
    print(f"{name}: {res[name][0] / base:.4f} x the periodic step ({base:.2f} ms)")

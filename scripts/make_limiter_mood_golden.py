#!/usr/bin/env python3
"""Writes tests/golden/limiter_mood_tube.json: L1(rho), min rho, min p, troubled-cell maximum and conservation defects of the numpy
restatement of the a-posteriori limiter (tests/limiter_mood_ref.py) on the periodic double Sod tube, for the cases the GPU tests
compare SubcellLimiter.run against.  CPU only; the 3-D cases are nx x 1 x 1 cells.  Takes about a quarter of an hour (p = 7 at 32 cells).

    python scripts/make_limiter_mood_golden.py [-j PROCESSES]
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(2, 4, 16), (2, 4, 32), (2, 4, 64), (3, 6, 16), (3, 6, 32), (3, 8, 16), (3, 8, 32)]      # (dim, N, nx)


def key(dim, N, nx):
    return "dim%d_N%d_nx%d" % (dim, N, nx)


def one(case):
    from tests import limiter_mood_ref as M
    dim, N, nx = case
    r = M.run_tube(N, nx, dim)
    print(key(*case), r, flush=True)
    return key(*case), r


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=min(len(CASES), os.cpu_count() or 1))
    args = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    with multiprocessing.Pool(args.j) as pool:
        res = dict(pool.map(one, sorted(CASES, key=lambda c: -c[1] ** c[0] * c[2] ** 2), chunksize=1))
    out = dict(problem="periodic double Sod tube along x, nx x 1 (x 1) cells, t_end = 0.1, CFL 0.4, d0 = 1e-4, eps = 1e-3, floor = 1e-12",
               source="tests/limiter_mood_ref.py run_tube (numpy restatement; scripts/make_limiter_mood_golden.py)",
               cases={key(*c): res[key(*c)] for c in CASES})
    path = os.path.join(ROOT, "tests", "golden", "limiter_mood_tube.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)

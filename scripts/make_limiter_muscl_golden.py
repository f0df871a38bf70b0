#!/usr/bin/env python3
"""Writes tests/golden/limiter_muscl_tube.json: steps, L1(rho), min rho, min p, troubled-cell maximum and conservation defects of the numpy
restatement of the a-posteriori limiter with the second-order patch update (tests/limiter_muscl_ref.py run_tube) on the periodic double Sod
tube, for the cases the GPU tests compare SubcellLimiter(fv_mode=FV_MUSCL_HANCOCK).run against -- and "rusanov_l1", L1(rho) of the same
restatement with the first-order update of the same windows.  CPU only; the 3-D case is nx x 1 x 1 cells.

Every recorded run must keep each decision of the detector at a relative distance of at least 1e-8 from its threshold
(limiter_ref.smallest_margin): rounding differences between this restatement and the kernels then cannot flip a mask.  A case that falls
below is replaced by another cell count, not excused.

    python scripts/make_limiter_muscl_golden.py [-j PROCESSES]
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(2, 4, 16), (3, 4, 16)]      # (dim, N, nx)
MARGIN = 1e-8


def key(dim, N, nx):
    return "dim%d_N%d_nx%d" % (dim, N, nx)


def one(case):
    from tests import limiter_muscl_ref as M2
    from tests import limiter_ref as LR
    dim, N, nx = case
    LR.reset_margin()
    r = M2.run_tube(N, nx, dim)
    r["smallest_margin"] = LR.smallest_margin()
    assert "failed" not in r, r
    assert r["smallest_margin"] >= MARGIN, "%s: a decision of the detector lies %.3e from its threshold" % (key(*case), r["smallest_margin"])
    r["rusanov_l1"] = M2.run_tube(N, nx, dim, scheme="rusanov")["l1"]
    print(key(*case), r, flush=True)
    return key(*case), r


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=min(len(CASES), os.cpu_count() or 1))
    args = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    with multiprocessing.Pool(args.j) as pool:
        res = dict(pool.map(one, CASES, chunksize=1))
    out = dict(problem="periodic double Sod tube along x, nx x 1 (x 1) cells, t_end = 0.1, CFL 0.4, d0 = 1e-4, eps = 1e-3, floor = 1e-12",
               source="tests/limiter_muscl_ref.py run_tube (numpy restatement; scripts/make_limiter_muscl_golden.py)",
               cases={key(*c): res[key(*c)] for c in CASES})
    path = os.path.join(ROOT, "tests", "golden", "limiter_muscl_tube.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)

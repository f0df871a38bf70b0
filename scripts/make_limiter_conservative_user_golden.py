#!/usr/bin/env python3
"""Writes tests/golden/limiter_conservative_dam_break.json: steps, min h, troubled-cell maximum, unresolved count, the conservation defect
of (h, hu, hv) and the depth change of the numpy restatement of the conservative a-posteriori limiter for a generated term set
(tests/limiter_conservative_user_ref.py, rounds = 3) on the periodic shallow-water double dam break.  CPU only.

    python scripts/make_limiter_conservative_user_golden.py [-j PROCESSES]
"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(2, 4, 16), (2, 6, 16), (2, 8, 16)]      # (dim, N, nx)
ROUNDS = 3


def key(dim, N, nx):
    return "dim%d_N%d_nx%d" % (dim, N, nx)


def one(case):
    from tests import limiter_conservative_user_ref as U
    dim, N, nx = case
    r = U.run_dam_break(N, nx, rounds=ROUNDS, dim=dim)
    r["bound"] = U.bound(r["steps"])
    print(key(*case), r, flush=True)
    return key(*case), r


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=min(len(CASES), os.cpu_count() or 1))
    args = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    with multiprocessing.Pool(args.j) as pool:
        res = dict(pool.map(one, sorted(CASES, key=lambda c: -c[1] ** c[0] * c[2] ** 2), chunksize=1))
    out = dict(problem="periodic double dam break along x (h = 1 | 0.1 | 1, g = 9.81), nx x 1 cells, t_end = 0.05, CFL 0.4, criterion [h], dmp = (0,), "
                       "d0 = 1e-4, eps = 1e-3, floor = 1e-12, conservative interface with %d rounds; bound = 16 steps 2^-53" % ROUNDS,
               source="tests/limiter_conservative_user_ref.py run_dam_break (numpy restatement; scripts/make_limiter_conservative_user_golden.py)",
               cases={key(*c): res[key(*c)] for c in CASES})
    path = os.path.join(ROOT, "tests", "golden", "limiter_conservative_dam_break.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)

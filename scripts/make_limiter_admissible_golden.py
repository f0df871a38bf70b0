"""Writes tests/golden/limiter_dam_break.json: the periodic double dam break for shallow water through the numpy restatement of the
a-posteriori limiter with the term set's own criterion (tests/limiter_admissible_ref.py), the values SubcellLimiter.run is held to in
tests/test_limiter_admissible.py.  Refuses to write a case in which the restatement itself does not keep h > 0.

    python scripts/make_limiter_admissible_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import limiter_admissible_ref as R      # noqa: E402

CASES = [(4, 16, 0.4), (6, 16, 0.4)]               # (N, nx, cfl): p = 3 and p = 5 on 16 x 1 cells to t = 0.05


def main():
    out = {}
    for N, nx, cfl in CASES:
        r = R.run_dam_break(N, nx, 2, t_end=0.05, cfl=cfl)
        print(r)
        if "failed" in r or not r["min_h"] > 0:
            raise SystemExit("the restatement does not keep h > 0 at N = %d, CFL %g: lower the CFL of this case here and in the test" % (N, cfl))
        out["dim2_N%d_nx%d" % (N, nx)] = r
    path = os.path.join(ROOT, "tests", "golden", "limiter_dam_break.json")
    with open(path, "w") as f:
        json.dump({"generator": "scripts/make_limiter_admissible_golden.py", "cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()

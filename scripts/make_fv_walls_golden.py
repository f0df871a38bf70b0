"""tests/golden/fv_walls_sod.json: the walled Sod tube of examples/sod_tube_fv_walls.py at 16 patches, integrated on the host by the
long-double restatement (tests/fv_boundary_ref.py) with the example's CFL rule -- the value tests/test_fv_boundary_gpu.py holds the example to.

usage: python scripts/make_fv_walls_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from examples.sod_tube_fv_walls import initial_state, l1_density
from exahype_amd import Wall
from oracle import fv_reference as R
from tests import fv_boundary_ref as B

NX, P, T_END, CFL = 16, 4, 0.1, 0.4


def main():
    U = initial_state(NX, P)
    h = 1.0 / (NX * P)
    kinds, data = B.faces_of({(0, 0): Wall(), (0, 1): Wall()}, 2, 5, 0, R.PDE_EULER)
    t, steps = 0.0, 0
    while t < T_END * (1 - 1e-14):
        lam = max(float(np.max(R.max_eigenvalue(U, d, R.PDE_EULER))) for d in range(2))
        dt = min(CFL * h / 2 / lam, T_END - t)
        U = B.grid_update(U, dt, h, 2, 5, R.PDE_EULER, kinds, data, track=False).new.astype(np.float64)
        t += dt
        steps += 1
    out = {"patches": NX, "patch_size": P, "t_end": T_END, "cfl": CFL, "steps": steps, "l1_rho": l1_density(U[..., 0], T_END)}
    with open(os.path.join(ROOT, "tests", "golden", "fv_walls_sod.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(out)


if __name__ == "__main__":
    main()

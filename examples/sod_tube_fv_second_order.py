"""The Sod shock tube of examples/sod_tube_fv_walls.py between its two walls, first and second order side by side.

`FVPatchGrid(mode=FV_RUSANOV)` is the first-order run (one launch per step: halo fill, update and CFL scan).  `FVPatchGrid(halo_size=2,
mode=FV_MUSCL_HANCOCK, fused=False)` is the second-order one: minmod slopes, an unsplit half-step predictor and the Rusanov flux of the
predicted face states.  Its stencil reads two halo layers and their edge entries, which belong to diagonal patches, so it runs in the
two-pass form -- the halo fill of the array with halo (neighbours, wrap, walls), then the in-place patch update.  At t = 0.1 no wave has
reached a wall and the exact Riemann solution is the yardstick: prints the steps, the smallest density and pressure and the L1 error of the
density of both runs (256 volumes: 1.13e-2 against 3.97e-3).

usage: python examples/sod_tube_fv_second_order.py [patches along x = 64] [patch size = 4] [t_end = 0.1]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.sod_tube_fv_walls import G, initial_state, l1_density
from exahype_amd import solvers as exa


def run(mode, nx, P, t_end, cfl):
    second = mode == exa.FV_MUSCL_HANCOCK
    g = exa.FVPatchGrid(2, (nx, 1), P, 2 if second else 1, 5, 0, exa.PDE_EULER, mode, length=1.0,
                        boundary={(0, 0): exa.Wall(), (0, 1): exa.Wall()}, fused=not second)          # axis 1 is not named: periodic
    g.set_interior(initial_state(nx, P))
    steps = g.run(t_end, cfl=cfl)
    u = g.interior()
    rho = u[..., 0]
    p = (G - 1) * (u[..., 4] - 0.5 * (u[..., 1] ** 2 + u[..., 2] ** 2 + u[..., 3] ** 2) / rho)
    return {"steps": steps, "min_rho": float(rho.min()), "min_p": float(p.min()), "l1": l1_density(rho, t_end)}


def main(nx=64, P=4, t_end=0.1, cfl=0.4):
    out = {}
    for name, mode in (("rusanov", exa.FV_RUSANOV), ("muscl_hancock", exa.FV_MUSCL_HANCOCK)):
        r = out[name] = run(mode, nx, P, t_end, cfl)
        print("%-13s: %d steps to t = %.4f on %d x 1 patches of %d x %d volumes, min rho = %.6f, min p = %.6f, L1(rho) = %.8f"
              % (name, r["steps"], t_end, nx, P, P, r["min_rho"], r["min_p"], r["l1"]))
    print("L1(rho): second order / first order = %.3f" % (out["muscl_hancock"]["l1"] / out["rusanov"]["l1"]))
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 64, int(a[1]) if len(a) > 1 else 4, float(a[2]) if len(a) > 2 else 0.1)

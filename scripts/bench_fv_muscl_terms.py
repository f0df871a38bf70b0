"""Time per one-launch MUSCL-Hancock grid step (FVPatchGrid(fused=FUSED_EDGES).step) with and without a source / a non-conservative product
(profiles/fv_muscl_terms.txt), taken the way scripts/bench_fv_muscl_grid.py takes its numbers.

    python scripts/bench_fv_muscl_terms.py [repeats = 9] [warm-up = 3] [--builtin-only] [--tree DIR]

Term sets:  euler (built in)        the hand-written exa::Euler -- the instantiation a source / ncp must leave as it was
            euler_sympy             the same system generated with muscl_hancock=True
            euler_gravity           ... with the body force as a source (muscl_terms=True)
            two_layer, no ncp       the two advected fields of tests/user_term_sets.two_layer_like(3) alone
            two_layer_like          ... with their coupling as an ncp (muscl_terms=True)
Shapes: 2-D P = 4 on a 1024 x 1024 grid (2^20 patches) and 3-D P = 8 on a 32 x 32 x 32 grid (32 768 patches), H = 2, periodic, dt / h = 0.01.
Per set the median of `repeats` steps timed by device events after `warm-up` untimed ones; the sets alternate inside a repeat.
--builtin-only times the built-in Euler set alone; --tree DIR imports exahype_amd from another checkout (built there), which is how the
instantiation of an earlier commit is timed against this one's on the same machine.
"""
import os
import sys

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
BUILTIN_ONLY = "--builtin-only" in sys.argv
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    ARGS.remove(TREE)
sys.path.insert(0, TREE)
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


def term_sets():
    """-> [(label, pde id, n_real, initial state builder)]"""
    def euler_state(shape, gen):
        U = torch.rand(shape + (5,), dtype=torch.float64, device="cuda", generator=gen)
        U[..., 0] += 1.0                                          # density in [1, 2]
        U[..., 1:4] -= 0.5                                        # momenta in [-1/2, 1/2]
        U[..., 4] += 2.5                                          # energy in [2.5, 3.5]: p > 0.8
        return U

    def fields_state(shape, gen):
        return torch.rand(shape + (2,), dtype=torch.float64, device="cuda", generator=gen) + 1.0
    sets = [("euler (built in)", exa.PDE_EULER, 5, euler_state)]
    if BUILTIN_ONLY:
        return sets
    from exahype_amd.pde_codegen import SympyPDE
    from tests import fv_muscl_grid_cases as G
    from tests import fv_muscl_terms_cases as K
    from tests import user_term_sets as T
    tl = T.two_layer_like(3)
    plain = SympyPDE(2, flux=lambda q, d: [e.subs(dict(zip(tl.q, q)), simultaneous=True) for e in tl.flux_exprs[d]],
                     max_eigenvalue=lambda q, d: tl.eig_exprs[d], max_dim=3, name="two_layer_no_ncp_muscl", muscl_hancock=True)
    sets += [("euler_sympy", G.flagged("euler_sympy").register(), 5, euler_state),
             ("euler_gravity", K.flagged(K.EG).register(), 5, euler_state),
             ("two_layer, no ncp", plain.register(), 2, fields_state),
             ("two_layer_like", K.flagged(K.TL).register(), 2, fields_state)]
    return sets


def main(repeats=9, warmup=3):
    if not torch.cuda.is_available():
        raise SystemExit("bench_fv_muscl_terms.py measures on a GPU: none is available")
    sets = term_sets()
    print("exahype_amd from %s" % os.path.dirname(os.path.abspath(exa.__file__)))
    for dim, grid, P in SHAPES:
        n = int(np.prod(grid))
        grids = []
        for label, pde, m, build in sets:
            g = exa.FVPatchGrid(dim, grid, P, 2, m, 0, pde, exa.FV_MUSCL_HANCOCK, length=H_VOLUME * grid[0] * P, fused=exa.FUSED_EDGES)
            g.set_interior(build(grid + (P,) * dim, torch.Generator(device="cuda").manual_seed(7)))
            grids.append((label, g))
        ms = {label: [] for label, _ in grids}
        for k in range(warmup + repeats):
            for label, g in grids:
                t = timed(lambda: g.step(DT))
                if k >= warmup:
                    ms[label].append(t)
        print("%d-D P = %d, grid %s (%d patches), H = 2, periodic, one launch per step; median of %d after %d warm-up steps"
              % (dim, P, "x".join(str(x) for x in grid), n, repeats, warmup))
        for label, g in grids:
            assert bool(torch.isfinite(g.interior_device()).all()), label
            print("  %-18s %8.4f ms per step   (min %.4f, max %.4f)" % (label, float(np.median(ms[label])), min(ms[label]), max(ms[label])))
        del grids
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(*(int(a) for a in ARGS[:2]))

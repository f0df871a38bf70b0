"""A decaying wave, q_t + a . grad q = -k q, first and second order side by side -- a term set with a SOURCE in the second-order mode.

The system is given as SymPy expressions in two forms that are the same PDE: the flux form (f_d = a_d q, source -k q) and the
non-conservative form (f = 0, ncp B_d dq = a_d dq, source -k q).  `SympyPDE(..., muscl_hancock=True, muscl_terms=True)` takes source and ncp
into the MUSCL-Hancock update: the source by the midpoint rule in time (half a step of it in the predictor, dt S at the half-step state), the
ncp in the predictor, as the jump term of the predicted face states and at the half-step state times the volume's slope.

`FVPatchGrid(mode=FV_RUSANOV)` is the first-order run (one launch per step), `FVPatchGrid(halo_size=2, mode=FV_MUSCL_HANCOCK,
fused=FUSED_EDGES)` the second-order one, also one launch per step.  q0 = sin 2 pi (x + y) on the periodic unit square, a = (1, 1/2), k = 1.5;
the exact solution is exp(-k t) q0(x - a t).  Prints the steps and the L1 error of both runs in both forms (64^2 volumes, t = 0.5: 5.16e-3 in
second order).

usage: python examples/advection_reaction_fv_second_order.py [patches per axis = 16] [patch size = 4] [t_end = 0.5]
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

A, K, CFL, T_END = (1.0, 0.5), 1.5, 0.4, 0.5
FORMS = ("flux", "ncp")


@functools.lru_cache(maxsize=None)
def term_set(form):
    """the wave's term set in flux form or in ncp form, for both modes of FVPatchGrid"""
    import sympy
    from exahype_amd.pde_codegen import SympyPDE
    a = [sympy.Float(x) for x in A]
    eig = lambda q, d: sympy.Abs(a[d])                                   # noqa: E731
    src = lambda q: [-sympy.Float(K) * q[0]]                            # noqa: E731
    if form == "flux":
        return SympyPDE(1, flux=lambda q, d: [a[d] * q[0]], max_eigenvalue=eig, source=src, max_dim=2, name="advection_reaction_flux",
                        muscl_hancock=True, muscl_terms=True)
    assert form == "ncp", form
    return SympyPDE(1, flux=lambda q, d: [sympy.Integer(0)], max_eigenvalue=eig, source=src, ncp=lambda q, dq, d: [a[d] * dq[0]], max_dim=2,
                    name="advection_reaction_ncp", muscl_hancock=True, muscl_terms=True)


def wave(N):
    """-> (G [N, N, 1] at t = 0, exact(t) [N, N]) on the volume centres of the unit square"""
    x = (np.arange(N) + 0.5) / N
    X, Y = np.meshgrid(x, x, indexing="ij")
    f = lambda t: np.exp(-K * t) * np.sin(2 * np.pi * ((X - A[0] * t) + (Y - A[1] * t)))     # noqa: E731
    return f(0.0)[..., None], f


def run(form, second, npatch, P, t_end, cfl=CFL):
    from exahype_amd import solvers as exa
    from oracle.fv_reference import assemble, cut_patches
    G, exact = wave(npatch * P)
    pid = term_set(form).register()
    if second:
        g = exa.FVPatchGrid(2, (npatch, npatch), P, 2, 1, 0, pid, exa.FV_MUSCL_HANCOCK, length=1.0, fused=exa.FUSED_EDGES)
    else:
        g = exa.FVPatchGrid(2, (npatch, npatch), P, 1, 1, 0, pid, exa.FV_RUSANOV, length=1.0)
    g.set_interior(cut_patches(G, 2, (npatch, npatch), P))
    steps = g.run(t_end, cfl=cfl)
    return {"steps": steps, "l1": float(np.mean(np.abs(assemble(g.interior(), 2)[..., 0] - exact(t_end))))}


def main(npatch=16, P=4, t_end=T_END):
    out = {}
    for form in FORMS:
        for name, second in (("rusanov", False), ("muscl_hancock", True)):
            r = out[form, name] = run(form, second, npatch, P, t_end)
            print("%-4s form, %-13s: %d steps to t = %.4f on %d x %d patches of %d x %d volumes, L1 = %.8e"
                  % (form, name, r["steps"], t_end, npatch, npatch, P, P, r["l1"]))
        print("%-4s form: second order / first order = %.3f" % (form, out[form, "muscl_hancock"]["l1"] / out[form, "rusanov"]["l1"]))
    return out


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 16, int(a[1]) if len(a) > 1 else 4, float(a[2]) if len(a) > 2 else T_END)

"""FVPatchGrid in mode FV_MUSCL_HANCOCK (fused=False, halo_size 2), generated term sets with muscl_hancock=True and HIPPrinter's
scheme="fv-muscl-hancock", on the GPU.

One step of the grid must equal the restatement (tests/fv_muscl_ref.py) applied to the ASSEMBLED global array, within the bound 2^-53 E in
every volume: the kernel sees patches whose halo layers the two-pass driver filled, the restatement one array with two ghost layers -- they
agree only if every halo entry the stencil reads, the EDGE entries among them, came from the right (diagonal) patch or boundary rule.  A
periodic step conserves every evolved variable to the rounding of its own updates.  The runs are the recorded ones of
tests/golden/fv_muscl_runs.json (the fp64 numpy form; tests/test_fv_muscl_reference.py).
"""
import functools
import json
import math
import os

import numpy as np
import pytest

from oracle import fv_reference as R
from tests import fv_cases as K1
from tests import fv_muscl_cases as K
from tests import fv_muscl_ref as M
from tests.util import log_fv_measurement

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fv_muscl_runs.json")))


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from exahype_amd import solvers
    return solvers


def _states(dim, V, family, seed, n):
    return K1.state(family, n, dim, 1, 0, V, seed).reshape(n, V)


def _grid_cases(exa):
    wall = exa.Wall()
    return {
        "2d-5x3-periodic": (2, (5, 3), 4, 5, 0, None),
        "2d-1x7-periodic": (2, (1, 7), 4, 5, 5, None),
        "3d-2x3x2-states": (3, (2, 3, 2), 4, 5, 0, "states"),
        "2d-3x2-wall-outflow-dirichlet": (2, (3, 2), 4, 5, 1, {(0, 0): wall, (0, 1): exa.Outflow(), (1, 0): "dirichlet", (1, 1): wall}),
    }


@pytest.mark.parametrize("family", ("benign", "riemann"))
@pytest.mark.parametrize("case", ("2d-5x3-periodic", "2d-1x7-periodic", "3d-2x3x2-states", "2d-3x2-wall-outflow-dirichlet"))
def test_grid_step_equals_the_restatement_on_the_global_array(exa, case, family):
    from exahype_amd.boundary import fv_faces
    dim, grid, P, n_real, n_aux, bc = _grid_cases(exa)[case]
    V = n_real + n_aux
    n = int(np.prod(grid))
    U = K1.state(family, n, dim, P, 0, V, 41 + dim).reshape(grid + (P,) * dim + (V,))
    boundary = conditions = None
    extra = None
    if bc == "states":
        b = _states(dim, V, family, 977, 2 * dim)
        boundary = {(a, s): b[2 * a + s] for a in range(dim) for s in range(2)}
        extra = b
    elif bc is not None:
        boundary = {k: (exa.Dirichlet(_states(dim, V, family, 978, 1)[0]) if v == "dirichlet" else v) for k, v in bc.items()}
        conditions = fv_faces(boundary, dim, n_real, n_aux, exa.PDE_EULER)[2]
        extra = _states(dim, V, family, 978, 1)
    lam = max(float(np.max(R.max_eigenvalue(np.concatenate([U.reshape(-1, V)] + ([extra] if extra is not None else [])), d, R.PDE_EULER))) for d in range(dim))
    h = K.H_VOLUME
    dt = K.CFL * h / (dim * lam)
    g = exa.FVPatchGrid(dim, grid, P, 2, n_real, n_aux, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, length=h * grid[0] * P, boundary=boundary, fused=False)
    assert abs(g.h - h) < 1e-15
    g.set_interior(U)
    g.step(dt)
    after = g.interior()
    ref = M.grid_update(U, dt, g.h, dim, n_real, R.PDE_EULER, boundary=boundary if conditions is None else None, conditions=conditions)
    worst = M.ratio(after, ref)
    print("%s %s: err / bound %.3f" % (case, family, worst))
    log_fv_measurement(what="grid %s %s" % (case, family), ratio=worst, scheme="muscl-hancock")
    assert worst <= 1.0, (case, family, worst)
    assert np.array_equal(after[..., n_real:], U[..., n_real:]), "auxiliary variables changed"
    if bc is None:                                                # periodic: the total of every evolved variable moves by rounding only
        for v in range(n_real):
            drift = abs(math.fsum(after[..., v].ravel()) - math.fsum(U[..., v].ravel()))
            bound = float(R.U53 * np.sum(ref.E[..., v]))
            print("  variable %d: total moves by %.3e, bound %.3e" % (v, drift, bound))
            assert drift <= bound, (v, drift, bound)


def _l1_wave(exa, npatch, mode, H, fused):
    N = npatch * 4
    G, rho = M.density_wave(N)
    g = exa.FVPatchGrid(2, (npatch, npatch), 4, H, 5, 0, exa.PDE_EULER, mode, length=1.0, fused=fused)
    g.set_interior(R.cut_patches(G, 2, (npatch, npatch), 4))
    steps = g.run(0.25, cfl=GOLDEN["cfl"])
    return float(np.mean(np.abs(R.assemble(g.interior(), 2)[..., 0] - rho(0.25)))), steps


def test_density_wave_run(exa):
    l1 = {}
    for npatch in (16, 32):
        l1[npatch], steps = _l1_wave(exa, npatch, exa.FV_MUSCL_HANCOCK, 2, False)
        want = GOLDEN["density_wave"]["muscl_%d" % (4 * npatch)]
        print("density wave %d^2 volumes: L1(rho) %.6e in %d steps (recorded %.6e in %d)" % (4 * npatch, l1[npatch], steps, want["l1"], want["steps"]))
        assert steps == want["steps"], (steps, want)
        assert abs(l1[npatch] / want["l1"] - 1) <= 1e-10, (l1[npatch], want)
    order = math.log2(l1[16] / l1[32])
    first, _ = _l1_wave(exa, 16, exa.FV_RUSANOV, 1, True)
    print("order %.3f (reference 1.81); 64^2: %.3e against the Rusanov mode's %.3e, ratio %.3f (reference 0.12)" % (order, l1[16], first, l1[16] / first))
    assert order >= 1.5, order
    assert l1[16] <= 0.25 * first, (l1[16], first)


def test_sod_between_walls(exa):
    from examples.sod_tube_fv_walls import initial_state, l1_density
    nx, P = 64, 4
    res = {}
    for name, mode, H, fused in (("muscl", exa.FV_MUSCL_HANCOCK, 2, False), ("rusanov", exa.FV_RUSANOV, 1, True)):
        g = exa.FVPatchGrid(2, (nx, 1), P, H, 5, 0, exa.PDE_EULER, mode, length=1.0, boundary={(0, 0): exa.Wall(), (0, 1): exa.Wall()}, fused=fused)
        g.set_interior(initial_state(nx, P))
        steps = g.run(0.1, cfl=GOLDEN["cfl"])
        u = g.interior()
        rho = u[..., 0]
        p = 0.4 * (u[..., 4] - 0.5 * (u[..., 1] ** 2 + u[..., 2] ** 2 + u[..., 3] ** 2) / rho)
        res[name] = (l1_density(rho, 0.1), float(rho.min()), float(p.min()), steps)
        print("Sod %s: L1(rho) %.6e, min rho %.6f, min p %.6f, %d steps" % ((name,) + res[name]))
    l1, rmin, pmin, steps = res["muscl"]
    assert rmin >= 0.125 - 1e-12 and pmin >= 0.1 - 1e-12, (rmin, pmin)
    assert l1 <= 0.5 * res["rusanov"][0], (l1, res["rusanov"][0])
    want = GOLDEN["sod"]["muscl"]
    assert steps == want["steps"] and abs(l1 / want["l1"] - 1) <= 1e-10, (steps, l1, want)


# ---- generated term sets ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _flagged(name):
    """the term set tests/user_term_sets.py defines under `name`, with the keyword"""
    from exahype_amd.pde_codegen import SympyPDE
    from tests import user_term_sets as T
    base = getattr(T, name)()
    sub = lambda e, qq: e.subs(dict(zip(base.q, qq)), simultaneous=True)     # noqa: E731
    return SympyPDE(base.n_vars, flux=lambda qq, d: [sub(e, qq) for e in base.flux_exprs[d]], max_eigenvalue=lambda qq, d: sub(base.eig_exprs[d], qq),
                    max_dim=base.max_dim, name=base.name + "_muscl", muscl_hancock=True)


@pytest.mark.parametrize("P", (4, 8))
def test_generated_shallow_water_against_the_restatement(exa, P):
    import torch
    from tests import fv_user_cases as KU
    spde = _flagged("swe")
    terms = R.UserTerms(spde)
    pid = spde.register()
    assert exa._lib.load().exa_pde_flags(pid) & 16
    n, H, n_aux = 7, 2, 1
    kern = exa.FVRusanovKernel(2, P, H, 3, n_aux, n, pid, exa.FV_MUSCL_HANCOCK)
    for family in ("benign", "riemann"):
        Q = KU.state(KU.SW, family, n, 2, P, H, 3 + n_aux, 500 + P)
        lam = float(np.max(np.abs(Q[..., 1:3] / Q[..., :1]) + np.sqrt(9.81 * Q[..., :1])))          # |u_n| + sqrt(g h)
        h = K.H_VOLUME
        dt = K.CFL * h / (2 * lam)
        ref = M.update(Q, dt, h, 2, P, H, 3, n_aux, terms=terms)
        qd = torch.as_tensor(Q).cuda()
        kern.time_step(qd, dt, h)
        got = qd.cpu().numpy()
        worst = M.ratio(got, ref, M.interior(2, P, H))
        print("generated shallow water P = %d %s: err / bound %.3f" % (P, family, worst))
        log_fv_measurement(what="user swe P%d %s" % (P, family), ratio=worst, scheme="muscl-hancock")
        assert worst <= 1.0, (P, family, worst)
        keep = np.ones(Q.shape[1:], dtype=bool)
        keep[M.interior(2, P, H)[1:] + (slice(0, 3),)] = False
        assert np.array_equal(got[:, keep], Q[:, keep])
        out = kern.time_step_oop(torch.as_tensor(Q).cuda(), dt, h).cpu().numpy()
        assert np.array_equal(out, got[M.interior(2, P, H)])


def test_generated_euler_against_the_builtin_kernel(exa):
    import torch
    spde = _flagged("euler_sympy")
    n, P, H = 5, 4, 2
    Q = K1.state("benign", n, 3, P, H, 5, 77)
    dt, h = K.cfl_step(Q, 3, R.PDE_EULER)
    res = []
    for pde in (exa.PDE_EULER, spde.register()):
        qd = torch.as_tensor(Q).cuda()
        exa.FVRusanovKernel(3, P, H, 5, 0, n, pde, exa.FV_MUSCL_HANCOCK).time_step(qd, dt, h)
        res.append(qd.cpu().numpy())
    err = float(np.max(np.abs(res[0] - res[1])) / np.max(np.abs(res[0])))
    print("generated Euler against the built-in kernel: %.3e of the largest magnitude" % err)
    assert err <= 1e-12, err
    assert not np.array_equal(res[0], Q)


def test_plan_on_a_term_set_without_the_keyword_is_refused(exa):
    from exahype_amd import _lib
    from tests import user_term_sets as T
    pid = T.swe().register()
    assert not (_lib.load().exa_pde_flags(pid) & 16)
    with pytest.raises(_lib.ExaHypeHipError, match="muscl_hancock=True"):
        exa.FVRusanovKernel(2, 4, 2, 3, 0, 1, pid, exa.FV_MUSCL_HANCOCK)


def test_hipprinter_scheme(exa):
    import torch
    from exahype_amd.KernelBuilder import KernelBuilder
    from exahype_amd.printers.HIPPrinter import HIPPrinter
    n, P, H = 6, 4, 2
    k = KernelBuilder(2, P, H, 5, 0, n)
    pr = HIPPrinter(k, scheme="fv-muscl-hancock", pde="euler")
    assert "fv_muscl_kernel<2>" in pr.code and "fv-muscl-hancock" in pr.code and "exa_fv_plan_create(dev, 2, 2, 4, 2, 5, 0, 6, 1" in pr.code
    with pytest.raises(ValueError, match="two halo layers"):
        HIPPrinter(KernelBuilder(2, P, 1, 5, 0, n), scheme="fv-muscl-hancock", pde="euler")
    Q = K1.state("benign", n, 2, P, H, 5, 78)
    dt, h = K.cfl_step(Q, 2, R.PDE_EULER)
    a = Q.copy()
    pr.run(a, dt, h=h)
    qd = torch.as_tensor(Q).cuda()
    exa.FVRusanovKernel(2, P, H, 5, 0, n, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK).time_step(qd, dt, h)
    assert np.array_equal(a, qd.cpu().numpy()) and not np.array_equal(a, Q)

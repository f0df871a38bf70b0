"""The MUSCL-Hancock kernels on term sets with a source and / or a non-conservative product (SympyPDE(muscl_hancock=True, muscl_terms=True)), on
the GPU, against the long-double restatement tests/fv_muscl_terms_ref.py (tests/test_fv_muscl_terms_reference.py shows on the CPU that a plain
fp64 evaluation stays inside its bound and that every mutant of a new term leaves it 100-fold).

  * every row of tests/fv_muscl_terms_cases.PATCH_ROWS times both families through its entries (in place, masked, out of place): evolved
    interior values within 2^-53 E; halo layers, auxiliary variables and masked-out patches bit-unchanged; out of place bit-equal to in place;
  * the GRID_ROWS: FUSED_EDGES bit-equal to fused=False, both inside the bound of grid_update on the assembled array, the returned lambda
    bit-equal to exa_fv_max_eigenvalue on the new states;
  * exa_pde_flags of the three sets; HIPPrinter(scheme="fv-muscl-hancock", pde=coupled_state) equals the plan call bit for bit;
  * FVPatchGrid.run on the advection-reaction wave reproduces the recorded fp64 runs (steps equal, L1 within 1e-10), flux form and ncp form;
  * Euler with gravity from rest: the midpoint rule is exact, momentum rho g t and energy p / (gamma - 1) + rho |g|^2 t^2 / 2 to 1e-13 --
    dt, not dt / h, scales the source;
  * SubcellLimiter(fv_mode=FV_MUSCL_HANCOCK) refuses such a set and names FV_RUSANOV.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import fv_reference as R
from tests import fv_muscl_terms_cases as K
from tests import fv_muscl_terms_ref as T
from tests.util import log_fv_measurement

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fv_muscl_terms_runs.json")))


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from exahype_amd import solvers
    return solvers


def _run(kern, entry, Q, dt, h, n):
    """one form of the call on the device -> (result as numpy, masked patches or None)"""
    import torch
    qd = torch.as_tensor(Q).cuda()
    if entry == "inplace":
        kern.time_step(qd, dt, h)
        return qd.cpu().numpy(), None
    if entry == "slot":
        slot = K.slot_of(n)
        kern.time_step(qd, dt, h, slot=torch.as_tensor(slot).cuda())
        return qd.cpu().numpy(), slot < 0
    out = kern.time_step_oop(qd, dt, h)
    assert np.array_equal(qd.cpu().numpy(), Q), "time_step_oop wrote its input"
    return out.cpu().numpy(), None


@pytest.mark.parametrize("row", K.PATCH_ROWS, ids=K.patch_id)
def test_patch_update_within_bound(exa, row):
    name, dim, P, H, n_aux, n, entries = row
    m, tm = K.n_real(name), K.terms(name)
    kern = exa.FVRusanovKernel(dim, P, H, m, n_aux, n, K.flagged(name).register(), exa.FV_MUSCL_HANCOCK)
    sel = T.interior(dim, P, H)
    for family in K.FAMILIES:
        Q = K.patch_state(row, family)
        dt, h = K.cfl_step(name, dim, Q.reshape(-1, Q.shape[-1]))
        ref = T.update(Q, dt, h, dim, P, H, m, n_aux, terms=tm)           # one reference, shared by the row's entries
        keep = np.ones(Q.shape[1:], dtype=bool)
        keep[sel[1:] + (slice(0, m),)] = False                            # halo entries and auxiliary variables
        results = {}
        for entry in entries:
            what = "%s %s %s" % (K.patch_id(row), family, entry)
            got, masked = _run(kern, entry, Q, dt, h, n)
            results[entry] = got
            gi = got[sel] if entry != "oop" else got.reshape(Q[sel].shape)
            live = np.ones(n, dtype=bool) if masked is None else ~masked
            assert live.any() and (masked is None or masked.any())
            err = np.abs(gi[..., :m].astype(R.LD) - ref.new[sel][..., :m])
            worst = float(np.max((err / (R.U53 * ref.E))[live]))
            print("%s: err / bound %.3f" % (what, worst))
            log_fv_measurement(what=what, row=K.patch_id(row), family=family, entry=entry, ratio=worst, scheme="muscl-hancock-terms")
            assert worst <= 1.0, (what, worst)
            assert not np.array_equal(gi[live][..., :m], Q[sel][live][..., :m])
            assert np.array_equal(gi[..., m:], Q[sel][..., m:]), what + ": auxiliary variables changed"
            if entry != "oop":
                assert np.array_equal(got[:, keep], Q[:, keep]), what + ": halo or auxiliary values changed"
                assert np.array_equal(got[~live], Q[~live]), what + ": a masked patch was written"
        if "oop" in results and "inplace" in results:
            assert np.array_equal(results["oop"].reshape(Q[sel].shape), results["inplace"][sel]), "out of place differs from in place"
        if "slot" in results and "inplace" in results:
            live = K.slot_of(n) >= 0
            assert np.array_equal(results["slot"][live], results["inplace"][live]), "the masked call differs on the patches in use"


def _grid(exa, row, s, fused):
    name, dim, P, n_aux, grid, _, _ = row
    g = exa.FVPatchGrid(dim, grid, P, 2, K.n_real(name), n_aux, K.flagged(name).register(), exa.FV_MUSCL_HANCOCK, length=s.h * grid[0] * P,
                        boundary=s.boundary, fused=fused)
    assert abs(g.h - s.h) < 1e-15
    return g


@pytest.mark.parametrize("row", K.GRID_ROWS, ids=K.grid_id)
def test_grid_step_within_bound(exa, row):
    import torch
    name, dim, P, n_aux, grid, faces, forms = row
    m, tm = K.n_real(name), K.terms(name)
    for family in K.FAMILIES:
        s = K.grid_setup(row, family)
        g = _grid(exa, row, s, exa.FUSED_EDGES)
        g.set_interior(s.U)
        g.step(s.dt)
        after = g.interior()
        ref = T.grid_update(s.U, s.dt, g.h, dim, m, terms=tm, conditions=s.conditions)
        worst = T.ratio(after, ref)
        print("%s %s: err / bound %.3f" % (K.grid_id(row), family, worst))
        log_fv_measurement(what="grid one launch %s %s" % (K.grid_id(row), family), ratio=worst, scheme="muscl-hancock-terms")
        assert worst <= 1.0, (K.grid_id(row), family, worst)
        assert np.array_equal(after[..., m:], s.U[..., m:]), "auxiliary variables changed"
        assert not np.array_equal(after[..., :m], s.U[..., :m])
        two = _grid(exa, row, s, False)
        two.set_interior(s.U)
        two.step(s.dt)
        assert np.array_equal(after, two.interior()), "the one-launch step and the two-pass form differ"
        if "two-pass" in forms:                                       # ... the two-pass form held to the bound in its own right
            w2 = T.ratio(two.interior(), ref)
            print("%s %s, two passes: err / bound %.3f" % (K.grid_id(row), family, w2))
            assert w2 <= 1.0, (K.grid_id(row), family, w2)
        # the CFL scan: the entry itself on the same input, its lambda against a scan of the array it wrote
        lib, plan = g.lib, g.kernel._plan
        q, out = torch.as_tensor(s.U).cuda().contiguous(), torch.full(s.U.shape, float("nan"), dtype=torch.float64, device="cuda")
        lam, scan = torch.full((1,), -1.0, dtype=torch.float64, device="cuda"), torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
        data = C.c_void_p(g._bstate.data_ptr()) if g._bstate is not None else None
        exa.check(lib.exa_fv_grid_step_muscl_device(plan, C.c_void_p(q.data_ptr()), C.c_void_p(out.data_ptr()), g._grid_arr, g._kinds, data, s.dt, g.h,
                                                    C.c_void_p(lam.data_ptr()), None))
        exa.check(lib.exa_fv_max_eigenvalue(plan, C.c_void_p(out.data_ptr()), 1, None, 0.0, g.h, C.c_void_p(scan.data_ptr()), None))
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), after) and np.array_equal(q.cpu().numpy(), s.U)
        lam, scan = float(lam[0]), float(scan[0])
        print("  lambda of the new states %.17g (scan %.17g)" % (lam, scan))
        assert lam > 0.0 and np.float64(lam).tobytes() == np.float64(scan).tobytes(), (lam, scan)


def test_flags_of_the_three_sets(exa):
    lib = exa._lib.load()
    for name in K.SETS:
        flags = lib.exa_pde_flags(K.flagged(name).register())
        assert flags & exa._lib.PDE_FLAG_MUSCL_HANCOCK == 16 and flags & exa._lib.PDE_FLAG_MUSCL_TERMS == 32, (name, flags)
        assert bool(flags & exa._lib.PDE_FLAG_NCP) == K.terms(name).has_ncp and not flags & exa._lib.PDE_FLAG_XT, (name, flags)


def test_hipprinter_scheme_on_a_set_with_terms(exa):
    import torch
    from exahype_amd.KernelBuilder import KernelBuilder
    from exahype_amd.printers.HIPPrinter import HIPPrinter
    row = K.PATCH_ROWS[5]
    name, dim, P, H, n_aux, n, _ = row
    assert name == K.CS
    pr = HIPPrinter(KernelBuilder(dim, P, H, 3, n_aux, n), scheme="fv-muscl-hancock", pde=K.flagged(name))
    assert "fv_muscl_kernel<2>" in pr.code and "muscl_terms=True" in pr.code
    Q = K.patch_state(row, "benign")
    dt, h = K.cfl_step(name, dim, Q.reshape(-1, Q.shape[-1]))
    a = Q.copy()
    pr.run(a, dt, h=h)
    qd = torch.as_tensor(Q).cuda()
    exa.FVRusanovKernel(dim, P, H, 3, n_aux, n, K.flagged(name).register(), exa.FV_MUSCL_HANCOCK).time_step(qd, dt, h)
    assert np.array_equal(a, qd.cpu().numpy()) and not np.array_equal(a, Q)


@pytest.mark.parametrize("form", ("flux", "ncp"))
def test_advection_reaction_run(exa, form):
    from examples import advection_reaction_fv_second_order as X
    for npatch in (16, 32):
        r = X.run(form, True, npatch, 4, X.T_END, GOLDEN["cfl"])
        want = GOLDEN[form]["muscl_%d" % (4 * npatch)]
        print("%s form, %d^2 volumes: L1 %.6e in %d steps (recorded %.6e in %d)" % (form, 4 * npatch, r["l1"], r["steps"], want["l1"], want["steps"]))
        assert r["steps"] == want["steps"], (r, want)
        assert abs(r["l1"] / want["l1"] - 1) <= 1e-10, (r, want)


def test_euler_with_gravity_from_rest(exa):
    """uniform rho = 1, p = 1 at rest on a periodic 2 x 2 grid: the fluxes cancel, the source acts alone, and the midpoint rule integrates it
    exactly -- m = rho g t, E = p / (gamma - 1) + rho |g|^2 t^2 / 2.  With dt / h in place of dt the momentum would be 8 times as large."""
    g3 = np.array([0.3, -0.5, 0.8])                                 # tests/user_term_sets.euler_gravity's default
    P, dt, nsteps = 4, 0.01, 5
    for fused in (exa.FUSED_EDGES, False):
        g = exa.FVPatchGrid(2, (2, 2), P, 2, 5, 0, K.flagged(K.EG).register(), exa.FV_MUSCL_HANCOCK, length=1.0, fused=fused)
        assert abs(g.h - 0.125) < 1e-15
        U = np.zeros((2, 2, P, P, 5))
        U[..., 0], U[..., 4] = 1.0, 1.0 / 0.4
        g.set_interior(U)
        for _ in range(nsteps):
            g.step(dt)
        u, t = g.interior(), nsteps * dt
        p = 0.4 * (u[..., 4] - 0.5 * (u[..., 1] ** 2 + u[..., 2] ** 2 + u[..., 3] ** 2) / u[..., 0])
        assert np.all(u[..., 0] == 1.0), "the density moved"
        assert np.max(np.abs(p - 1.0)) <= 1e-13 and np.max(p) - np.min(p) <= 1e-13, (p.min(), p.max())
        for a in range(3):
            assert np.max(np.abs(u[..., 1 + a] / (g3[a] * t) - 1)) <= 1e-13, (a, u[0, 0, 0, 0, 1 + a], g3[a] * t)
        E = 1.0 / 0.4 + 0.5 * float(g3 @ g3) * t * t
        assert np.max(np.abs(u[..., 4] / E - 1)) <= 1e-13, (u[0, 0, 0, 0, 4], E)


def test_limiter_refuses_the_second_order_mode_on_such_a_set(exa):
    s = exa.AderDgSolver(2, 3, (2, 2), pde=K.flagged(K.EG).register(), n_vars=5)
    with pytest.raises(ValueError, match="FV_RUSANOV") as e:
        exa.SubcellLimiter(s, capacity=4, fv_mode=exa.FV_MUSCL_HANCOCK)
    assert "muscl_terms" in str(e.value)
    with pytest.raises(ValueError, match="FV_RUSANOV"):               # (an ncp is refused as it always was)
        exa.SubcellLimiter(exa.AderDgSolver(2, 3, (2, 2), pde=K.flagged(K.TL).register(), n_vars=2), capacity=4, fv_mode=exa.FV_MUSCL_HANCOCK)

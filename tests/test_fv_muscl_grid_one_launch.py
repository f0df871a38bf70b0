"""The one-launch MUSCL-Hancock grid step on halo-less arrays (exa_fv_grid_step_muscl_device; FVPatchGrid(fused=FUSED_EDGES)) on the GPU.

One step of every case of tests/fv_muscl_grid_cases.py, families `benign` and `riemann`, must
  - equal the long-double restatement (tests/fv_muscl_ref.py) applied to the ASSEMBLED global array within 2^-53 E in every volume: the kernel
    gathers the window of a patch itself, so they agree only if every entry the stencil reads, the EDGE entries among them, came from the right
    (diagonal) patch or boundary rule (tests/test_fv_muscl_grid_one_launch_host.py shows that every case sees its edge entries);
  - equal one step of the two-pass form (fused=False) bit for bit: the same device functions, no contraction;
  - leave the auxiliary variables as they were, and (periodic) conserve every evolved variable to the rounding of its own updates;
  - return the CFL scan of the new states bit for bit as exa_fv_max_eigenvalue gives it.
The runs are the recorded ones of tests/golden/fv_muscl_runs.json, by the two-pass form's own criterion.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from oracle import fv_reference as R
from tests import fv_muscl_grid_cases as G
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


def _pde_id(exa, s):
    if s.terms_name == "swe":
        return G.flagged("swe").register()
    return exa.PDE_ADVECTION if s.terms_name == "adv" else exa.PDE_EULER


def _grid(exa, s, fused, pde=None):
    g = exa.FVPatchGrid(s.dim, s.grid, s.P, 2, s.n_real, s.n_aux, _pde_id(exa, s) if pde is None else pde, exa.FV_MUSCL_HANCOCK,
                        length=s.h * s.grid[0] * s.P, boundary=s.boundary, fused=fused)
    assert abs(g.h - s.h) < 1e-15
    return g


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("case", G.GPU_CASES)
def test_one_launch_step(exa, case, family):
    _one_step(exa, case, family)


@pytest.mark.parametrize("case", G.BLIND_TO_ITS_CORNERS)
def test_all_faces_prescribed_form(exa, case):
    """boundary = one state per face, all 2 dim faces named: FVPatchGrid hands every kind as EXA_FV_FACE_STATE.  (The restatement cannot see the
    edge entries at this domain's corners -- tests/fv_muscl_grid_cases.py -- the bit equality with the two-pass form can.)"""
    _one_step(exa, case, "benign")


def _one_step(exa, case, family):
    import torch
    s = G.setup(case, family)
    pde = _pde_id(exa, s)
    g = _grid(exa, s, exa.FUSED_EDGES, pde)
    assert g.fused and g.fused_edges and tuple(g.U.shape) == s.U.shape
    g.set_interior(s.U)
    g.step(s.dt)
    after = g.interior()
    ref = G.reference(s, g.h)
    worst = M.ratio(after, ref)
    print("%s %s: err / bound %.3f" % (case, family, worst))
    log_fv_measurement(what="grid one launch %s %s" % (case, family), ratio=worst, scheme="muscl-hancock")
    assert worst <= 1.0, (case, family, worst)
    two = _grid(exa, s, False, pde)
    two.set_interior(s.U)
    two.step(s.dt)
    assert np.array_equal(after, two.interior()), "the one-launch step and the two-pass form differ"
    assert np.array_equal(after[..., s.n_real:], s.U[..., s.n_real:]), "auxiliary variables changed"
    assert not np.array_equal(after[..., :s.n_real], s.U[..., :s.n_real])
    if s.periodic:                                                # the total of every evolved variable moves by rounding only
        for v in range(s.n_real):
            drift = abs(math.fsum(after[..., v].ravel()) - math.fsum(s.U[..., v].ravel()))
            bound = float(R.U53 * np.sum(ref.E[..., v]))
            print("  variable %d: total moves by %.3e, bound %.3e" % (v, drift, bound))
            assert drift <= bound, (v, drift, bound)
    # the CFL scan: the entry itself on the same input, its lambda against a scan of the array it wrote
    lib, plan = g.lib, g.kernel._plan
    q, out = torch.as_tensor(s.U).cuda().contiguous(), torch.full(s.U.shape, float("nan"), dtype=torch.float64, device="cuda")
    lam, scan = torch.full((1,), -1.0, dtype=torch.float64, device="cuda"), torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    kinds = g._kinds if g._kinds is not None else ((C.c_int * (2 * s.dim))(*[1] * (2 * s.dim)) if g._bstate is not None else None)
    data = C.c_void_p(g._bstate.data_ptr()) if g._bstate is not None else None
    exa.check(lib.exa_fv_grid_step_muscl_device(plan, C.c_void_p(q.data_ptr()), C.c_void_p(out.data_ptr()), g._grid_arr, kinds, data, s.dt, g.h,
                                                C.c_void_p(lam.data_ptr()), None))
    exa.check(lib.exa_fv_max_eigenvalue(plan, C.c_void_p(out.data_ptr()), 1, None, 0.0, g.h, C.c_void_p(scan.data_ptr()), None))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), after) and np.array_equal(q.cpu().numpy(), s.U)
    lam, scan = float(lam[0]), float(scan[0])
    print("  lambda of the new states %.17g (scan %.17g)" % (lam, scan))
    assert lam > 0.0 and np.float64(lam).tobytes() == np.float64(scan).tobytes(), (lam, scan)
    fresh = _grid(exa, s, False, pde)
    fresh.set_interior(after)
    assert g._lam_valid and g.max_eigenvalue() == fresh.max_eigenvalue()
    assert g.max_eigenvalue() == (max(lam, g._lam_boundary) if g._lam_boundary is not None else lam)


def test_three_steps_stay_bit_equal_to_the_two_pass_form(exa):
    s = G.setup("2d-P4-6x7-periodic", "benign")
    a, b = _grid(exa, s, exa.FUSED_EDGES), _grid(exa, s, False)
    a.set_interior(s.U)
    b.set_interior(s.U)
    for k in range(3):
        a.step(s.dt)
        b.step(s.dt)
        assert np.array_equal(a.interior(), b.interior()), k
        assert a.max_eigenvalue() == b.max_eigenvalue(), k
    assert abs(a.time - 3 * s.dt) < 1e-15 and not np.array_equal(a.interior(), s.U)
    assert np.array_equal(a.with_halo().cpu().numpy(), b.with_halo().cpu().numpy())


def _l1_wave(exa, npatch):
    G0, rho = M.density_wave(npatch * 4)
    g = exa.FVPatchGrid(2, (npatch, npatch), 4, 2, 5, 0, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, length=1.0, fused=exa.FUSED_EDGES)
    g.set_interior(R.cut_patches(G0, 2, (npatch, npatch), 4))
    steps = g.run(0.25, cfl=GOLDEN["cfl"])
    return float(np.mean(np.abs(R.assemble(g.interior(), 2)[..., 0] - rho(0.25)))), steps


def test_density_wave_run(exa):
    for npatch in (16, 32):
        l1, steps = _l1_wave(exa, npatch)
        want = GOLDEN["density_wave"]["muscl_%d" % (4 * npatch)]
        print("density wave %d^2 volumes: L1(rho) %.6e in %d steps (recorded %.6e in %d)" % (4 * npatch, l1, steps, want["l1"], want["steps"]))
        assert steps == want["steps"], (steps, want)
        assert abs(l1 / want["l1"] - 1) <= 1e-10, (l1, want)


def test_sod_between_walls(exa):
    from examples.sod_tube_fv_walls import initial_state, l1_density
    nx, P = 64, 4
    g = exa.FVPatchGrid(2, (nx, 1), P, 2, 5, 0, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, length=1.0, boundary={(0, 0): exa.Wall(), (0, 1): exa.Wall()},
                        fused=exa.FUSED_EDGES)
    g.set_interior(initial_state(nx, P))
    steps = g.run(0.1, cfl=GOLDEN["cfl"])
    l1 = l1_density(g.interior()[..., 0], 0.1)
    want = GOLDEN["sod"]["muscl"]
    print("Sod through the one-launch step: L1(rho) %.6e in %d steps (recorded %.6e in %d)" % (l1, steps, want["l1"], want["steps"]))
    assert steps == want["steps"] and abs(l1 / want["l1"] - 1) <= 1e-10, (steps, l1, want)


def test_refusals_on_the_device(exa):
    """every call returns an error code before anything is launched"""
    import torch
    from exahype_amd import _lib
    lib = _lib.load()
    grid = _lib.larr([2, 2])

    def call(kern, q, out, grid=grid, kinds=None, data=None, h=0.1):
        return lib.exa_fv_grid_step_muscl_device(kern._plan, C.c_void_p(q.data_ptr()), C.c_void_p(out.data_ptr()), grid, kinds, data, 1e-3, h, None, None)

    def refused(rc, *words):
        msg = lib.exa_last_error().decode()
        assert rc == -1 and all(w in msg for w in words), (rc, msg)
    q, out = torch.ones(4 * 16 * 5, dtype=torch.float64, device="cuda"), torch.zeros(4 * 16 * 5, dtype=torch.float64, device="cuda")
    one = exa.FVRusanovKernel(2, 1, 2, 5, 0, 4, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK)
    refused(call(one, q, out), "patch_size", "exa_fv_time_step_device")
    with pytest.raises(ValueError, match="patch_size"):
        exa.FVPatchGrid(2, (2, 2), 1, 2, 5, 0, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, fused=exa.FUSED_EDGES)
    refused(call(exa.FVRusanovKernel(2, 4, 2, 5, 0, 4, exa.PDE_EULER, exa.FV_RUSANOV), q, out), "EXA_FV_MUSCL_HANCOCK", "exa_fv_grid_step_device")
    kern = exa.FVRusanovKernel(2, 4, 2, 5, 0, 4, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK)
    refused(call(kern, q, q), "array of their own")
    refused(call(kern, q, out, grid=_lib.larr([2, 3])), "6 patches", "plan 4")
    refused(call(kern, q, out, kinds=(C.c_int * 4)(0, 3, 0, 0)), "face_kind[1]")
    refused(call(kern, q, out, kinds=(C.c_int * 4)(0, 1, 0, 0)), "face_data_dev")
    refused(call(kern, q, out, h=0.0), "h > 0")
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(q.min()) == 1.0                 # nothing ran
    with pytest.raises(ValueError, match="Dirichlet"):
        exa.FVPatchGrid(2, (2, 2), 4, 2, 5, 0, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, boundary={(0, 0): exa.Dirichlet(lambda x, t: x)}, fused=exa.FUSED_EDGES)
    with pytest.raises(ValueError, match="FV_MUSCL_HANCOCK"):
        exa.FVPatchGrid(2, (2, 2), 4, 1, 5, 0, exa.PDE_EULER, exa.FV_RUSANOV, fused=exa.FUSED_EDGES)
    with pytest.raises(ValueError, match="fused=False") as e:                       # the default stays a refusal, and names both ways out
        exa.FVPatchGrid(2, (2, 2), 4, 2, 5, 0, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK)
    assert "FUSED_EDGES" in str(e.value)

"""The plane-streaming MUSCL-Hancock kernel (fv_muscl_stream_kernel, exahype_amd/csrc/exa_fv_muscl.hpp; FVRusanovKernel(stream_planes=...)) on the GPU,
for the tables of tests/fv_muscl_stream_cases.py.

  1. FV_STREAM_ALWAYS against the resident kernel wherever both serve a shape: every double of the array bit-equal -- halos and auxiliary
     variables included -- through the three entries (in place, with a slot array, out of place), with 1 and 5 patches, and a second launch
     bit-equal to the first.  The two kernels call the same per-volume device functions on the same operands; only where the axis-0 neighbours
     stand differs.
  2. the shapes only streaming serves: every evolved variable of every interior volume within 2^-53 E of the long-double restatement
     (tests/fv_muscl_ref.py; tests/test_fv_muscl_stream_reference.py shows on the CPU that a plain fp64 evaluation stays inside it on these rows),
     halo, auxiliary and masked values bit-equal to the input, out of place bit-equal to in place, and NaN in every entry outside the stencil
     invisible.
  3. plan selection: FV_STREAM_IF_NEEDED is the resident plan at P = 8 and the streamed one at P = 10; a streamed plan is refused by
     exa_fv_grid_step_muscl_device and by FVPatchGrid(fused=FUSED_EDGES).
  4. one step of the two-pass grid form with streamed patches against the restatement on the assembled array.
  5. generated term sets: forced streaming bit-equal to the set's own resident kernel; generated Euler at P = 10 against the built-in streamed
     result; Euler with gravity (muscl_terms=True) at P = 10 within the bound of tests/fv_muscl_terms_ref.py.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import fv_reference as R
from tests import fv_cases as K1
from tests import fv_muscl_cases as K
from tests import fv_muscl_ref as M
from tests import fv_muscl_stream_cases as KS
from tests.util import log_fv_measurement

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from exahype_amd import solvers
    return solvers


def _pde(exa, pde):
    return exa.PDE_EULER if pde == R.PDE_EULER else exa.PDE_ADVECTION


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _run(kern, entry, Q, dt, h, n):
    """one form of the call on the device -> (result as numpy, masked patches or None)"""
    import torch
    qd = torch.as_tensor(Q).cuda()
    if entry == "inplace":
        kern.time_step(qd, dt, h)
        return qd.cpu().numpy(), None
    if entry == "slot":
        slot = K1.slot_of(n)
        kern.time_step(qd, dt, h, slot=torch.as_tensor(slot).cuda())
        return qd.cpu().numpy(), slot < 0
    out = kern.time_step_oop(qd, dt, h)
    assert np.array_equal(_bits(qd.cpu().numpy()), _bits(Q)), "time_step_oop wrote its input"
    return out.cpu().numpy(), None


# ---- 1. forced streaming against the resident kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", KS.EQUAL_SHAPES, ids=KS.shape_id)
def test_streamed_equals_resident_bit_for_bit(exa, shape):
    P, H, n_real, n_aux, pde = shape
    for n in KS.EQUAL_COUNTS:
        row = KS.equal_row(shape, n)
        resident = exa.FVRusanovKernel(3, P, H, n_real, n_aux, n, _pde(exa, pde), exa.FV_MUSCL_HANCOCK)
        streamed = exa.FVRusanovKernel(3, P, H, n_real, n_aux, n, _pde(exa, pde), exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_ALWAYS)
        assert streamed.streamed and not resident.streamed
        for family in K.families(row):
            Q = K.row_state(row, family)
            dt, h = K.cfl_step(Q, 3, pde)
            for entry in KS.ENTRIES:
                what = "%s n = %d %s %s" % (KS.shape_id(shape), n, family, entry)
                want, _ = _run(resident, entry, Q, dt, h, n)
                got, masked = _run(streamed, entry, Q, dt, h, n)
                assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), what + ": the streamed kernel differs from the resident one"
                if entry == "inplace":
                    assert not np.array_equal(got, Q), what + ": nothing was updated"
                again, _ = _run(streamed, entry, Q, dt, h, n)
                assert np.array_equal(_bits(again), _bits(got)), what + ": a second launch differs"


# ---- 2. the shapes only streaming serves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", KS.STREAM_ROWS, ids=K.row_id)
def test_streamed_patch_update_within_bound(exa, row):
    dim, P, H, n_real, n_aux, n, pde, _ = row
    kern = exa.FVRusanovKernel(dim, P, H, n_real, n_aux, n, _pde(exa, pde), exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_IF_NEEDED)
    assert kern.streamed
    sel = M.interior(dim, P, H)
    outside = M.outside_stencil(dim, P, H)
    for family in K.families(row):
        Q = K.row_state(row, family)
        dt, h = K.cfl_step(Q, dim, pde)
        ref = M.update(Q, dt, h, dim, P, H, n_real, n_aux, pde)              # one reference, shared by the three forms
        keep = np.ones(Q.shape[1:], dtype=bool)
        keep[sel[1:] + (slice(0, n_real),)] = False                          # halo entries and auxiliary variables
        results = {}
        for entry in KS.ENTRIES:
            what = "%s %s %s" % (K.row_id(row), family, entry)
            got, masked = _run(kern, entry, Q, dt, h, n)
            results[entry] = got
            gi = got[sel] if entry != "oop" else got.reshape(Q[sel].shape)
            live = np.ones(n, dtype=bool) if masked is None else ~masked
            assert live.any() and (masked is None or masked.any())
            err = np.abs(gi[..., :n_real].astype(R.LD) - ref.new[sel][..., :n_real])
            worst = float(np.max((err / (R.U53 * ref.E))[live]))
            print("%s: err / bound %.3f" % (what, worst))
            log_fv_measurement(what=what, row=K.row_id(row), family=family, entry=entry, ratio=worst, scheme="muscl-hancock-streamed")
            assert worst <= 1.0, (what, worst)
            assert not np.array_equal(gi[live][..., :n_real], Q[sel][live][..., :n_real]), what + ": nothing was updated"
            assert np.array_equal(_bits(gi[..., n_real:]), _bits(Q[sel][..., n_real:])), what + ": auxiliary variables changed"
            if entry != "oop":
                assert np.array_equal(_bits(got[:, keep]), _bits(Q[:, keep])), what + ": halo or auxiliary values changed"
                assert np.array_equal(_bits(got[~live]), _bits(Q[~live])), what + ": a masked patch was written"
        assert np.array_equal(_bits(results["oop"].reshape(Q[sel].shape)), _bits(results["inplace"][sel])), "out of place differs from in place"
        live = K1.slot_of(n) >= 0
        assert np.array_equal(_bits(results["slot"][live]), _bits(results["inplace"][live])), "the masked call differs on the patches in use"
        again, _ = _run(kern, "inplace", Q, dt, h, n)
        assert np.array_equal(_bits(again), _bits(results["inplace"])), "a second launch differs"
        # nothing outside the stencil is read
        Qn = Q.copy()
        Qn[:, outside] = np.nan
        got_nan, _ = _run(kern, "inplace", Qn, dt, h, n)
        assert np.array_equal(_bits(got_nan[sel]), _bits(results["inplace"][sel])), "an entry outside the stencil was read"
        out_nan, _ = _run(kern, "oop", Qn, dt, h, n)
        assert np.array_equal(_bits(out_nan), _bits(results["oop"])), "an entry outside the stencil was read (out of place)"


def test_negative_control_on_a_streamed_shape(exa):
    """the measure sees a 1e-9 error on the streamed kernel: run with h (1 + 2^-30) it leaves the bound"""
    row = KS.STREAM_ROWS[0]
    dim, P, H, n_real, n_aux, n, pde, _ = row
    Q = K.row_state(row, "supersonic")
    dt, h = K.cfl_step(Q, dim, pde)
    kern = exa.FVRusanovKernel(dim, P, H, n_real, n_aux, n, _pde(exa, pde), exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_IF_NEEDED)
    got, _ = _run(kern, "inplace", Q, dt, h * (1 + 2.0 ** -30), n)
    worst = M.ratio(got, M.update(Q, dt, h, dim, P, H, n_real, n_aux, pde), M.interior(dim, P, H))
    print("negative control: err / bound %.3g" % worst)
    assert worst > 1.0, worst


def test_host_entry_and_coordinates_on_a_streamed_plan(exa):
    """exa_fv_time_step_host, _device_at and _device_masked_at serve a streamed plan: the same bits as the plain device call"""
    import torch
    row = KS.STREAM_ROWS[0]
    dim, P, H, n_real, n_aux, n, pde, _ = row
    Q = K.row_state(row, "benign")
    dt, h = K.cfl_step(Q, dim, pde)
    kern = exa.FVRusanovKernel(dim, P, H, n_real, n_aux, n, _pde(exa, pde), exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_IF_NEEDED)
    want, _ = _run(kern, "inplace", Q, dt, h, n)
    host = Q.copy()
    kern.time_step(host, dt, h)
    assert np.array_equal(_bits(host), _bits(want))
    cen = torch.rand(n, dim, dtype=torch.float64, device="cuda")
    qd = torch.as_tensor(Q).cuda()
    kern.time_step(qd, dt, h, t=0.7, centres=cen)
    assert np.array_equal(_bits(qd.cpu().numpy()), _bits(want))
    slot = K1.slot_of(n)
    qd = torch.as_tensor(Q).cuda()
    kern.time_step(qd, dt, h, slot=torch.as_tensor(slot).cuda(), t=0.7, centres=cen)
    res = qd.cpu().numpy()
    assert np.array_equal(_bits(res[slot >= 0]), _bits(want[slot >= 0])) and np.array_equal(_bits(res[slot < 0]), _bits(Q[slot < 0]))
    # exa_fv_max_eigenvalue is unaffected by the form of the plan
    lam = torch.zeros(1, dtype=torch.float64, device="cuda")
    qd = torch.as_tensor(Q).cuda()
    exa.check(kern.lib.exa_fv_max_eigenvalue(kern._plan, C.c_void_p(qd.data_ptr()), 0, None, 0.0, h, C.c_void_p(lam.data_ptr()), None))
    sel = M.interior(dim, P, H)
    want_lam = max(float(np.max(R.max_eigenvalue(Q[sel], d, pde))) for d in range(dim))
    assert abs(float(lam[0]) / want_lam - 1) < 1e-14, (float(lam[0]), want_lam)


# ---- 3. plan selection ------------------------------------------------------------------------------------------------------------------
def test_plan_selection_and_grid_step_refusals(exa):
    import torch
    from exahype_amd import _lib
    mk = lambda P, sp, n=1: exa.FVRusanovKernel(3, P, 2, 5, 0, n, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, stream_planes=sp)     # noqa: E731
    assert not mk(8, exa.FV_STREAM_IF_NEEDED).streamed and mk(10, exa.FV_STREAM_IF_NEEDED).streamed
    assert mk(8, exa.FV_STREAM_ALWAYS).streamed and not mk(8, exa.FV_STREAM_NEVER).streamed
    assert not exa.FVRusanovKernel(2, 8, 2, 5, 0, 1, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_IF_NEEDED).streamed
    with pytest.raises(_lib.ExaHypeHipError, match=r"178880.*163840"):               # the default refuses P = 10 as it did
        mk(10, exa.FV_STREAM_NEVER)
    with pytest.raises(_lib.ExaHypeHipError, match="173280"):
        mk(20, exa.FV_STREAM_IF_NEEDED)
    # the one-launch grid step refuses a streamed plan and names the two-pass form
    kern = mk(4, exa.FV_STREAM_ALWAYS, 4)
    U = torch.zeros(2, 1, 2, 4, 4, 4, 5, dtype=torch.float64, device="cuda")
    U[..., 0], U[..., 4] = 1.0, 2.5
    U2 = torch.full_like(U, 7.0)
    lam = torch.zeros(1, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
    rc = kern.lib.exa_fv_grid_step_muscl_device(kern._plan, p(U), p(U2), _lib.larr([2, 1, 2]), None, None, 1e-3, 0.1, p(lam), None)
    msg = kern.lib.exa_last_error().decode()
    assert rc == -1 and "plane by plane" in msg and "two-pass" in msg and "exa_fv_time_step_device" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((U2 == 7.0).all())
    with pytest.raises(ValueError, match="fused=False"):
        exa.FVPatchGrid(3, (2, 1, 2), 10, 2, 5, 0, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, fused=exa.FUSED_EDGES, stream_planes=exa.FV_STREAM_IF_NEEDED)
    with pytest.raises(ValueError, match="fused=False"):
        exa.FVPatchGrid(3, (2, 1, 2), 4, 2, 5, 0, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, fused=exa.FUSED_EDGES, stream_planes=exa.FV_STREAM_ALWAYS)
    # ... while IF_NEEDED on a shape with a resident plan keeps the one-launch step
    g = exa.FVPatchGrid(3, (2, 1, 2), 4, 2, 5, 0, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, fused=exa.FUSED_EDGES, stream_planes=exa.FV_STREAM_IF_NEEDED)
    assert not g.kernel.streamed
    # a mode other than FV_MUSCL_HANCOCK takes no stream_planes
    with pytest.raises(_lib.ExaHypeHipError, match="stream_planes"):
        exa.FVRusanovKernel(3, 4, 1, 5, 0, 1, exa.PDE_EULER, exa.FV_RUSANOV, stream_planes=exa.FV_STREAM_IF_NEEDED)


# ---- 4. the two-pass grid step with streamed patches ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("benign", "riemann"))
def test_two_pass_grid_step_with_streamed_patches(exa, family):
    dim, grid, P, n_real = 3, (2, 1, 2), 10, 5
    n = int(np.prod(grid))
    U = K1.state(family, n, dim, P, 0, n_real, 47).reshape(grid + (P,) * dim + (n_real,))
    lam = max(float(np.max(R.max_eigenvalue(U.reshape(-1, n_real), d, R.PDE_EULER))) for d in range(dim))
    h = K.H_VOLUME
    dt = K.CFL * h / (dim * lam)
    g = exa.FVPatchGrid(dim, grid, P, halo_size=2, mode=exa.FV_MUSCL_HANCOCK, length=h * grid[0] * P, fused=False,
                        stream_planes=exa.FV_STREAM_IF_NEEDED)
    assert g.kernel.streamed and abs(g.h - h) < 1e-15
    g.set_interior(U)
    g.step(dt)
    after = g.interior()
    ref = M.grid_update(U, dt, g.h, dim, n_real, R.PDE_EULER)
    worst = M.ratio(after, ref)
    print("two-pass grid step, streamed patches, %s: err / bound %.3f" % (family, worst))
    log_fv_measurement(what="grid streamed %s" % family, ratio=worst, scheme="muscl-hancock-streamed")
    assert worst <= 1.0, (family, worst)
    assert not np.array_equal(after, U)


# ---- 5. generated term sets -------------------------------------------------------------------------------------------------------------
def test_generated_sets_forced_streaming_equals_their_resident_kernel(exa):
    from tests import fv_muscl_terms_cases as KT
    from tests.test_fv_muscl_grid import _flagged
    n, P, H = 3, 4, 2
    for name, spde, m, n_aux in (("euler_sympy", _flagged("euler_sympy"), 5, 1), (KT.EG, KT.flagged(KT.EG), 5, 0), (KT.TL, KT.flagged(KT.TL), 2, 1)):
        pid = spde.register()
        Q = K1.state("benign", n, 3, P, H, m + n_aux, 91) if m == 5 else KT.state(name, "benign", n, 3, P, H, m + n_aux, 91)
        dt, h = (K.cfl_step(Q, 3, R.PDE_EULER) if m == 5 else KT.cfl_step(name, 3, Q.reshape(-1, Q.shape[-1])))
        resident = exa.FVRusanovKernel(3, P, H, m, n_aux, n, pid, exa.FV_MUSCL_HANCOCK)
        streamed = exa.FVRusanovKernel(3, P, H, m, n_aux, n, pid, exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_ALWAYS)
        assert streamed.streamed and not resident.streamed
        for entry in KS.ENTRIES:
            want, _ = _run(resident, entry, Q, dt, h, n)
            got, _ = _run(streamed, entry, Q, dt, h, n)
            assert np.array_equal(_bits(got), _bits(want)), "%s %s: the streamed kernel differs from the resident one" % (name, entry)
            if entry == "inplace":
                assert not np.array_equal(got, Q)


def test_generated_euler_streamed_against_the_builtin_kernel(exa):
    import torch
    from tests.test_fv_muscl_grid import _flagged
    spde = _flagged("euler_sympy")
    n, P, H = 2, 10, 2
    Q = K1.state("benign", n, 3, P, H, 5, 77)
    dt, h = K.cfl_step(Q, 3, R.PDE_EULER)
    res = []
    for pde in (exa.PDE_EULER, spde.register()):
        kern = exa.FVRusanovKernel(3, P, H, 5, 0, n, pde, exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_IF_NEEDED)
        assert kern.streamed
        qd = torch.as_tensor(Q).cuda()
        kern.time_step(qd, dt, h)
        res.append(qd.cpu().numpy())
    err = float(np.max(np.abs(res[0] - res[1])) / np.max(np.abs(res[0])))
    print("generated Euler against the built-in kernel, streamed, P = 10: %.3e of the largest magnitude" % err)
    assert err <= 1e-14, err
    assert not np.array_equal(res[0], Q)


def test_generated_euler_with_gravity_streamed_within_bound(exa):
    from tests import fv_muscl_terms_cases as KT
    from tests import fv_muscl_terms_ref as T
    name, dim, P, H, n = KT.EG, 3, 10, 2, 2
    m, tm = KT.n_real(name), KT.terms(name)
    kern = exa.FVRusanovKernel(dim, P, H, m, 0, n, KT.flagged(name).register(), exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_IF_NEEDED)
    assert kern.streamed
    sel = T.interior(dim, P, H)
    for family in KT.FAMILIES:
        Q = KT.state(name, family, n, dim, P, H, m, 733 + KT.FAMILIES.index(family))
        dt, h = KT.cfl_step(name, dim, Q.reshape(-1, Q.shape[-1]))
        ref = T.update(Q, dt, h, dim, P, H, m, 0, terms=tm)
        got, _ = _run(kern, "inplace", Q, dt, h, n)
        err = np.abs(got[sel][..., :m].astype(R.LD) - ref.new[sel][..., :m])
        worst = float(np.max(err / (R.U53 * ref.E)))
        print("Euler with gravity, streamed, P = 10 %s: err / bound %.3f" % (family, worst))
        log_fv_measurement(what="user gravity streamed %s" % family, ratio=worst, scheme="muscl-hancock-terms-streamed")
        assert worst <= 1.0, (family, worst)
        keep = np.ones(Q.shape[1:], dtype=bool)
        keep[sel[1:] + (slice(0, m),)] = False
        assert np.array_equal(_bits(got[:, keep]), _bits(Q[:, keep])) and not np.array_equal(got[sel], Q[sel])
        out, _ = _run(kern, "oop", Q, dt, h, n)
        assert np.array_equal(_bits(out.reshape(Q[sel].shape)), _bits(got[sel]))

"""The MUSCL-Hancock patch kernels (exahype_amd/csrc/exa_fv_muscl.hpp, mode FV_MUSCL_HANCOCK) against the long-double restatement
(tests/fv_muscl_ref.py), for every row of tests/fv_muscl_cases.py times every state family, through the three forms of the call: in place, with
a slot array (fv_cases.SLOT_PATTERN) and out of place.

Per case: every evolved variable of every interior volume lies within 2^-53 E of the restatement (E: the operation count of the five
statements, tests/fv_muscl_ref.py -- tests/test_fv_muscl_reference.py shows on the CPU that a plain fp64 evaluation stays inside it and that
every mutant leaves it 100-fold); halo and auxiliary values are bit-equal to the input; masked patches are bit-equal; the out-of-place result
is bit-equal to the in-place one (a store before a neighbour's read would show here); a second launch is bit-equal to the first; and with
every entry outside the stencil -- (+-2, +-1), the 3-D corners, layers beyond the second -- set to NaN the result is bit-equal to the one
without.  EXA_FV_ERR_LOG=<file>: one JSON line per comparison (tests/util.py log_fv_measurement).
"""
import ctypes as C

import numpy as np
import pytest

from oracle import fv_reference as R
from tests import fv_cases as K1
from tests import fv_muscl_cases as K
from tests import fv_muscl_ref as M
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


def _run(exa, kern, entry, Q, dt, h, n):
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
    assert np.array_equal(qd.cpu().numpy(), Q, equal_nan=True), "time_step_oop wrote its input"
    return out.cpu().numpy(), None


@pytest.mark.parametrize("row", K.ROWS, ids=K.row_id)
def test_patch_update_within_bound(exa, row):
    dim, P, H, n_real, n_aux, n, pde, _ = row
    kern = exa.FVRusanovKernel(dim, P, H, n_real, n_aux, n, _pde(exa, pde), exa.FV_MUSCL_HANCOCK)
    sel = M.interior(dim, P, H)
    outside = M.outside_stencil(dim, P, H)
    for family in K.families(row):
        Q = K.row_state(row, family)
        dt, h = K.cfl_step(Q, dim, pde)
        ref = M.update(Q, dt, h, dim, P, H, n_real, n_aux, pde)              # one reference, shared by the three forms
        keep = np.ones(Q.shape[1:], dtype=bool)
        keep[sel[1:] + (slice(0, n_real),)] = False                          # halo entries and auxiliary variables
        results = {}
        for entry in K.ENTRIES:
            what = "%s %s %s" % (K.row_id(row), family, entry)
            got, masked = _run(exa, kern, entry, Q, dt, h, n)
            results[entry] = got
            gi = got[sel] if entry != "oop" else got.reshape(Q[sel].shape)
            live = np.ones(n, dtype=bool) if masked is None else ~masked
            err = np.abs(gi[..., :n_real].astype(R.LD) - ref.new[sel][..., :n_real])
            worst = float(np.max((err / (R.U53 * ref.E))[live]))
            print("%s: err / bound %.3f" % (what, worst))
            log_fv_measurement(what=what, row=K.row_id(row), family=family, entry=entry, ratio=worst, scheme="muscl-hancock")
            assert worst <= 1.0, (what, worst)
            assert np.array_equal(gi[..., n_real:], Q[sel][..., n_real:]), what + ": auxiliary variables changed"
            if entry != "oop":
                assert np.array_equal(got[:, keep], Q[:, keep]), what + ": halo or auxiliary values changed"
                assert np.array_equal(got[~live], Q[~live]), what + ": a masked patch was written"
        assert np.array_equal(results["oop"].reshape(Q[sel].shape), results["inplace"][sel]), "out of place differs from in place"
        live = K1.slot_of(n) >= 0
        assert np.array_equal(results["slot"][live], results["inplace"][live]), "the masked call differs on the patches in use"
        # a second launch gives the same bits
        again, _ = _run(exa, kern, "inplace", Q, dt, h, n)
        assert np.array_equal(again, results["inplace"]), "a second launch differs"
        # nothing outside the stencil is read
        Qn = Q.copy()
        Qn[:, outside] = np.nan
        got_nan, _ = _run(exa, kern, "inplace", Qn, dt, h, n)
        assert np.array_equal(got_nan[sel], results["inplace"][sel]), "an entry outside the stencil was read"
        out_nan, _ = _run(exa, kern, "oop", Qn, dt, h, n)
        assert np.array_equal(out_nan, results["oop"]), "an entry outside the stencil was read (out of place)"


def test_negative_control_h_off_by_2m30(exa):
    """the measure sees a 1e-9 error on the real kernel: run with h (1 + 2^-30) it leaves the bound"""
    row = K.ROWS[1]
    dim, P, H, n_real, n_aux, n, pde, _ = row
    Q = K.row_state(row, "supersonic")
    dt, h = K.cfl_step(Q, dim, pde)
    kern = exa.FVRusanovKernel(dim, P, H, n_real, n_aux, n, _pde(exa, pde), exa.FV_MUSCL_HANCOCK)
    got, _ = _run(exa, kern, "inplace", Q, dt, h * (1 + 2.0 ** -30), n)
    worst = M.ratio(got, M.update(Q, dt, h, dim, P, H, n_real, n_aux, pde), M.interior(dim, P, H))
    print("negative control: err / bound %.3g" % worst)
    assert worst > 1.0, worst


def test_host_entry_and_coordinates_are_ignored(exa):
    """exa_fv_time_step_host, and _device_at / _device_masked_at with centres and a time: the same bits as the plain device call"""
    import torch
    row = K.ROWS[1]
    dim, P, H, n_real, n_aux, n, pde, _ = row
    Q = K.row_state(row, "benign")
    dt, h = K.cfl_step(Q, dim, pde)
    kern = exa.FVRusanovKernel(dim, P, H, n_real, n_aux, n, _pde(exa, pde), exa.FV_MUSCL_HANCOCK)
    want, _ = _run(exa, kern, "inplace", Q, dt, h, n)
    host = Q.copy()
    kern.time_step(host, dt, h)
    assert np.array_equal(host, want)
    cen = torch.rand(n, dim, dtype=torch.float64, device="cuda")
    qd = torch.as_tensor(Q).cuda()
    kern.time_step(qd, dt, h, t=0.7, centres=cen)
    assert np.array_equal(qd.cpu().numpy(), want)
    slot = K1.slot_of(n)
    qd = torch.as_tensor(Q).cuda()
    kern.time_step(qd, dt, h, slot=torch.as_tensor(slot).cuda(), t=0.7, centres=cen)
    assert np.array_equal(qd.cpu().numpy()[slot >= 0], want[slot >= 0]) and np.array_equal(qd.cpu().numpy()[slot < 0], Q[slot < 0])
    with pytest.raises(Exception, match="h > 0"):
        kern.time_step(torch.as_tensor(Q).cuda(), dt, 0.0)


def test_refusals_on_the_device(exa):
    """3-D P = 12 is refused at plan creation with the bytes; both grid-step entries refuse the mode"""
    import torch
    from exahype_amd import _lib
    with pytest.raises(_lib.ExaHypeHipError, match=r"273600.*163840"):
        exa.FVRusanovKernel(3, 12, 2, 5, 0, 1, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK)
    with pytest.raises(_lib.ExaHypeHipError, match="two halo layers"):
        exa.FVRusanovKernel(2, 4, 1, 5, 0, 1, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK)
    kern = exa.FVRusanovKernel(2, 4, 2, 5, 0, 4, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK)
    lib = kern.lib
    U = torch.zeros(2, 2, 4, 4, 5, dtype=torch.float64, device="cuda")
    U2 = torch.zeros_like(U)
    lam = torch.zeros(1, dtype=torch.float64, device="cuda")
    grid = _lib.larr([2, 2])
    p = lambda t: C.c_void_p(t.data_ptr())     # noqa: E731
    rc = lib.exa_fv_grid_step_device(kern._plan, p(U), p(U2), grid, None, None, 0.0, 1e-3, 0.1, p(lam), None)
    msg = lib.exa_last_error().decode()
    assert rc == -1 and "face neighbours only" in msg and "edge neighbours" in msg and "array with halo" in msg, (rc, msg)
    kinds = (C.c_int * 4)(0, 0, 0, 0)
    rc = lib.exa_fv_grid_step_device_bc(kern._plan, p(U), p(U2), grid, kinds, None, None, 0.0, 1e-3, 0.1, p(lam), None)
    assert rc == -1 and "face neighbours only" in lib.exa_last_error().decode()
    with pytest.raises(ValueError, match="fused=False"):
        exa.FVPatchGrid(2, (2, 2), 4, 2, 5, 0, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK)
    with pytest.raises(ValueError, match="halo_size"):
        exa.FVPatchGrid(2, (2, 2), 4, 1, 5, 0, exa.PDE_EULER, exa.FV_MUSCL_HANCOCK, fused=False)

"""Which entry of include/exahype_hip.h serves which term set: the availability matrix, built-in and generated sets alike, in 2-D and 3-D.

Every cell is either served (EXA_OK, finite output, exa_last_error untouched) or refused with an error code and a piece of the message, before
any launch.  The tables below are written from capi.cpp and the kernel units' launchers as they stand; VALUES are not this file's business (the
per-unit suites hold every entry to its restatement).  Only entries of the header are called, through exahype_amd._lib.

Term sets: the built-in ones, three generated ones that other test modules define (their side libraries are the cached ones) and an id nobody
registered:
    ref2d, euler, advection     EXA_PDE_EULER_REF2D (2-D only, no MUSCL-Hancock, no conservative interface), EXA_PDE_EULER, EXA_PDE_ADVECTION
    euler_sympy                 tests/user_term_sets.py: 3-D, no optional unit
    swe_cons                    tests/test_limiter_conservative_user.py: 2-D only, admissible= and conservative_interface=True
    euler_muscl                 tests/fv_muscl_grid_cases.py flagged("euler_sympy"): 3-D, muscl_hancock=True
    unregistered                100 + 999

Shapes: the smallest each entry takes -- FV P = 2, H = 1 (first-order modes) or 2 (EXA_FV_MUSCL_HANCOCK), 2 patches as a 2 x 1 (x 1) grid; DG and
limiter N = 2, 2 x 2 (x 2) cells, cell 0 listed as troubled; a smooth positive state.

CPU: the cells exa_fv_plan_create[_streamed] / exa_dg_plan_create refuse before they look for a device.  GPU: every cell."""
import ctypes as C
import functools

import numpy as np
import pytest

from exahype_amd import _lib

gpu = pytest.mark.gpu
INVALID, NO_DEVICE = -1, -3
SETS = ("ref2d", "euler", "advection", "euler_sympy", "swe_cons", "euler_muscl", "unregistered")
BUILTIN = {"ref2d": _lib.PDE_EULER_REF2D, "euler": _lib.PDE_EULER, "advection": _lib.PDE_ADVECTION, "unregistered": 100 + 999}
NV = {"ref2d": 5, "euler": 5, "advection": 1, "euler_sympy": 5, "swe_cons": 3, "euler_muscl": 5, "unregistered": 5}
# a positive state of each layout: (rho, m, E) with E last -- ref2d: E fourth --, (h, hu, hv), one advected scalar
BASE = {"ref2d": (1.0, 0.1, 0.1, 2.5, 0.0), "euler": (1.0, 0.1, 0.1, 0.1, 2.5), "advection": (1.0,), "swe_cons": (1.0, 0.1, 0.1)}
BASE["euler_sympy"] = BASE["euler_muscl"] = BASE["unregistered"] = BASE["euler"]


@functools.lru_cache(maxsize=None)
def pde_id(name):
    if name in BUILTIN:
        return BUILTIN[name]
    if name == "euler_sympy":
        from tests.user_term_sets import euler_sympy
        return euler_sympy().register()
    if name == "swe_cons":
        from tests.test_limiter_conservative_user import swe_cons
        return swe_cons().register()
    from tests.fv_muscl_grid_cases import flagged
    return flagged("euler_sympy").register()


# ---- the expected matrix.  None: served.  ("plan", text): the plan's creation is refused.  ("call", text): the plan exists, every entry of the
# row refuses.  text: a piece of the message.
def plan(text):
    return ("plan", text)


def call(text):
    return ("call", text)


REF_2D_ONLY = plan("EULER_REF2D is the reference's 2-D term set")
REF_QUIRK = plan("EULER_REF2D is the reference's quirk set")
NO_MUSCL = plan("was generated without the MUSCL-Hancock kernel; build it with SympyPDE(..., muscl_hancock=True)")
UNREGISTERED = plan("pde 1099 is not registered")
STREAM_2D = plan("EXA_FV_STREAM_ALWAYS in 2-D")
NO_FV_3D = call("no FV kernel for dim 3")
NO_DG = plan("ADER-DG: no kernels for dim")
NO_INTERFACE = call("the conservative interface is built for the built-in Euler (pde 1, 5 variables) and advection (pde 2, 1 variable) sets")


def row(ref2d, euler, advection, euler_sympy, swe_cons, euler_muscl, unregistered):
    return dict(zip(SETS, (ref2d, euler, advection, euler_sympy, swe_cons, euler_muscl, unregistered)))


FIRST_ORDER = {2: row(None, None, None, None, None, None, UNREGISTERED),
               3: row(REF_2D_ONLY, None, None, None, NO_FV_3D, None, UNREGISTERED)}
MUSCL = {2: row(REF_QUIRK, None, None, NO_MUSCL, NO_MUSCL, None, UNREGISTERED),
         3: row(REF_2D_ONLY, None, None, NO_MUSCL, NO_MUSCL, None, UNREGISTERED)}
# rows: (mode, halo_size, stream_planes) -> {dim: {set: expectation}}.  The entries of a row: the in-place step; first-order modes also out of
# place, the grid step exa_fv_grid_step_device_bc and exa_fv_max_eigenvalue; resident MUSCL-Hancock also out of place and exa_fv_grid_step_muscl_device
FV = {
    "faithful": (_lib.FV_FAITHFUL, 1, _lib.FV_STREAM_NEVER, FIRST_ORDER),
    "rusanov": (_lib.FV_RUSANOV, 1, _lib.FV_STREAM_NEVER, FIRST_ORDER),
    "muscl": (_lib.FV_MUSCL_HANCOCK, 2, _lib.FV_STREAM_NEVER, MUSCL),
    # (the stream_planes check comes before the term set is looked at)
    "muscl-streamed": (_lib.FV_MUSCL_HANCOCK, 2, _lib.FV_STREAM_ALWAYS, {2: row(*[STREAM_2D] * 7), 3: MUSCL[3]}),
}
# exa_pde_eval_device with normal = dim - 1
EVAL = {2: row(None, None, None, None, None, None, call("pde 1099 is not registered")),
        3: row(call("EULER_REF2D needs normal < 2"), None, None, None, None, None, call("pde 1099 is not registered"))}
DG = {2: row(None, None, None, None, None, None, NO_DG),
      3: row(NO_DG, None, None, None, NO_DG, None, NO_DG)}
# on a DG plan that exists: exa_lim_snapshot is served for every set; exa_lim_detect reads the Euler layout where the set has no criterion
DETECT = row(None, None, call("exa_lim_detect: needs a density and an energy (n_vars >= 2), the plan has 1"), None, None, None, None)
# exa_lim_face_flux / exa_lim_interface_correct.  (A set that has the interface with another variable count than the plan's cannot be reached: a DG
# plan takes the set's own count only.)
INTERFACE = row(NO_INTERFACE, None, None, NO_INTERFACE, None, NO_INTERFACE, None)

CELLS = [(name, dim, s) for name in FV for dim in (2, 3) for s in SETS]
# (the generated sets' side libraries are the ones other unmarked tests build and register)
CPU_FV_CELLS = [(name, dim, s) for name, dim, s in CELLS if FV[name][3][dim][s] is not None and FV[name][3][dim][s][0] == "plan"]
CPU_DG_CELLS = [(dim, s) for dim in (2, 3) for s in SETS if DG[dim][s] is not None]


def last_error():
    return _lib.load().exa_last_error().decode()


def refused(rc, want, what):
    assert rc == INVALID and want[1] in last_error(), (what, rc, last_error())


def fv_plan(name, dim, s):
    mode, H, stream, _ = FV[name]
    p = C.c_void_p()
    rc = _lib.load().exa_fv_plan_create_streamed(0, mode, dim, 2, H, NV[s], 0, 2, pde_id(s), stream, C.byref(p))
    return rc, p


def dg_plan(dim, s):
    p = C.c_void_p()
    rc = _lib.load().exa_dg_plan_create(0, dim, 2, NV[s], pde_id(s), -1, _lib.larr([2] * dim), C.byref(p))
    return rc, p


@pytest.mark.parametrize("name,dim,s", CPU_FV_CELLS)
def test_fv_plan_refusals_need_no_device(name, dim, s):
    rc, p = fv_plan(name, dim, s)
    refused(rc, FV[name][3][dim][s], "exa_fv_plan_create_streamed")
    assert not p.value


@pytest.mark.parametrize("dim,s", CPU_DG_CELLS)
def test_dg_plan_refusals_need_no_device(dim, s):
    rc, p = dg_plan(dim, s)
    refused(rc, DG[dim][s], "exa_dg_plan_create")
    assert not p.value


def test_the_tables_name_every_cell():
    for _, _, _, table in FV.values():
        assert sorted(table) == [2, 3] and all(sorted(table[d]) == sorted(SETS) for d in table)
    # counted by hand from the rows above -- first-order: unregistered twice, ref2d in 3-D, for two modes; resident MUSCL-Hancock: ref2d,
    # euler_sympy, swe_cons and unregistered in both dimensions; streamed: all seven sets in 2-D, those four in 3-D.  DG: unregistered twice, ref2d
    # and swe_cons in 3-D
    assert len(CPU_FV_CELLS) == 2 * 3 + 8 + 11 and len(CPU_DG_CELLS) == 4


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def state(s, shape):
    """[shape.., nv]: BASE with a smooth 10 % modulation of the first variable"""
    n = int(np.prod(shape))
    q = np.tile(np.array(BASE[s]), (n, 1))
    q[:, 0] *= 1.0 + 0.1 * np.sin(2 * np.pi * (np.arange(n) + 0.5) / n)
    return q.reshape(tuple(shape) + (NV[s],))


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


SENTINEL = -7.25


def fresh(*shape):
    """an output array no entry has written yet"""
    return dev(np.full(shape, SENTINEL))


def finite(*tensors):
    """every element is finite, and the first variable of every state is not the sentinel any more: the entry did launch"""
    import torch
    torch.cuda.synchronize()
    return all(bool(torch.isfinite(t.double()).all()) and bool((t.reshape(-1, t.shape[-1])[:, 0] != SENTINEL).all()) for t in tensors)


class Untouched:
    """leaves a known message behind exa_last_error; .ok(rc, ..): the call was served and did not write one"""

    def __init__(self):
        assert _lib.load().exa_device_count(None) == INVALID
        self.mark = last_error()
        assert "exa_device_count" in self.mark

    def ok(self, rc, what):
        assert rc == 0 and last_error() == self.mark, (what, rc, last_error())


@gpu
@pytest.mark.parametrize("name,dim,s", CELLS)
def test_fv_entries(name, dim, s):
    lib = _lib.load()
    mode, H, stream, table = FV[name]
    want = table[dim][s]
    pde_id(s)                                                      # (registered before the mark: building a side library may write messages)
    mark = Untouched()
    rc, p = fv_plan(name, dim, s)
    if want is not None and want[0] == "plan":
        refused(rc, want, "exa_fv_plan_create_streamed")
        return
    mark.ok(rc, "exa_fv_plan_create_streamed")
    try:
        assert lib.exa_fv_plan_is_streamed(p) == (stream == _lib.FV_STREAM_ALWAYS)
        P, S, nv = 2, 2 + 2 * H, NV[s]
        assert lib.exa_fv_q_count(p) == 2 * S ** dim * nv and lib.exa_fv_qout_count(p) == 2 * P ** dim * nv
        q, qin = dev(state(s, (2,) + (S,) * dim)), dev(state(s, (2,) + (S,) * dim))
        u, out, nxt = dev(state(s, (2,) + (P,) * dim)), fresh(*((2,) + (P,) * dim + (nv,))), fresh(*((2,) + (P,) * dim + (nv,)))
        lam_grid, lam_scan = fresh(1, 1), fresh(1, 1)
        grid = _lib.larr([2] + [1] * (dim - 1))
        dt, h = 1e-3, 0.5
        entries = [("exa_fv_time_step_device", lambda: lib.exa_fv_time_step_device(p, q.data_ptr(), dt, h, None), (q,))]
        if stream == _lib.FV_STREAM_NEVER:
            entries.append(("exa_fv_time_step_device_oop", lambda: lib.exa_fv_time_step_device_oop(p, qin.data_ptr(), out.data_ptr(), None, 0.0, dt, h, None), (out,)))
        if mode != _lib.FV_MUSCL_HANCOCK:
            entries.append(("exa_fv_grid_step_device_bc", lambda: lib.exa_fv_grid_step_device_bc(p, u.data_ptr(), nxt.data_ptr(), grid, None, None, None, 0.0, dt, h,
                                                                                                 lam_grid.data_ptr(), None), (nxt, lam_grid)))
            entries.append(("exa_fv_max_eigenvalue", lambda: lib.exa_fv_max_eigenvalue(p, qin.data_ptr(), 0, None, 0.0, h, lam_scan.data_ptr(), None), (lam_scan,)))
        elif stream == _lib.FV_STREAM_NEVER:
            entries.append(("exa_fv_grid_step_muscl_device", lambda: lib.exa_fv_grid_step_muscl_device(p, u.data_ptr(), nxt.data_ptr(), grid, None, None, dt, h,
                                                                                                       lam_grid.data_ptr(), None), (nxt, lam_grid)))
        for what, entry, written in entries:
            if want is None:
                mark.ok(entry(), what)
                assert finite(*written), what
                assert written[0] is not q or not bool((q == qin).all()), what      # (in place: the states moved)
            else:
                refused(entry(), want, what)
    finally:
        lib.exa_fv_plan_destroy(p)


@gpu
@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("s", SETS)
def test_pde_eval(s, dim):
    lib = _lib.load()
    want = EVAL[dim][s]
    q = dev(state(s, (7,)))
    f, lam = fresh(7, NV[s]), fresh(7, 1)
    if want is None:
        mark = Untouched()
        mark.ok(lib.exa_pde_eval_device(pde_id(s), dim - 1, 7, NV[s], q.data_ptr(), f.data_ptr(), lam.data_ptr(), None), "exa_pde_eval_device")
        assert finite(f, lam)
    else:
        refused(lib.exa_pde_eval_device(pde_id(s), dim - 1, 7, NV[s], q.data_ptr(), f.data_ptr(), lam.data_ptr(), None), want, "exa_pde_eval_device")


@gpu
@pytest.mark.parametrize("dim", (2, 3))
@pytest.mark.parametrize("s", SETS)
def test_dg_and_limiter_entries(s, dim):
    lib = _lib.load()
    want = DG[dim][s]
    pde_id(s)
    mark = Untouched()
    rc, p = dg_plan(dim, s)
    if want is not None:
        refused(rc, want, "exa_dg_plan_create")
        return
    mark.ok(rc, "exa_dg_plan_create")
    try:
        N, nv, ncells = 2, NV[s], 2 ** dim
        assert lib.exa_dg_dof_count(p) == ncells * N ** dim * nv
        u = dev(state(s, (2,) * dim + (N,) * dim))
        trace = fresh(lib.exa_dg_trace_count(p))
        dt, dx = 1e-3, _lib.darr([0.5] * dim)
        mark.ok(lib.exa_dg_step_periodic(p, u.data_ptr(), trace.data_ptr(), dt, dx, 1, None), "exa_dg_step_periodic")
        assert finite(u, trace)

        nb = lib.exa_lim_bounds_count(p)
        assert nb == (2 if s == "swe_cons" else 4)                 # (swe_cons watches the depth; every other set here: the Euler layout's two)
        old, bounds, mask = fresh(*u.shape), fresh(ncells, nb), dev(np.zeros(ncells, dtype=np.uint8))
        mark.ok(lib.exa_lim_snapshot(p, u.data_ptr(), old.data_ptr(), bounds.data_ptr(), None), "exa_lim_snapshot")
        assert finite(old, bounds)
        rc = lib.exa_lim_detect(p, u.data_ptr(), bounds.data_ptr(), None, None, 1e-4, 1e-3, 1e-12, mask.data_ptr(), None)
        if DETECT[s] is None:
            mark.ok(rc, "exa_lim_detect")
            assert finite(mask)
        else:
            refused(rc, DETECT[s], "exa_lim_detect")
            mark = Untouched()

        cells = dev(np.array([0], dtype=np.int64))
        mask = dev(np.array([1] + [0] * (ncells - 1), dtype=np.uint8))
        patch = dev(np.zeros(lib.exa_lim_patch_count(p)))
        fvflux = fresh(lib.exa_lim_face_flux_count(p))
        mark.ok(lib.exa_dg_project_patches(p, u.data_ptr(), cells.data_ptr(), 1, patch.data_ptr(), None), "exa_dg_project_patches")
        flux = lib.exa_lim_face_flux(p, patch.data_ptr(), cells.data_ptr(), 1, fvflux.data_ptr(), None)
        if INTERFACE[s] is None:
            mark.ok(flux, "exa_lim_face_flux")
            mark.ok(lib.exa_lim_interface_correct(p, u.data_ptr(), trace.data_ptr(), cells.data_ptr(), 1, mask.data_ptr(), None, fvflux.data_ptr(), dt, dx, None),
                    "exa_lim_interface_correct")
            assert finite(patch, fvflux, u)
        else:
            refused(flux, INTERFACE[s], "exa_lim_face_flux")
            refused(lib.exa_lim_interface_correct(p, u.data_ptr(), trace.data_ptr(), cells.data_ptr(), 1, mask.data_ptr(), None, fvflux.data_ptr(), dt, dx, None),
                    INTERFACE[s], "exa_lim_interface_correct")
    finally:
        lib.exa_dg_plan_destroy(p)

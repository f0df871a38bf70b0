"""CPU checks for the plane-streaming form of the MUSCL-Hancock update (exa_fv_plan_create_streamed; tests/fv_muscl_stream_cases.py) -- no GPU.

  * the Python restatement of fv_muscl_stream_plan gives the byte counts the plan was designed to (106 880 B at P = 15, 158 720 B at P = 19,
    173 280 B at P = 20, 5 + 0 variables), serves 3-D P = 1 .. 19 and refuses P = 20; the resident plan stops at P = 9 (P = 10: 178 880 B);
  * exa_fv_plan_create_streamed's argument checks come before the device check: every refusal is EXA_ERR_INVALID with its message, the shapes
    the restatement serves are not refused, and stream_planes = 0 answers what exa_fv_plan_create answers on the shapes
    tests/test_fv_muscl_reference.py uses;
  * the plain fp64 form of the scheme (fv_muscl_ref.fp64_update) stays inside the long-double bound 2^-53 E on the new rows: the rows can be
    measured with it;
  * the header, the loader and the Python layer agree on the three constants.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fv_muscl_cases as K
from tests import fv_muscl_ref as M
from tests import fv_muscl_stream_cases as KS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXA_OK, EXA_ERR_INVALID, EXA_ERR_NO_DEVICE = 0, -1, -3
NEVER, IF_NEEDED, ALWAYS = 0, 1, 2
MUSCL = 2


def test_plan_restatement():
    assert KS.stream_need(15, 5, 5) == 106880 and KS.stream_need(19, 5, 5) == 158720 and KS.stream_need(20, 5, 5) == 173280
    for P in range(1, 20):
        ring, nt, lds = KS.stream_plan(P, 5, 5)
        assert nt == 256 and lds <= KS.LDS_AVAILABLE and ring in (5, 6), (P, ring, nt, lds)
        assert lds == KS.stream_need(P, 5, 5) + (ring - 5) * 8 * (P + 4) ** 2 * 5
        assert (ring == 6) == (KS.stream_need(P, 5, 5) + 8 * (P + 4) ** 2 * 5 <= KS.LDS_AVAILABLE), P
    assert KS.stream_plan(15, 5, 5) == (6, 256, 121320) and KS.stream_plan(17, 5, 5)[0] == 6 and KS.stream_plan(18, 5, 5)[0] == 5
    assert KS.stream_plan(19, 5, 5) == (5, 256, 158720)
    assert KS.stream_plan(20, 5, 5) is None
    # the resident plan: P = 9 fits, P = 10, 11, 15 do not
    assert K.lds_plan(3, 9, 5, 5) is not None and K.lds_plan(3, 10, 5, 5) is None
    assert 8 * (14 ** 3 * 5 + 12 ** 3 * 5) == 178880 and 8 * (15 ** 3 * 5 + 13 ** 3 * 5) == 222880 and 8 * (19 ** 3 * 5 + 17 ** 3 * 5) == 470880
    # every row of the tables has the plan it is there for
    for row in KS.STREAM_ROWS:
        _, P, H, n_real, n_aux, n, pde, _ = row
        assert K.lds_plan(3, P, n_real, n_real + n_aux) is None and KS.stream_plan(P, n_real, n_real + n_aux) is not None, row
    assert [KS.stream_plan(r[1], r[3], r[3] + r[4])[0] for r in KS.STREAM_ROWS].count(5) >= 1      # the five-plane ring is reached
    for shape in KS.EQUAL_SHAPES:
        P, H, n_real, n_aux, pde = shape
        assert K.lds_plan(3, P, n_real, n_real + n_aux) is not None and KS.stream_plan(P, n_real, n_real + n_aux) is not None, shape


def test_constants():
    text = open(os.path.join(ROOT, "include", "exahype_hip.h")).read()
    for name, value in (("NEVER", 0), ("IF_NEEDED", 1), ("ALWAYS", 2)):
        assert re.search(r"^#define\s+EXA_FV_STREAM_%s\s+%d\b" % (name, value), text, flags=re.M), name
    from exahype_amd import _lib, solvers
    assert (_lib.FV_STREAM_NEVER, _lib.FV_STREAM_IF_NEEDED, _lib.FV_STREAM_ALWAYS) == (0, 1, 2)
    assert (solvers.FV_STREAM_NEVER, solvers.FV_STREAM_IF_NEEDED, solvers.FV_STREAM_ALWAYS) == (0, 1, 2)


def _create(lib, *args, streamed=None):
    """-> (rc, message, is_streamed or None)"""
    h = C.c_void_p()
    rc = lib.exa_fv_plan_create(*args, C.byref(h)) if streamed is None else lib.exa_fv_plan_create_streamed(*args, streamed, C.byref(h))
    msg = lib.exa_last_error().decode()
    is_streamed = None
    if rc == EXA_OK:
        is_streamed = lib.exa_fv_plan_is_streamed(h)
        lib.exa_fv_plan_destroy(h)
    return rc, msg, is_streamed


def test_streamed_plan_refusals():
    from exahype_amd import _lib
    lib = _lib.load()
    e = _lib.PDE_EULER
    # a non-zero stream_planes with another mode
    for mode, H in ((0, 1), (1, 1)):
        for sp in (IF_NEEDED, ALWAYS):
            rc, msg, _ = _create(lib, 0, mode, 3, 4, H, 5, 0, 1, e, streamed=sp)
            assert rc == EXA_ERR_INVALID and "EXA_FV_MUSCL_HANCOCK" in msg and "stream_planes" in msg, (mode, sp, rc, msg)
    # ALWAYS in 2-D; IF_NEEDED in 2-D behaves as NEVER
    rc, msg, _ = _create(lib, 0, MUSCL, 2, 4, 2, 5, 0, 1, e, streamed=ALWAYS)
    assert rc == EXA_ERR_INVALID and "EXA_FV_STREAM_ALWAYS" in msg and "3-D only" in msg, (rc, msg)
    rc, msg, st = _create(lib, 0, MUSCL, 2, 4, 2, 5, 0, 1, e, streamed=IF_NEEDED)
    assert rc in (EXA_OK, EXA_ERR_NO_DEVICE) and st in (None, 0), (rc, msg, st)
    rc, msg, _ = _create(lib, 0, MUSCL, 2, 64, 2, 5, 0, 1, e, streamed=IF_NEEDED)           # 2-D P = 64: the resident plan's refusal, as it reads today
    want = _create(lib, 0, MUSCL, 2, 64, 2, 5, 0, 1, e)
    assert rc == EXA_ERR_INVALID and (rc, msg) == want[:2] and "window and predictor" in msg, (rc, msg)
    # a shape whose streamed plan does not fit: both byte counts
    for sp in (IF_NEEDED, ALWAYS):
        rc, msg, _ = _create(lib, 0, MUSCL, 3, 20, 2, 5, 0, 1, e, streamed=sp)
        resident = 8 * (24 ** 3 * 5 + 22 ** 3 * 5)
        assert rc == EXA_ERR_INVALID and str(resident) in msg and "173280" in msg and "163840" in msg, (sp, rc, msg)
    rc, msg, _ = _create(lib, 0, MUSCL, 3, 15, 2, 8, 2, 1, _lib.PDE_ADVECTION, streamed=IF_NEEDED)      # 8 + 2 variables at P = 15
    assert rc == EXA_ERR_INVALID and str(KS.stream_need(15, 8, 10)) in msg, (rc, msg)
    # an unknown value
    for sp in (3, -1):
        rc, msg, _ = _create(lib, 0, MUSCL, 3, 4, 2, 5, 0, 1, e, streamed=sp)
        assert rc == EXA_ERR_INVALID and "unknown stream_planes %d" % sp in msg, (sp, rc, msg)
    # the checks both entries share still come first
    rc, msg, _ = _create(lib, 0, 3, 3, 4, 2, 5, 0, 1, e, streamed=IF_NEEDED)
    assert rc == EXA_ERR_INVALID and "unknown FV mode 3" in msg, (rc, msg)
    rc, msg, _ = _create(lib, 0, MUSCL, 3, 12, 1, 5, 0, 1, e, streamed=IF_NEEDED)
    assert rc == EXA_ERR_INVALID and "two halo layers" in msg, (rc, msg)
    rc, msg, _ = _create(lib, 0, MUSCL, 3, 12, 2, 5, 0, 1, 100 + 57, streamed=IF_NEEDED)
    assert rc == EXA_ERR_INVALID and "not registered" in msg, (rc, msg)


def test_streamed_plan_serves_what_the_restatement_serves():
    from exahype_amd import _lib
    lib = _lib.load()
    gpu = _lib.device_count() > 0
    for P in range(1, 20):
        for sp in (IF_NEEDED, ALWAYS):
            rc, msg, st = _create(lib, 0, MUSCL, 3, P, 2, 5, 0, 1, _lib.PDE_EULER, streamed=sp)
            assert rc == (EXA_OK if gpu else EXA_ERR_NO_DEVICE), (P, sp, rc, msg)
            if gpu:
                assert st == (1 if sp == ALWAYS or K.lds_plan(3, P, 5, 5) is None else 0), (P, sp, st)
    for row in KS.STREAM_ROWS:
        _, P, H, n_real, n_aux, n, pde, _ = row
        rc, msg, _ = _create(lib, 0, MUSCL, 3, P, H, n_real, n_aux, n, _lib.PDE_EULER if pde == K.E else _lib.PDE_ADVECTION, streamed=IF_NEEDED)
        assert rc != EXA_ERR_INVALID, (row, msg)
        rc, msg, _ = _create(lib, 0, MUSCL, 3, P, H, n_real, n_aux, n, _lib.PDE_EULER if pde == K.E else _lib.PDE_ADVECTION)
        assert rc == EXA_ERR_INVALID and "bytes of LDS" in msg, (row, msg)          # the old entry refuses them as it did


def test_stream_planes_0_is_the_old_entry():
    """the argument lists of tests/test_fv_muscl_reference.py (test_plan_create_takes_mode_2, test_plan_create_refusals): the same code, the same
    message"""
    from exahype_amd import _lib
    lib = _lib.load()
    e = _lib.PDE_EULER
    shapes = [(0, 2, 2, 4, 2, 5, 0, 1, e), (0, 2, 2, 4, 1, 5, 0, 1, e), (0, 2, 2, 4, 2, 5, 0, 1, _lib.PDE_EULER_REF2D), (0, 3, 2, 4, 2, 5, 0, 1, e),
              (0, 2, 3, 12, 2, 5, 0, 1, e), (0, 1, 2, 4, 0, 5, 0, 1, e)]
    shapes += [(0, 2, 2, p, 2, 5, 0, 1, e) for p in range(1, 33)] + [(0, 2, 2, p, 2, 5, 5, 1, e) for p in range(1, 21)]
    shapes += [(0, 2, 3, p, 2, 5, 1, 1, e) for p in range(1, 9)]
    refused = 0
    for args in shapes:
        old = _create(lib, *args)
        new = _create(lib, *args, streamed=NEVER)
        assert old == new and new[2] in (None, 0), (args, old, new)
        refused += old[0] == EXA_ERR_INVALID
    assert refused == 5
    rc, msg, _ = _create(lib, 0, 2, 3, 12, 2, 5, 0, 1, e, streamed=NEVER)
    assert rc == EXA_ERR_INVALID and "273600" in msg and "163840" in msg, (rc, msg)


@pytest.mark.parametrize("row", KS.STREAM_ROWS, ids=K.row_id)
def test_fp64_form_is_inside_the_bound_on_the_new_rows(row):
    dim, P, H, n_real, n_aux, n, pde, _ = row
    sel = M.interior(dim, P, H)
    for family in K.families(row):
        Q = K.row_state(row, family)
        dt, h = K.cfl_step(Q, dim, pde)
        ref = M.update(Q, dt, h, dim, P, H, n_real, n_aux, pde)
        worst = M.ratio(M.fp64_update(Q, dt, h, dim, P, H, n_real, pde), ref, sel)
        print("%s %s: fp64 form err / bound %.3f" % (K.row_id(row), family, worst))
        assert 0.0 < worst <= 1.0, (K.row_id(row), family, worst)
        keep = np.ones(Q.shape[1:], dtype=bool)
        keep[sel[1:] + (slice(0, n_real),)] = False
        assert np.array_equal(ref.new[:, keep].astype(np.float64), Q[:, keep])

"""CPU checks of what the halo-2 projection of the limiter is held to (tests/limiter_muscl_ref.py) and of the feature's surface -- no GPU.

  * numpy's fp64 tensor products, assembled into the patch with halo 2, stay inside rounding_factor(dim, N) (|P| x .. x |P|) |u| on every case
    of tests/limiter_muscl_cases.py (periodic grids and faces with conditions): the bound is satisfiable, and mirrors, signs and copies add
    nothing to it;
  * every mutant of the restatement leaves that bound 100-fold on at least one case: none is exempt;
  * ghost_extend() without a mutant is fv_muscl_ref.global_with_ghosts bit for bit;
  * the restatement reproduces tests/golden/limiter_muscl_tube.json for 2-D N = 4 on 16 cells;
  * SubcellLimiter has fv_mode; the three C entry points are declared, exported and bound, return EXA_ERR_INVALID on a NULL plan or a bad argument and
    EXA_ERR_NO_DEVICE without a device;
  * the example's exact solution is the restatement's.
"""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest

from oracle import fv_reference as R
from oracle import limiter_reference as L
from oracle.dg_operators import operators
from oracle.limiter_numpy import apply_all_axes, projection_matrix
from tests import fv_muscl_ref as F
from tests import limiter_cases as K
from tests import limiter_muscl_cases as KM
from tests import limiter_muscl_ref as M2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
ENTRY_POINTS = ("exa_lim_patch_count_halo", "exa_lim_project_patches_halo2", "exa_lim_reconstruct_patches_halo")


def _P(N):
    return projection_matrix(operators(N)["xi"], 2 * N - 1)


def _all_inputs(dim, N):
    out = [(None, nc, u) for nc, u in KM.inputs(dim, N)]
    return out + [(cond, nc, u) for _, cond, nc, u in KM.bc_inputs(dim, N)]


def _worst(dim, N, mutant=None, fp64=False):
    """the largest |patch - reference| / bound over every cell of every case; fp64: the patch from numpy's fp64 products, else the mutant's
    patch in long double"""
    P = _P(N)
    worst = 0.0
    for cond, nc, u in _all_inputs(dim, N):
        proj, absproj = L.project_grid(u, P.astype(LD)), L.project_grid(np.abs(u), np.abs(P).astype(LD))
        p64 = apply_all_axes(P, u, dim, dim) if fp64 else None
        for cell in range(int(np.prod(nc))):
            cc = np.unravel_index(cell, nc)
            ref = M2.build_patch2(proj, cc, cond)
            bound = L.rounding_factor(dim, N) * M2.build_patch2(absproj, cc, M2.abs_conditions(cond))
            got = M2.build_patch2(p64, cc, cond) if fp64 else M2.build_patch2(proj, cc, cond, mutant)
            worst = max(worst, K.worst_ratio(got, ref, bound))
    return worst


@pytest.mark.parametrize("dim,N", KM.KERNEL_CASES)
def test_fp64_products_are_inside_the_bound(dim, N):
    assert _worst(dim, N, fp64=True) <= 1.0


@pytest.mark.parametrize("mutant", M2.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    worst = max(_worst(dim, N, mutant) for dim, N in ((2, 3), (3, 2)))
    assert worst >= 100.0, (mutant, worst)


def test_ghost_extend_is_the_products_halo_fill():
    for dim, N in ((2, 3), (3, 2)):
        P = _P(N)
        for cond, nc, u in _all_inputs(dim, N):
            G = R.assemble(apply_all_axes(P, u, dim, dim), dim)
            assert np.array_equal(M2.ghost_extend(G, dim, cond), F.global_with_ghosts(G, dim, conditions=cond))


def test_unread_entries_are_the_nearest_interior_value():
    dim, N = 3, 2
    Ns = 2 * N - 1
    nc, u = KM.inputs(dim, N)[0]
    proj = apply_all_axes(_P(N), u, dim, dim)
    patch = M2.build_patch2(proj, (1, 2, 0))
    near = M2.nearest_interior_index(dim, Ns)
    unread = F.outside_stencil(dim, Ns, 2)
    assert unread.sum() == (Ns + 4) ** 3 - Ns ** 3 - 6 * 2 * Ns ** 2 - 12 * Ns
    assert np.array_equal(patch[unread], patch[tuple(near)][unread])


def test_tube_golden_2d():
    """the restatement reproduces its committed run (2-D N = 4, 16 cells); every decision of the detector keeps its distance from a threshold"""
    from tests import limiter_ref as LR
    with open(os.path.join(ROOT, "tests", "golden", "limiter_muscl_tube.json")) as f:
        want = json.load(f)["cases"]["dim2_N4_nx16"]
    LR.reset_margin()
    got = M2.run_tube(4, 16, 2)
    assert LR.smallest_margin() >= 1e-8
    assert got["steps"] == want["steps"] and got["max_troubled"] == want["max_troubled"]
    for k in ("l1", "min_rho", "min_p"):
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), (k, got[k], want[k])
    assert got["min_rho"] > 0 and got["min_p"] > 0
    assert got["l1"] < want["rusanov_l1"]


def test_subcell_limiter_has_fv_mode():
    from exahype_amd import solvers as exa
    p = inspect.signature(exa.SubcellLimiter).parameters
    assert "fv_mode" in p and p["fv_mode"].default == exa.FV_RUSANOV
    assert list(p)[:2] == ["solver", "capacity"]


def test_entry_points_declared_exported_and_bound():
    from exahype_amd import _lib
    header = open(os.path.join(ROOT, "include", "exahype_hip.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name


def test_entry_points_fail_loudly():
    """EXA_ERR_INVALID (-1) on a NULL plan and on a bad argument beside a plan; without a device EXA_ERR_NO_DEVICE (-3)"""
    import torch
    from exahype_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    cells = (C.c_long * 8)()
    kinds = (C.c_int * 6)(0, 0, 0, 0, 0, 0)
    plan = C.create_string_buffer(4096)                          # stands in for a plan on a machine that cannot create one (device 0, no cells)
    P, B, L_ = C.cast(plan, C.c_void_p), C.cast(buf, C.c_void_p), C.cast(cells, C.c_void_p)
    assert lib.exa_lim_patch_count_halo(None, 2) == -1 and b"NULL plan" in lib.exa_last_error()
    assert lib.exa_lim_patch_count_halo(P, 0) == -1 and lib.exa_lim_patch_count_halo(P, 3) == -1 and b"halo must be 1 or 2" in lib.exa_last_error()
    for args in ((None, B, L_, 1, B, None, None), (P, None, L_, 1, B, None, None), (P, B, None, 1, B, None, None), (P, B, L_, 1, None, None, None),
                 (P, B, L_, -1, B, None, None)):
        assert lib.exa_lim_project_patches_halo2(*args, None) == -1
        assert b"exa_lim_project_patches_halo2" in lib.exa_last_error()
    for args in ((None, B, L_, 1, B, 2), (P, None, L_, 1, B, 2), (P, B, None, 1, B, 2), (P, B, L_, 1, None, 2), (P, B, L_, -1, B, 2),
                 (P, B, L_, 1, B, 0), (P, B, L_, 1, B, 3)):
        assert lib.exa_lim_reconstruct_patches_halo(*args, None) == -1
        assert b"exa_lim_reconstruct_patches_halo" in lib.exa_last_error()
    if not torch.cuda.is_available():
        assert lib.exa_lim_project_patches_halo2(P, B, L_, 1, B, None, None, None) == -3
        assert b"no CPU fallback" in lib.exa_last_error()
        assert lib.exa_lim_project_patches_halo2(P, B, L_, 1, B, kinds, None, None) == -3          # (all kinds periodic: no data needed)
        assert b"no CPU fallback" in lib.exa_last_error()
        assert lib.exa_lim_reconstruct_patches_halo(P, B, L_, 1, B, 2, None) == -3
        assert b"no CPU fallback" in lib.exa_last_error()


def test_example_exact_solution_is_the_restatements():
    from examples import sod_tube_limited_second_order as ex
    from tests import limiter_mood_ref as M
    x = np.linspace(0.01, 0.99, 197)
    assert np.array_equal(ex.exact_double(x, 0.1), M.exact_double(x, 0.1))

"""The one-launch MUSCL-Hancock grid step without a GPU: the entry point is declared, bound and exported and refuses a NULL plan; the opt-in
value exists; and every grid case the GPU tests run (tests/fv_muscl_grid_cases.py) can SEE its edge entries -- with the edge ghost entries of
the global array replaced by the nearest interior value (what a gather of face neighbours only would leave), the update leaves the bound
2^-53 E of the restatement.  A case whose inputs could not tell the two apart would prove nothing on the GPU.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import fv_reference as R
from tests import fv_muscl_grid_cases as G
from tests import fv_muscl_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "exa_fv_grid_step_muscl_device"


def test_entry_declared_bound_and_exported():
    from exahype_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "exahype_hip.h")).read(), flags=re.S)
    decl = re.search(r"int\s+%s\s*\(([^)]*)\)" % NAME, text)
    assert decl, "include/exahype_hip.h does not declare %s" % NAME
    assert len(decl.group(1).split(",")) == 10
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 10
    assert hasattr(_lib.load(), NAME)


def test_null_plan_is_refused_with_a_message():
    from exahype_amd import _lib
    lib = _lib.load()
    rc = lib.exa_fv_grid_step_muscl_device(None, None, None, _lib.larr([1, 1]), None, None, 0.1, 0.1, None, None)
    assert rc == -1                                                # EXA_ERR_INVALID
    msg = lib.exa_last_error().decode()
    assert NAME in msg and "NULL" in msg, msg


def test_opt_in_value():
    from exahype_amd import solvers
    assert solvers.FUSED_EDGES == "edges"
    assert solvers.FUSED_EDGES is not True and solvers.FUSED_EDGES                 # (distinct from the default, and true: the states live halo-less)


def _edges_from_the_interior(A, dim):
    """A: the global array with two ghost layers -> a copy whose edge ghost entries (layer 1 along two axes, any position along a third) hold the
    nearest interior value"""
    B = A.copy()
    for a in range(dim):
        for b in range(a + 1, dim):
            for sa in (0, 1):
                for sb in (0, 1):
                    dst, src = [slice(None)] * A.ndim, [slice(None)] * A.ndim
                    na, nb = A.shape[a], A.shape[b]
                    dst[a], src[a] = (1, 2) if sa == 0 else (na - 2, na - 3)
                    dst[b], src[b] = (1, 2) if sb == 0 else (nb - 2, nb - 3)
                    B[tuple(dst)] = A[tuple(src)]
    return B


def _ratios(case):
    """err / bound of the fp64 restatement of `case` (benign) with its own ghost entries, and with the edge ghost entries from the interior"""
    s = G.setup(case, "benign")
    ref = G.reference(s)
    A = M.global_with_ghosts(R.assemble(s.U, s.dim), s.dim, s.ref_boundary, s.conditions)
    assert not np.array_equal(_edges_from_the_interior(A, s.dim), A)
    own = M.update_block(A[None].astype(np.float64), s.dt, s.h, s.dim, s.n_real, s.pde, s.terms, track=False)[0][0]
    face_only = M.update_block(_edges_from_the_interior(A, s.dim)[None].astype(np.float64), s.dt, s.h, s.dim, s.n_real, s.pde, s.terms, track=False)[0][0]
    r_own = M.ratio(R.cut_patches(own, s.dim, s.grid, s.P), ref)
    r_face = M.ratio(R.cut_patches(face_only, s.dim, s.grid, s.P), ref)
    print("%s: fp64 restatement err / bound %.3f; with the edge entries from the interior %.3e" % (case, r_own, r_face))
    return r_own, r_face


@pytest.mark.parametrize("case", G.GPU_CASES)
def test_the_inputs_see_their_edge_entries(case):
    r_own, r_face = _ratios(case)
    assert r_own <= 1.0, (case, r_own)
    assert r_face > 1.0, (case, r_face)


@pytest.mark.parametrize("case", G.BLIND_TO_ITS_CORNERS)
def test_why_a_case_is_off_the_gpu_list(case):
    """prescribed states on both faces of a corner: the update does not depend on the edge entry there, so the case is not on the GPU list"""
    assert case in G.CASES and case not in G.GPU_CASES
    r_own, r_face = _ratios(case)
    assert r_own <= 1.0 and r_face <= 1.0, (case, r_own, r_face)

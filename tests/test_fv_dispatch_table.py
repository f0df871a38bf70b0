"""tests/fv_cases.py reaches every branch of `fv_dispatch` (exahype_amd/csrc/fv_rusanov.hip) in corrected mode: fv_cases.branch() restates the
dispatch conditions, every row names the branch it reaches, every branch has a row, and the thresholds branch() assumes are the ones the
source states -- a later change of a threshold turns this red instead of silently moving a case.  The thresholds are matched as literal source
lines, so a pure reformat of fv_dispatch turns the last test red too: it fails closed -- whoever reformats the dispatch confirms the thresholds
and updates the needles."""
import os
import re

from tests import fv_cases as K

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "exahype_amd", "csrc", "fv_rusanov.hip")


def test_every_row_reaches_the_branch_it_names():
    for row in K.ROWS:
        assert K.branch(*row[1:]) == row[0], K.row_id(row)
        assert row[0] in K.BRANCHES


def test_every_branch_has_a_row():
    reached = {K.branch(*row[1:]) for row in K.ROWS}
    assert reached == set(K.BRANCHES), set(K.BRANCHES) ^ reached
    entries = {row[8].split(":")[0] + (":" + row[8].split(":")[1] if ":" in row[8] else "") for row in K.ROWS}
    assert entries == {"inplace", "slot", "oop", "grid:periodic", "grid:dirichlet"}
    grids = [K.grid_of(r)[0] for r in K.ROWS if r[8].startswith("grid")]
    assert any(1 in g for g in grids)                                                        # an extent of 1: the patch is its own neighbour
    assert any(r[0].startswith("slab") and r[6] % 8 for r in K.ROWS if r[8].startswith("grid"))     # fv_xcd_contiguous: a count that is no multiple of 8
    # the kernel with the fast reciprocal / square root is reached through the in-place call, the masked call and the grid step
    assert {r[8].split(":")[0] for r in K.ROWS if K.uses_device_primitives(r)} == {"inplace", "slot", "grid"}


def test_thresholds_are_the_ones_the_source_states():
    src = open(SRC).read()
    body = src[src.index("static int fv_dispatch("):src.index("static int fv_mode(")]
    for needle in ["if (ncell <= 256) {", "const int ppb = (int)(256 / ncell);", "n_patches >= (long)ppb * 2048",
                   "if (DIM == 2 && P == 4 && H == 1 && m == 5 && V == 10) {", "lds <= 64 * 1024", "} else if (ncell <= 1024) {",
                   "DIM == 3 && P * P <= 256 && S * S * V <= 2 * SLAB_NR * SLAB_NT", "(!cd.out || GRID) && (!GRID || 4 * H * P * V <= SLAB_NH * SLAB_NT)",
                   "if (lds > 64 * 1024) {", "} else if (ncell <= 4096) {", "(GRID ? (size_t)ppb * 32 : 0)", "(GRID ? 32 : 0)"]:
        assert needle in body, needle
    for name, value in [("SLAB_NT", 256), ("SLAB_NR", 4), ("SLAB_NH", 2), ("MAXV", 8)]:
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name
    assert "return ((size_t)3 * slab_slot(S, V) + (cache ? (size_t)2 * S * S * 3 : 0)) * sizeof(double);" in src
    assert "return (S * S * V + 2) & ~1;" in src

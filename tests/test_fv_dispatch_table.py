"""tests/fv_cases.py reaches every branch of `fv_dispatch` (exahype_amd/csrc/fv_rusanov.hip) in corrected mode: fv_cases.branch() restates the
dispatch conditions, every row names the branch it reaches, every branch has a row, and the thresholds branch() assumes are the ones the
source states -- a later change of a threshold turns this red instead of silently moving a case.  The thresholds are matched as literal source
lines, so a pure reformat of fv_dispatch turns the last test red too: it fails closed -- whoever reformats the dispatch confirms the thresholds
and updates the needles.

tests/fv_user_cases.py does the same for the kernels as they are instantiated for generated term sets: its branch() carries the two properties
of the term set (terms that see position / time, an ncp) that close the plane-streaming kernel."""
import os
import re

import numpy as np

from tests import fv_cases as K
from tests import fv_user_cases as U

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


def test_every_user_row_reaches_the_branch_it_names():
    for row in U.ROWS:
        assert U.branch_of(row) == row[0], U.row_id(row)
        assert row[0] in U.BRANCHES


def test_every_branch_a_generated_term_set_reaches_has_a_row():
    assert {U.branch_of(row) for row in U.ROWS} == set(U.BRANCHES)
    # a generated term set has no cached scalars on the FV path and its ring stays under 64 KiB: of fv_cases' branches, all but those two kinds
    assert {b.replace("slab-generic", "slab").replace("slab-fitnv", "slab") for b in K.BRANCHES if "cache" not in b} == set(U.BRANCHES)
    entries = {r[7].split(":")[0] + (":" + r[7].split(":")[1] if ":" in r[7] else "") for r in U.ROWS}
    assert entries == {"inplace", "inplace-origin", "slot", "oop", "grid:periodic", "grid:dirichlet"}
    # the rows the plane-streaming kernel refuses at run time: 3-D patches of more than 1024 volumes with position / time terms, and with an ncp alone
    big = [r for r in U.ROWS if r[2] == 3 and r[3] ** 3 > 1024 and r[0] == "cpt4"]
    assert {r[1] for r in big} == {U.CR, U.TL} and {r[7].split(":")[0] for r in big if r[1] == U.CR} == {"inplace", "slot", "oop", "grid"}
    for r in big:                                                   # ... and the same shapes WOULD stream planes without those terms
        if r[7] != "oop":
            assert U.branch(r[2], r[3], r[4], U.n_real(r), r[5], r[6], False, False, r[7]) == "slab", U.row_id(r)
    # every row of a term set that sees position / time hands distinct non-zero centres and t != 0 over, but the one in-place default
    for r in U.ROWS:
        c, t = U.coordinates(r)
        if U.term_set(r[1]).uses_xt and r[7] != "inplace-origin":
            assert t != 0 and np.all(c != 0) and len({tuple(x) for x in c}) == len(c) == r[6], U.row_id(r)
        else:
            assert c is None and t == 0
    assert sum(r[7] == "inplace-origin" for r in U.ROWS) == 1
    # no bare grid path (no LDS copy: the neighbour patch is read across the face) without a row that has an ncp and position terms
    assert any(U.is_grid(r) and r[0] in ("unstaged", "nt1024-unstaged", "cpt4") and r[1] == U.CR for r in U.ROWS)


def test_thresholds_are_the_ones_the_source_states():
    src = open(SRC).read()
    body = src[src.index("static int fv_dispatch("):src.index("static int fv_mode(")]
    for needle in ["if (ncell <= 256) {", "const int ppb = (int)(256 / ncell);", "n_patches >= (long)ppb * 2048",
                   "if (DIM == 2 && P == 4 && H == 1 && m == 5 && V == 10) {", "lds <= 64 * 1024", "} else if (ncell <= 1024) {",
                   "DIM == 3 && P * P <= 256 && S * S * V <= 2 * SLAB_NR * SLAB_NT", "!pde_has_xt<PDE>::value && !pde_has_ncp<PDE>::value",
                   "(!cd.out || GRID) && (!GRID || 4 * H * P * V <= SLAB_NH * SLAB_NT)",
                   "if (lds > 64 * 1024) {", "} else if (ncell <= 4096) {", "(GRID ? (size_t)ppb * 32 : 0)", "(GRID ? 32 : 0)"]:
        assert needle in body, needle
    for name, value in [("SLAB_NT", 256), ("SLAB_NR", 4), ("SLAB_NH", 2), ("MAXV", 8)]:
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name
    assert "return ((size_t)3 * slab_slot(S, V) + (cache ? (size_t)2 * S * S * 3 : 0)) * sizeof(double);" in src
    assert "return (S * S * V + 2) & ~1;" in src

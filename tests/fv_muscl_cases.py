"""The case table of the MUSCL-Hancock patch kernels (exahype_amd/csrc/exa_fv_muscl.hpp, mode FV_MUSCL_HANCOCK), shared by the CPU check of
the measure (tests/test_fv_muscl_reference.py) and the GPU tests (tests/test_fv_muscl_kernels.py).

A row is (dim, P, H, n_real, n_aux, n_patches, pde, note).  What the rows reach in the kernel's LDS plan (fv_muscl_plan, exa_launch.hpp: per
patch 8 ((P + 4)^dim V + (P + 2)^dim n_real) bytes; plans up to 32 KiB share a 256-thread workgroup):

  2-D P = 1          1 000 + 360 B: 48 patches per workgroup (the LDS cap, not the thread count, sets it), 11 patches: one ragged workgroup
  2-D P = 4, V = 5   4 000 B: 16 patches per workgroup, 37 patches: three workgroups, the last one with 5
  2-D P = 4, V = 10  6 560 B: 9 patches per workgroup (144 of 256 threads have a volume)
  2-D P = 3, H = 3   the window is cut out of the patch row by row (H > 2); only the inner two layers count
  2-D P = 8          9 760 B: 4 patches per workgroup, 9 patches
  2-D P = 20, V = 10 65 440 B: one patch per workgroup, just below 64 KiB ... with the 5 + 5 variables of the reference's shape
  2-D P = 32         98 080 B: above 64 KiB (hipFuncSetAttribute) and above 80 KiB (512 threads), two volumes per thread
  3-D P = 2          8 640 + 2 560 B: 5 patches per workgroup
  3-D P = 4          29 120 B: 2 patches per workgroup, 6 patches
  3-D P = 8, V = 6   122 944 B: one patch per CU, two volumes per thread
  advection          n_real = 5 of its 8 variables, all 8, and 1 + 4 auxiliary

Euler rows run all five state families of tests/fv_cases.py, advection rows `benign`; every row runs in place, with slot (SLOT_PATTERN) and out
of place.  The step is the one a run takes at CFL 0.5 (dt = 0.5 h / (dim lambda_max)), h = 0.1.
"""
import numpy as np

from oracle import fv_reference as R
from tests import fv_cases as K

E, A = R.PDE_EULER, R.PDE_ADVECTION
FAMILIES = K.FAMILIES
ENTRIES = ("inplace", "slot", "oop")
H_VOLUME = K.H_VOLUME
CFL = 0.5

ROWS = [
    (2, 1, 2, 5, 0, 11, E, ""),
    (2, 4, 2, 5, 0, 37, E, "ragged last workgroup"),
    (2, 4, 2, 5, 5, 37, E, ""),
    (2, 3, 3, 5, 1, 5, E, "H > 2: only the inner two layers count"),
    (2, 8, 2, 5, 0, 9, E, ""),
    (2, 20, 2, 5, 5, 2, E, "crosses 64 KB of LDS"),
    (2, 32, 2, 5, 0, 2, E, "more volumes than threads"),
    (3, 2, 2, 5, 0, 5, E, ""),
    (3, 4, 2, 5, 0, 6, E, ""),
    (3, 8, 2, 5, 1, 2, E, ""),
    (2, 6, 2, 5, 1, 4, A, ""),
    (3, 5, 2, 8, 0, 2, A, ""),
    (2, 7, 2, 1, 4, 3, A, ""),
]
# the rows the CPU module evaluates the mutants on (small ones: a mutant needs one row it leaves the bound on)
CPU_MUTANT_ROWS = [r for r in ROWS if r[1] <= 8 and r[2] <= 3 and not (r[0] == 3 and r[1] == 8)]


def row_id(row):
    return "%dd-P%d-H%d-%d+%d-n%d-%s" % (row[0], row[1], row[2], row[3], row[4], row[5], "euler" if row[6] == E else "adv")


def families(row):
    return FAMILIES if row[6] == E else ("benign",)


def row_state(row, family):
    dim, P, H, n_real, n_aux, n, pde, _ = row
    seed = 300 * dim + P + 7 * H + K.FAMILIES.index(family)
    if pde == A and n_real < 5:                                   # a state of its own: the Euler families fill variables 0 .. 4
        return np.random.default_rng(seed).uniform(-1, 1, (n,) + (P + 2 * H,) * dim + (n_real + n_aux,))
    return K.state(family, n, dim, P, H, n_real + n_aux, seed)


def cfl_step(Q, dim, pde):
    """(dt, h): the step a run takes at CFL 0.5 on these states"""
    lam = 1.0 if pde == A else max(float(np.max(R.max_eigenvalue(Q, d, pde))) for d in range(dim))
    return float(CFL * H_VOLUME / (dim * lam)), H_VOLUME


def lds_plan(dim, P, n_real, V):
    """fv_muscl_plan (exa_launch.hpp) restated: (patches per workgroup, threads, LDS bytes); None where one patch does not fit 160 KiB"""
    per = 8 * ((P + 4) ** dim * V + (P + 2) ** dim * n_real)
    if per > 160 * 1024:
        return None
    ppb, ncell = 1, P ** dim
    if ncell <= 256 and 2 * per <= 64 * 1024:
        ppb = min(256 // ncell, 64 * 1024 // per)
    return ppb, (512 if dim == 2 and per > 80 * 1024 else 256), per * ppb

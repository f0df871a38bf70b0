"""Generated term sets of 4, 6, 7 and 8 variables, and the ADER-DG case tables built on them: shared by the CPU checks
(tests/test_dg_wide_reference.py) and the GPU parity tests (tests/test_dg_wide_sets.py).

Which stage-A kernel serves a term set depends on its variable count NV, its cached scalars NAUX and its source (dg_inst.hip stage_a_kind);
every other ADER-DG case of the suite has 1, 2, 3 or 5 variables.  The "ring" family couples every variable to two others with a coefficient
of its own per variable and per direction, so a swapped variable or direction index moves the result:

    F_d[v] = a_d (1 + v / 10) q_v + (1 / 5) q_{(v + 1) % NV} q_{(v + 2 + d) % NV} / den,     a = (1, -1/2, 3/4)

with the eigenvalue bound 2 + (2 / 5) mean_v |q_v| (states are 1 + 0.3 * random: |dF/dq| stays below it).  Exactly four sets are compiled:

    ring4    4 variables, den = 1
    ring6r   6 variables, den = q_0      (the generator caches 1 / q_0: NAUX = 1)
    ring7s   7 variables, den = 1,  source S_v = q_{(v + 3) % NV} / 2 - q_v
    ring8    8 variables, den = 1

The reference is oracle/aderdg_numpy.py on tests/test_user_pde.py's NumpyPDE (the same expressions, lambdified); tests/test_dg_wide_reference.py
pins it against long double.  Every case runs one step at the CFL-0.9 step and three steps at tests/dg_cases.py steps_dt (CFL 0.6; the single-stage
scheme, n_picard = 0, at its CFL 0.3 as everywhere in the suite: forward Euler in time amplifies rounding differences at 0.6).
"""
import functools

import numpy as np
import sympy

from tests.dg_cases import n_it_of, steps_dt
from tests.util import cfl_dt

A_DIR = (sympy.Integer(1), sympy.Rational(-1, 2), sympy.Rational(3, 4))
SETS = {"ring4": (4, False, False), "ring6r": (6, True, False), "ring7s": (7, False, True), "ring8": (8, False, False)}     # NV, den = q_0, source


def ring_flux(nv, over_q0, swap=None):
    def flux(q, d):
        den = q[0] if over_q0 else 1
        f = [A_DIR[d] * (1 + sympy.Rational(v, 10)) * q[v] + sympy.Rational(1, 5) * q[(v + 1) % nv] * q[(v + 2 + d) % nv] / den for v in range(nv)]
        if swap is not None:
            f[swap[0]], f[swap[1]] = f[swap[1]], f[swap[0]]
        return f
    return flux


@functools.lru_cache(maxsize=None)
def ring(name, swap=None):
    """The SympyPDE of one of the four sets (swap=(i, j): its flux with the components i and j exchanged -- never compiled, the sensitivity
    check's oracle only)."""
    from exahype_amd.pde_codegen import SympyPDE
    nv, over_q0, with_source = SETS[name]
    eig = lambda q, d: 2 + sympy.Rational(2, 5) * sum(sympy.Abs(x) for x in q) / nv
    source = (lambda q: [q[(v + 3) % nv] / 2 - q[v] for v in range(nv)]) if with_source else None
    return SympyPDE(nv, flux=ring_flux(nv, over_q0, swap), max_eigenvalue=eig, source=source, max_dim=3,
                    name=name if swap is None else "%s_swap%d%d" % ((name,) + tuple(swap)))


@functools.lru_cache(maxsize=None)
def numpy_pde(name, swap=None):
    from tests.test_user_pde import NumpyPDE
    return NumpyPDE(ring(name, swap))


# ---- case tables: (set, N, nc, n_picards, stage-A family for n_picard != 0, three-step run) ---------------------------------------------------
# family: the substring of AderDgSolver.stage_a_kernel_name() for a Picard loop; n_picard = 0 takes the single-stage kernel where the LDS kernel
# serves the order and the streamed one where it does not (family_of).  The three-step run is dropped (False) only where a row cannot see its last
# Picard iteration after three steps (tests/test_dg_wide_reference.py measures every row): its one-step comparison stays.
ALL_PICARD = (-1, 0, 2)
LDS, STREAM, REG, M8 = "dg_stage_a_kernel<", "dg_stage_a_stream_kernel<", "dg_stage_a_reg_kernel<", "dg_stage_a_m8_kernel<"
SINGLE = "dg_stage_a_single_kernel<"
ROWS_3D = [
    ("ring8", 2, (2, 2, 2), ALL_PICARD, LDS, True),            # cpb 16
    ("ring8", 3, (2, 2, 2), ALL_PICARD, STREAM, True),
    ("ring8", 3, (1, 1, 1), ALL_PICARD, STREAM, True),          # its own neighbour everywhere
    ("ring8", 4, (2, 1, 2), ALL_PICARD, STREAM, True),
    ("ring8", 5, (1, 2, 2), ALL_PICARD, STREAM, True),
    ("ring8", 6, (1, 1, 2), ALL_PICARD, STREAM, True),
    ("ring8", 7, (1, 1, 1), ALL_PICARD, STREAM, True),
    ("ring8", 3, (9, 8, 8), (-1,), STREAM, False),              # 576 cells > the persistent grid of 256 workgroups: its second pass (one step only)
    ("ring6r", 4, (2, 2, 1), ALL_PICARD, LDS, True),
    ("ring6r", 5, (2, 1, 2), ALL_PICARD, STREAM, True),         # streamed kernel with a cached scalar
    ("ring6r", 6, (1, 2, 1), ALL_PICARD, STREAM, True),
    ("ring6r", 7, (1, 1, 2), ALL_PICARD, STREAM, True),
    ("ring7s", 3, (2, 2, 1), ALL_PICARD, None, True),           # (families of ring7s and of ring4 at N = 5, 7, 8: WIDE_FAMILY below, read from the selector)
    ("ring7s", 5, (1, 2, 1), ALL_PICARD, None, True),
    ("ring7s", 6, (2, 1, 1), ALL_PICARD, None, True),
    ("ring4", 6, (2, 2, 2), ALL_PICARD, REG, True),
    ("ring4", 5, (2, 1, 2), ALL_PICARD, None, True),
    ("ring4", 7, (1, 2, 1), ALL_PICARD, None, True),
    ("ring4", 8, (1, 1, 2), ALL_PICARD + (6,), None, True),     # (6: see NO_MUTANT)
]
# The one case whose last Picard iteration lies under the visibility bound of assert_dg_parity (100 * DG_TOL = 1e-9 of the increment): the ring
# flux is weakly nonlinear, and at N = 8 the eighth iteration moves one CFL-0.9 step by 7.0e-10 (2.5e-10 to 1.2e-9 over eight other seeds), three
# CFL-0.6 steps by 1.8e-11.  The case stays and is held to DG_TOL without a mutant; the row runs n_picard = 6 as well -- the iteration count is a
# run-time argument of the same kernel -- whose mutant is 8.3e-7 (one step) and 4.0e-8 (three steps).
NO_MUTANT = {("ring4", 3, 8, -1)}
ROWS_2D = [
    ("ring8", 7, (2, 2), ALL_PICARD, LDS, True),
    ("ring8", 4, (3, 2), ALL_PICARD, LDS, True),
    ("ring6r", 5, (3, 2), ALL_PICARD, LDS, True),
    ("ring7s", 6, (2, 3), ALL_PICARD, LDS, True),
]
FUSED_ROWS = [("ring8", 3, (5, 3)), ("ring8", 7, (2, 3)), ("ring6r", 4, (7, 4))]         # 2-D, n_picard = 0, fused_single_stage
SWAP_ROWS = [("ring8", 3, (2, 2, 2)), ("ring6r", 5, (2, 1, 2)), ("ring7s", 5, (1, 2, 1)), ("ring4", 7, (1, 2, 1))]     # one streamed row per set
REFUSED = [("ring8", 3, 8), ("ring6r", 3, 8), ("ring8", 2, 8), ("ring6r", 2, 8)]         # (set, dim, N): no stage-A kernel
BOUNDARY_ROW = ("ring8", 3, (3, 2, 2))
# rows whose family the issue left to the selector's output (tests/golden/stage_a_selection_wide.txt; pinned by test_dg_wide_reference.py)
WIDE_FAMILY = {("ring7s", 3): LDS, ("ring7s", 5): STREAM, ("ring7s", 6): STREAM, ("ring4", 5): LDS, ("ring4", 7): STREAM, ("ring4", 8): M8}


def all_rows():
    return [(3,) + r for r in ROWS_3D] + [(2,) + r for r in ROWS_2D]


def family_of(name, dim, N, n_picard, family):
    family = family or WIDE_FAMILY[(name, N)]
    if n_picard == 0:
        return SINGLE if family in (LDS, REG) else STREAM          # (m8 serves a Picard loop only: the single-stage scheme streams)
    return family


def wide_input(name, dim, N, nc):
    """u, dx, the CFL-0.9 step"""
    nv = SETS[name][0]
    rng = np.random.default_rng(1000 * nv + 100 * dim + 10 * N + sum(nc))
    u = 1.0 + 0.3 * rng.random(tuple(nc) + (N,) * dim + (nv,))
    dx = [(0.9, 1.1, 0.7)[a] / nc[a] for a in range(dim)]
    return u, dx, cfl_dt(u, dx, dim, N, pde=numpy_pde(name), m=nv)


@functools.lru_cache(maxsize=None)
def reference(name, dim, N, nc, n_it, steps, swap=None, single_stage=False):
    """u after `steps` steps of oracle/aderdg_numpy.py (1: the CFL-0.9 step; 3: steps_dt).  n_it = 0 with single_stage: step_single_stage, what the
    kernels of n_picard = 0 restate; computed once per case and shared (read-only)."""
    from oracle import aderdg_numpy as A
    from oracle.dg_operators import operators
    u, dx, dt = wide_input(name, dim, N, nc)
    if steps > 1:
        dt = steps_dt(dt, single_stage=single_stage)
    pde, ops = numpy_pde(name, swap), operators(N)
    for _ in range(steps):
        u = A.step_single_stage(u, dt, dx, ops, pde) if single_stage else A.step(u, dt, dx, ops, pde, n_it=n_it)
    u.setflags(write=False)
    return u


def want_and_mutant(name, dim, N, nc, n_picard, steps):
    """(oracle result, the same with one Picard iteration less or None for the single-stage scheme)"""
    n_it = n_it_of(N, n_picard)
    if n_it == 0:
        return reference(name, dim, N, nc, 0, steps, single_stage=True), None
    return reference(name, dim, N, nc, n_it, steps), None if (name, dim, N, n_picard) in NO_MUTANT else reference(name, dim, N, nc, n_it - 1, steps)

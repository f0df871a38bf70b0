"""The grid cases of the one-launch MUSCL-Hancock step (exa_fv_grid_step_muscl_device, FVPatchGrid(fused=FUSED_EDGES)), shared by the CPU check
of the inputs (tests/test_fv_muscl_grid_one_launch_host.py) and the GPU tests (tests/test_fv_muscl_grid_one_launch.py).

A case is (dim, grid, P, n_real, n_aux, term set, faces); what each reaches in fv_muscl_grid_kernel (plan: fv_muscl_plan, tests/fv_muscl_cases.py):

  2d-P4-5x3-periodic        15 patches in one ragged workgroup (16 patches per workgroup)
  2d-P4-6x7-periodic        three workgroups, neighbours in other workgroups, ragged tail
  2d-P4-1x7-periodic-aux    extent 1 (face and diagonal neighbour are the patch itself or its row), 5 + 5 variables
  2d-P2-2x2-periodic        the smallest patch; both neighbours of an axis are the same patch
  2d-P4-3x2-wall-outflow-dirichlet   corners where two different rules compose
  2d-P4-3x2-periodic0-wall-dirichlet mirror / state composed with a periodic diagonal
  3d-P4-2x3x2-states        12 edge lines, 2 patches per workgroup, every face a prescribed state (BLIND_TO_ITS_CORNERS: not on the GPU list)
  3d-P2-3x1x2-periodic      5 patches per workgroup, extent 1 in 3-D
  3d-P4-2x2x2-mixed         wall, outflow, Dirichlet and periodic faces over the three axes
  3d-P8-1x2x1-periodic      122 944 B plan, two volumes per thread
  2d-P20-2x1-periodic       plan just below 64 KiB
  2d-P32-1x2-periodic       512-thread plan, above 64 KiB of LDS
  adv-2d-P7-2x2-periodic    n_real = 1 of the advection's variables, 4 auxiliary ones
  swe-2d-P4-3x2-periodic    generated shallow water (muscl_hancock=True): the side library's grid launcher

Faces: None (periodic), "states" (every face a prescribed state of the family: the all-faces form of FVPatchGrid) or {(axis, side): "wall" |
"outflow" | "dirichlet"} (a face that is not named is periodic).  The step is the one a run takes at CFL 0.5, h = 0.1.
"""
import collections
import functools

import numpy as np

from oracle import fv_reference as R
from tests import fv_cases as K1
from tests import fv_muscl_cases as K

FAMILIES = ("benign", "riemann")
W, O, D = "wall", "outflow", "dirichlet"
CASES = {
    "2d-P4-5x3-periodic": (2, (5, 3), 4, 5, 0, "euler", None),
    "2d-P4-6x7-periodic": (2, (6, 7), 4, 5, 0, "euler", None),
    "2d-P4-1x7-periodic-aux": (2, (1, 7), 4, 5, 5, "euler", None),
    "2d-P2-2x2-periodic": (2, (2, 2), 2, 5, 0, "euler", None),
    "2d-P4-3x2-wall-outflow-dirichlet": (2, (3, 2), 4, 5, 1, "euler", {(0, 0): W, (0, 1): O, (1, 0): D, (1, 1): W}),
    "2d-P4-3x2-periodic0-wall-dirichlet": (2, (3, 2), 4, 5, 1, "euler", {(1, 0): W, (1, 1): D}),
    "3d-P4-2x3x2-states": (3, (2, 3, 2), 4, 5, 0, "euler", "states"),
    "3d-P2-3x1x2-periodic": (3, (3, 1, 2), 2, 5, 0, "euler", None),
    "3d-P4-2x2x2-mixed": (3, (2, 2, 2), 4, 5, 1, "euler", {(0, 0): W, (0, 1): O, (1, 0): D, (1, 1): W}),
    "3d-P8-1x2x1-periodic": (3, (1, 2, 1), 8, 5, 1, "euler", None),
    "2d-P20-2x1-periodic": (2, (2, 1), 20, 5, 5, "euler", None),
    "2d-P32-1x2-periodic": (2, (1, 2), 32, 5, 0, "euler", None),
    "adv-2d-P7-2x2-periodic": (2, (2, 2), 7, 1, 4, "adv", None),
    "swe-2d-P4-3x2-periodic": (2, (3, 2), 4, 3, 0, "swe", None),
}
# Not on the GPU list: beyond two prescribed-state faces the slopes of the ghost volumes next to a domain corner vanish whatever the edge entry holds
# (one of the two differences is state - state = 0), so the restatement on the global array cannot tell a wrong edge entry from a right one
# (tests/test_fv_muscl_grid_one_launch_host.py).  The GPU module still runs it, as the test of the all-faces-prescribed form of FVPatchGrid.
BLIND_TO_ITS_CORNERS = ("3d-P4-2x3x2-states",)
GPU_CASES = tuple(sorted(c for c in CASES if c not in BLIND_TO_ITS_CORNERS))
Setup = collections.namedtuple("Setup", "dim grid P n_real n_aux terms_name U dt h boundary conditions ref_boundary pde terms periodic")


@functools.lru_cache(maxsize=None)
def flagged(name):
    """the term set tests/user_term_sets.py defines under `name`, with the keyword muscl_hancock=True"""
    from exahype_amd.pde_codegen import SympyPDE
    from tests import user_term_sets as T
    base = getattr(T, name)()
    sub = lambda e, qq: e.subs(dict(zip(base.q, qq)), simultaneous=True)     # noqa: E731
    return SympyPDE(base.n_vars, flux=lambda qq, d: [sub(e, qq) for e in base.flux_exprs[d]], max_eigenvalue=lambda qq, d: sub(base.eig_exprs[d], qq),
                    max_dim=base.max_dim, name=base.name + "_muscl", muscl_hancock=True)


def _states(dim, V, family, seed, n):
    return K1.state(family, n, dim, 1, 0, V, seed).reshape(n, V)


def _advection_state(family, grid, dim, P, V, seed):
    rng = np.random.default_rng(seed)
    U = rng.uniform(-1, 1, grid + (P,) * dim + (V,))
    if family == "riemann":                                       # a jump in the middle of the domain along axis 0, noise 1e-3
        G = R.assemble(U, dim)
        x = np.indices(G.shape[:dim])[0]
        G[..., 0] = np.where(x < G.shape[0] // 2, 1.0, 0.125) + 1e-3 * G[..., 0]
        U = np.ascontiguousarray(R.cut_patches(G, dim, grid, P))
    return U


def setup(case, family):
    """-> Setup: the input U [g.., P.., V], the step (dt, h), `boundary` as FVPatchGrid takes it, `conditions` / `ref_boundary` as
    tests/fv_muscl_ref.py grid_update takes them, the restatement's term set (pde, terms)"""
    from exahype_amd import boundary as B
    dim, grid, P, n_real, n_aux, name, faces = CASES[case]
    V, n = n_real + n_aux, int(np.prod(grid))
    shape = grid + (P,) * dim + (V,)
    h = K.H_VOLUME
    boundary = conditions = ref_boundary = extra = terms = None
    pde = R.PDE_EULER
    if name == "adv":
        pde = R.PDE_ADVECTION
        # (one variable of uniform noise: the minmod slopes next to a domain corner are zero for one seed in three, whatever the edge entry holds;
        # 62 is a seed at which the host module's check of the inputs passes)
        U = _advection_state(family, grid, dim, P, V, 62 + FAMILIES.index(family))
        lam = 1.0
    elif name == "swe":
        from tests import fv_user_cases as KU
        terms = R.UserTerms(flagged("swe"))
        U = KU.state(KU.SW, family, n, dim, P, 0, V, 500 + P).reshape(shape)
        lam = float(np.max(np.abs(U[..., 1:3] / U[..., :1]) + np.sqrt(9.81 * U[..., :1])))          # |u_n| + sqrt(g h)
    else:
        U = K1.state(family, n, dim, P, 0, V, 41 + dim).reshape(shape)
        if faces == "states":
            extra = _states(dim, V, family, 977, 2 * dim)
            boundary = ref_boundary = {(a, s): extra[2 * a + s] for a in range(dim) for s in range(2)}
        elif faces is not None:
            extra = _states(dim, V, family, 978, 1)
            boundary = {k: {W: B.Wall(), O: B.Outflow(), D: B.Dirichlet(extra[0])}[v] for k, v in faces.items()}
            conditions = B.fv_faces(boundary, dim, n_real, n_aux, 1)[2]
        lam = max(float(np.max(R.max_eigenvalue(np.concatenate([U.reshape(-1, V)] + ([extra] if extra is not None else [])), d, R.PDE_EULER))) for d in range(dim))
    dt = K.CFL * h / (dim * lam)
    return Setup(dim, grid, P, n_real, n_aux, name, U, dt, h, boundary, conditions, ref_boundary, pde, terms, faces is None)


def reference(s, h=None):
    """the long-double restatement of one step on the assembled global array -> Result(new, M, E) in patch form"""
    from tests import fv_muscl_ref as M
    return M.grid_update(s.U, s.dt, s.h if h is None else h, s.dim, s.n_real, s.pde, terms=s.terms, boundary=s.ref_boundary, conditions=s.conditions)

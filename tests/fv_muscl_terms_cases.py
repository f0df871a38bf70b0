"""The case table of the MUSCL-Hancock kernels for term sets with a source and / or a non-conservative product (SympyPDE(muscl_hancock=True,
muscl_terms=True)), shared by the CPU check of the measure (tests/test_fv_muscl_terms_reference.py) and the GPU tests
(tests/test_fv_muscl_terms_kernels.py).

Three term sets, each built from the expressions of tests/user_term_sets.py the way tests/fv_muscl_grid_cases.flagged does it:

    euler_gravity    Euler with a constant body force: a source, S = (0, rho g, m . g)
    two_layer_like   two_layer_like(3): a flux and an ncp whose matrix sees the state
    coupled_state    the expressions of coupled_rational(3) at x = 0, t = 0: flux, source and ncp together

States: the families "benign" and "riemann" of tests/fv_user_cases.state.  The step is the one a run takes at CFL 0.5, h = 0.1.

PATCH_ROWS (set, dim, P, H, n_aux, n_patches, entries), the smallest shapes that still reach each code path:

    euler_gravity  2-D P = 4 H = 2, 7 patches      in place, masked (SLOT_PATTERN), out of place
    euler_gravity  2-D P = 4 H = 3 + 2 aux, 5      in place: the H > 2 staging, auxiliary values bit-unchanged
    euler_gravity  3-D P = 3 H = 2, 3              in place
    two_layer_like 2-D P = 5 H = 2, 5              in place, out of place
    two_layer_like 3-D P = 2 H = 2 + 1 aux, 4      masked
    coupled_state  2-D P = 4 H = 2, 6              in place
    coupled_state  3-D P = 4 H = 2, 2              in place

GRID_ROWS (set, dim, P, n_aux, grid, faces, forms): coupled_state 2-D 3 x 2 periodic (FUSED_EDGES and fused=False), two_layer_like 3-D 3 x 1 x 2
periodic (FUSED_EDGES), euler_gravity 2-D 3 x 2 + 1 aux with wall / outflow / Dirichlet / wall faces (FUSED_EDGES).
"""
import collections
import functools

import numpy as np

from oracle import fv_reference as R
from tests import fv_cases as K1
from tests import fv_user_cases as KU

FAMILIES = ("benign", "riemann")
H_VOLUME = K1.H_VOLUME
CFL = 0.5
SLOT_PATTERN = K1.SLOT_PATTERN
EG, TL, CS = "euler_gravity", "two_layer_like", "coupled_state"
SETS = (EG, TL, CS)
W, O, D = "wall", "outflow", "dirichlet"

PATCH_ROWS = [
    (EG, 2, 4, 2, 0, 7, ("inplace", "slot", "oop")),
    (EG, 2, 4, 3, 2, 5, ("inplace",)),
    (EG, 3, 3, 2, 0, 3, ("inplace",)),
    (TL, 2, 5, 2, 0, 5, ("inplace", "oop")),
    (TL, 3, 2, 2, 1, 4, ("slot",)),
    (CS, 2, 4, 2, 0, 6, ("inplace",)),
    (CS, 3, 4, 2, 0, 2, ("inplace",)),
]
GRID_ROWS = [
    (CS, 2, 4, 0, (3, 2), None, ("edges", "two-pass")),
    (TL, 3, 2, 0, (3, 1, 2), None, ("edges",)),
    (EG, 2, 4, 1, (3, 2), {(0, 0): W, (0, 1): O, (1, 0): D, (1, 1): W}, ("edges",)),
]
GridSetup = collections.namedtuple("GridSetup", "U dt h boundary conditions")


def _base(name):
    from tests import user_term_sets as T
    return {EG: T.euler_gravity, TL: lambda: T.two_layer_like(3), CS: lambda: T.coupled_rational(3)}[name]()


@functools.lru_cache(maxsize=None)
def flagged(name):
    """the term set with the keywords muscl_hancock=True, muscl_terms=True (coupled_state: coupled_rational(3) at x = 0, t = 0)"""
    from exahype_amd.pde_codegen import SympyPDE
    base = _base(name)
    at0 = {s: 0 for s in base.x + [base.t]}

    def sub(e, qq, dq=None):
        m = dict(zip(base.q, qq))
        if dq is not None:
            m.update(zip(base.dq, dq))
        return e.subs(at0).subs(m, simultaneous=True)
    kw = {}
    if base.source_exprs is not None:
        kw["source"] = lambda qq: [sub(e, qq) for e in base.source_exprs]
    if base.ncp_exprs is not None:
        kw["ncp"] = lambda qq, dq, d: [sub(e, qq, dq) for e in base.ncp_exprs[d]]
    return SympyPDE(base.n_vars, flux=lambda qq, d: [sub(e, qq) for e in base.flux_exprs[d]], max_eigenvalue=lambda qq, d: sub(base.eig_exprs[d], qq),
                    max_dim=base.max_dim, name=name + "_muscl_terms", muscl_hancock=True, muscl_terms=True, **kw)


@functools.lru_cache(maxsize=None)
def terms(name):
    return R.UserTerms(flagged(name))


def n_real(name):
    return flagged(name).n_vars


def _state_name(name):
    return KU.CR if name == CS else name


def state(name, family, n, dim, P, H, V, seed):
    """Q [n, S.., V] (H = 0: halo-less) of the family, as tests/fv_user_cases.state builds it"""
    return KU.state(_state_name(name), family, n, dim, P, H, V, seed)


def patch_id(row):
    return "%s-%dd-P%d-H%d-%d+%d-n%d" % (row[0], row[1], row[2], row[3], n_real(row[0]), row[4], row[5])


def grid_id(row):
    return "%s-%dd-P%d-%s-%s" % (row[0], row[1], row[2], "x".join(str(g) for g in row[4]), "periodic" if row[5] is None else "bounded")


def lam_max(name, dim, q):
    """long-double maximum of the eigenvalue over the states q [..., V]"""
    return max(float(np.max(R.user_max_eigenvalue(terms(name), q, d))) for d in range(dim))


def patch_state(row, family):
    name, dim, P, H, n_aux, n, _ = row
    return state(name, family, n, dim, P, H, n_real(name) + n_aux, 700 * dim + P + 7 * H + FAMILIES.index(family))


def cfl_step(name, dim, q):
    return float(CFL * H_VOLUME / (dim * lam_max(name, dim, q))), H_VOLUME


def slot_of(n):
    return K1.slot_of(n)


def grid_setup(row, family):
    """-> GridSetup: U [g.., P.., V], the step, `boundary` as FVPatchGrid takes it and `conditions` as the restatement's grid_update takes them"""
    from exahype_amd import boundary as B
    name, dim, P, n_aux, grid, faces, _ = row
    m = n_real(name)
    V, n = m + n_aux, int(np.prod(grid))
    U = state(name, family, n, dim, P, 0, V, 900 + dim + FAMILIES.index(family)).reshape(grid + (P,) * dim + (V,))
    extra = boundary = conditions = None
    if faces is not None:
        extra = state(name, family, 1, dim, 1, 0, V, 978).reshape(1, V)
        def wall(axis):                                              # (a generated set names its reflection: Euler's, -1 on the normal momentum)
            s = np.ones(m)
            s[1 + axis] = -1.0
            return B.Wall(s)
        boundary = {k: wall(k[0]) if v == W else (B.Outflow() if v == O else B.Dirichlet(extra[0])) for k, v in faces.items()}
        conditions = B.fv_faces(boundary, dim, m, n_aux, 100)[2]
    q = U.reshape(-1, V) if extra is None else np.concatenate([U.reshape(-1, V), extra])
    dt, h = cfl_step(name, dim, q)
    return GridSetup(U, dt, h, boundary, conditions)

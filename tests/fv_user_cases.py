"""The case table of the corrected FV Rusanov kernels as they are instantiated for GENERATED term sets (the side library of a SympyPDE:
`fv_dispatch<DIM, exa::UserPDE, ..>`), shared by the CPU check of the measure (tests/test_fv_user_reference.py), the dispatch check
(tests/test_fv_dispatch_table.py) and the GPU tests (tests/test_fv_user_kernels_hp.py).  The sibling of tests/fv_cases.py, which does the same for
the built-in term sets.

A row is (branch, term set, dim, P, H, n_aux, n_patches, entry); n_real is the term set's number of variables.  `branch` is the branch of
`fv_dispatch` the row reaches, restated by branch() below with the two properties of the term set that close the plane-streaming kernel
(`!pde_has_xt<PDE>::value && !pde_has_ncp<PDE>::value`): a 3-D patch of more than 1024 volumes whose term set sees position / time or carries an
ncp goes to the four-volumes-per-thread kernel.  A generated term set has no cached scalars in the FV path (no `fv_aux`), so its plane-streaming
kernel is the non-cached one ("slab"; n_real = NV, the form with compile-time variable count) and its ring never exceeds 64 KiB
(S^2 V <= 2048: at most 49 KB).  With V = n_real + n_aux, S = P + 2 H, ncell = P^dim, pvol = S^dim:

    ref               euler_gravity 2-D P = 4, H = 1, 5 + 5 variables: the compile-time shape
    ref-persistent    ... with 16 * 2048 + 37 patches (benign family only: one launch of 32 805 patches)
    staged            swe 2-D P = 8; coupled_rational 3-D P = 4 with 1 aux; coupled_rational 2-D P = 4 (3 + 0 variables: not the compile-time shape)
    unstaged          coupled_rational 3-D P = 6, H = 2 with 6 aux (V = 9: 72 000 B)
    nt1024-staged     coupled_rational 2-D P = 20; two_layer_like 3-D P = 9
    nt1024-unstaged   coupled_rational 3-D P = 10, H = 2 (2 744 * 3 * 8 = 65 856 B > 64 KiB)
    slab              euler_gravity 3-D 15^3 and 13^3 with 2 aux (a source, no position / time, no ncp)
    cpt4              coupled_rational 3-D 15^3 and two_layer_like 3-D 15^3 (the rows the plane-streaming kernel refuses: the limiter's patch at
                      p = 7); swe 2-D P = 40

Entries: "inplace" (time_step; a term set that sees position / time gets distinct non-zero patch centres and t = T0), "inplace-origin" (the
in-place default: every patch at the origin, t = 0), "slot" (the masked call; with centres: exa_fv_time_step_device_masked_at), "oop"
(time_step_oop), "grid:<periodic|dirichlet>:<extents>" (FVPatchGrid(fused=True, origin=ORIGIN, time=T0).step).  Of the grid rows, the 3-D P = 4
one runs the staged kernel (the halo layers are gathered into the LDS copy); the 15^3 and the P = 6, H = 2 ones have no LDS copy, so flux, eigenvalue
and ncp read the neighbour patch's volumes across a patch face.

Families (state()): benign; riemann -- piecewise constant with the jump inside the patch (even patches) or at its low face (odd ones) plus noise
of 1e-3; scaled_2^-20 -- the benign state times 2^-20.  Depth (swe) and density / pressure (euler_gravity) are positive in every family.  The
step is the one a run takes at CFL 0.9, h = 0.1, with lambda_max the long-double eigenvalue at the volumes' own coordinates and time.
"""
import functools

import numpy as np

from oracle import fv_reference as R
from tests import fv_cases as K
from tests import user_term_sets as T

FAMILIES = ("benign", "riemann", "scaled_2^-20")
BRANCHES = ("ref", "ref-persistent", "staged", "unstaged", "nt1024-staged", "nt1024-unstaged", "slab", "cpt4")
H_VOLUME = K.H_VOLUME
PERSISTENT_PATCHES = K.PERSISTENT_PATCHES
T0 = 0.37                                                  # the time of every row that hands coordinates over
ORIGIN = (0.2, -0.4, 0.6)                                  # low corner of the grid rows
SLOT_PATTERN = K.SLOT_PATTERN
EG, SW, TL, CR = "euler_gravity", "swe", "two_layer_like", "coupled_rational"

ROWS = [
    ("ref", EG, 2, 4, 1, 5, 37, "inplace"),
    ("ref", EG, 2, 4, 1, 5, 37, "slot"),
    ("ref", EG, 2, 4, 1, 5, 37, "oop"),
    ("ref-persistent", EG, 2, 4, 1, 5, PERSISTENT_PATCHES, "inplace"),
    ("staged", SW, 2, 8, 1, 0, 9, "inplace"),
    ("staged", CR, 3, 4, 1, 1, 6, "inplace"),
    ("staged", CR, 3, 4, 1, 1, 6, "inplace-origin"),
    ("staged", CR, 3, 4, 1, 1, 6, "oop"),
    ("unstaged", CR, 3, 6, 2, 6, 3, "inplace"),
    ("nt1024-staged", CR, 2, 20, 1, 0, 3, "inplace"),
    ("nt1024-staged", CR, 2, 20, 1, 0, 3, "slot"),
    ("nt1024-staged", TL, 3, 9, 1, 0, 2, "inplace"),
    ("nt1024-unstaged", CR, 3, 10, 2, 0, 2, "inplace"),
    ("slab", EG, 3, 15, 1, 0, 2, "inplace"),
    ("slab", EG, 3, 15, 1, 0, 3, "slot"),
    ("slab", EG, 3, 13, 1, 2, 3, "inplace"),
    ("slab", EG, 3, 13, 1, 2, 3, "slot"),
    ("cpt4", CR, 3, 15, 1, 0, 2, "inplace"),
    ("cpt4", CR, 3, 15, 1, 0, 3, "slot"),
    ("cpt4", CR, 3, 15, 1, 0, 2, "oop"),
    ("cpt4", TL, 3, 15, 1, 0, 2, "inplace"),
    ("cpt4", SW, 2, 40, 1, 0, 2, "inplace"),
    ("staged", CR, 2, 4, 1, 0, 6, "grid:periodic:3x2"),
    ("staged", CR, 2, 4, 1, 0, 5, "grid:dirichlet:1x5"),
    ("staged", CR, 3, 4, 1, 0, 12, "grid:dirichlet:2x3x2"),
    ("unstaged", CR, 3, 6, 2, 6, 4, "grid:dirichlet:2x1x2"),
    ("cpt4", CR, 3, 15, 1, 0, 2, "grid:periodic:1x2x1"),
    ("slab", EG, 3, 13, 1, 0, 6, "grid:periodic:2x1x3"),
    ("nt1024-staged", SW, 2, 24, 1, 0, 4, "grid:periodic:2x2"),
]


@functools.lru_cache(maxsize=None)
def term_set(name):
    """the SympyPDE (one object per name: built and registered once per process)"""
    return {EG: T.euler_gravity, SW: T.swe, TL: lambda: T.two_layer_like(3), CR: lambda: T.coupled_rational(3)}[name]()


@functools.lru_cache(maxsize=None)
def terms(name):
    return R.UserTerms(term_set(name))


def n_real(row):
    return term_set(row[1]).n_vars


def row_id(row):
    return "%s-%s-%dd-P%d-H%d-%d+%d-n%d-%s" % (row[0], row[1], row[2], row[3], row[4], n_real(row), row[5], row[6], row[7].replace(":", "_"))


def branch(dim, P, H, n_real, n_aux, n_patches, has_xt, has_ncp, entry):
    """fv_dispatch's conditions (fv_rusanov.hip) for a generated term set, corrected mode, 16-byte aligned arrays, n_real = NV"""
    V, S, ncell, pvol = n_real + n_aux, P + 2 * H, P ** dim, (P + 2 * H) ** dim
    grid, oop = entry.startswith("grid"), entry == "oop"
    if ncell <= 256:
        ppb = 256 // ncell
        lds = ppb * pvol * V * 8 + (ppb * 32 if grid else 0)
        if dim == 2 and P == 4 and H == 1 and n_real == 5 and V == 10:
            even = (ppb * (ncell if grid else pvol) * V) % 2 == 0
            return "ref-persistent" if lds <= 65536 and even and n_patches >= ppb * 2048 else "ref"
        return "staged" if lds <= 65536 else "unstaged"
    if ncell <= 1024:
        return "nt1024-staged" if pvol * V * 8 + (32 if grid else 0) <= 65536 else "nt1024-unstaged"
    if dim == 3 and P * P <= 256 and S * S * V <= 2048 and not has_xt and not has_ncp and (not oop) and (not grid or 4 * H * P * V <= 512):
        assert (3 * ((S * S * V + 2) & ~1)) * 8 <= 65536
        return "slab"
    assert ncell <= 4096
    return "cpt4"


def branch_of(row):
    _, name, dim, P, H, n_aux, n, entry = row
    p = term_set(name)
    return branch(dim, P, H, p.n_vars, n_aux, n, bool(p.uses_xt), p.ncp_exprs is not None, entry)


def is_grid(row):
    return row[7].startswith("grid")


def grid_of(row):
    kind, bc, ext = row[7].split(":")
    assert kind == "grid"
    g = tuple(int(x) for x in ext.split("x"))
    assert int(np.prod(g)) == row[6] and len(g) == row[2]
    return g, bc == "dirichlet"


def hands_coordinates(row):
    """does the row hand patch centres and a time to the kernel (every row of a term set that sees them, but the in-place default)"""
    return bool(term_set(row[1]).uses_xt) and row[7] != "inplace-origin"


def coordinates(row, n=None):
    """(centres [n, dim] or None, t): distinct non-zero centres in [-1.5, 1.5] (a grid row: those FVPatchGrid derives from ORIGIN, by its formula)"""
    _, name, dim, P, H, n_aux, n_patches, entry = row
    if not hands_coordinates(row):
        return None, 0.0
    if is_grid(row):
        g, _ = grid_of(row)
        idx = np.stack(np.meshgrid(*[np.arange(x) for x in g], indexing="ij"), axis=-1).reshape(-1, dim)
        return np.asarray(ORIGIN[:dim])[None, :] + (idx + 0.5) * P * H_VOLUME, T0
    rng = np.random.default_rng(500 + dim + P)
    c = rng.uniform(0.25, 1.5, (n_patches, dim)) * rng.choice([-1.0, 1.0], (n_patches, dim))
    return c[:n or n_patches], T0


_BASE = {SW: ((1.0, 0.0, 0.0), (0.5, 0.0, 0.0)), TL: ((1.0, 0.5), (0.25, 1.0)), CR: ((1.0, -0.5, 0.75), (0.25, 0.5, -0.25))}


def _benign(name, sh, rng):
    if name == SW:
        q = np.zeros(sh + (3,))
        q[..., 0] = 1.0 + 0.3 * rng.random(sh)
        q[..., 1] = q[..., 0] * (0.4 * rng.random(sh) - 0.2)
        q[..., 2] = q[..., 0] * (0.4 * rng.random(sh) - 0.2)
        return q
    return np.asarray(_BASE[name][0]) + 0.3 * rng.random(sh + (len(_BASE[name][0]),))


def _riemann(name, n, dim, S, H, P, seed):
    """piecewise constant, jump normal to axis seed % dim: inside the patch (even patches) or at its low face (odd patches), noise 1e-3"""
    rng = np.random.default_rng(seed)
    left, right = (np.asarray(x) for x in _BASE[name])
    q = np.zeros((n,) + (S,) * dim + (len(left),))
    co = np.indices((S,) * dim)[seed % dim]
    for k in range(n):
        at = H + P // 2 if k % 2 == 0 else H
        q[k] = np.where((co < at)[..., None], left, right)
    return q + 1e-3 * rng.uniform(-1, 1, q.shape)


def state(name, family, n, dim, P, H, V, seed):
    """Q [n, S.., V] (H = 0: halo-less): the term set's variables an admissible state of the family, the auxiliary ones uniform in [-1, 1]"""
    if name == EG:
        return K.state(family, n, dim, P, H, V, seed)
    S, m = P + 2 * H, term_set(name).n_vars
    sh = (n,) + (S,) * dim
    rng = np.random.default_rng(seed)
    Q = rng.uniform(-1, 1, sh + (V,))
    if family == "riemann":
        Q[..., :m] = _riemann(name, n, dim, S, H, P, seed)
    else:
        Q[..., :m] = _benign(name, sh, rng) * (2.0 ** -20 if family == "scaled_2^-20" else 1.0)
    return Q


def row_state(row, family, n=None):
    _, name, dim, P, H, n_aux, n_patches, entry = row
    seed = 100 * dim + P + 7 * H + FAMILIES.index(family)
    return state(name, family, n or n_patches, dim, P, 0 if is_grid(row) else H, n_real(row) + n_aux, seed)


def boundary_states(row, family):
    _, name, dim, P, H, n_aux, n_patches, entry = row
    b = state(name, family, 2 * dim, dim, 1, 0, n_real(row) + n_aux, 977 + FAMILIES.index(family)).reshape(2 * dim, -1)
    return {(a, s): b[2 * a + s] for a in range(dim) for s in range(2)}


def lam_max(row, interior_states, centres, t, extra=None):
    """long-double maximum of the eigenvalue over the interior volumes [n, P.., V] at their own coordinates and t (extra: boundary states, which the
    grid evaluates at the origin and t = 0)"""
    _, name, dim, P = row[:4]
    tm = terms(name)
    q = np.asarray(interior_states)
    X = R.volume_centres(centres, len(q), dim, P, H_VOLUME, track=False)
    lam = max(float(np.max(R.user_max_eigenvalue(tm, q, d, X, t))) for d in range(dim))
    if extra is not None:
        lam = max(lam, max(float(np.max(R.user_max_eigenvalue(tm, extra, d))) for d in range(dim)))
    return lam


def cfl_step(row, Q, centres, t, extra=None):
    """(dt, h) at CFL 0.9; Q with halo [n, S.., V] (a patch row) or halo-less [n, P.., V] (a grid row)"""
    _, name, dim, P, H = row[:5]
    q = Q if is_grid(row) else Q[R.interior(dim, P, H)]
    return float(0.9 * H_VOLUME / (dim * lam_max(row, q, centres, t, extra))), H_VOLUME


def slot_of(n):
    return K.slot_of(n)


def patches_with_halo(row, family, n=None):
    """the row's input as a patch array with halo (a grid row: stitched across the patches as the two-pass driver fills the halo layers)"""
    _, name, dim, P, H, n_aux, n_patches, entry = row
    if not is_grid(row):
        return row_state(row, family, n)
    from exahype_amd.solvers import fill_halos_dirichlet, fill_halos_periodic
    grid, dirichlet = grid_of(row)
    S, V = P + 2 * H, n_real(row) + n_aux
    Q = np.zeros(grid + (S,) * dim + (V,))
    Q[(slice(None),) * dim + (slice(H, H + P),) * dim] = row_state(row, family).reshape(grid + (P,) * dim + (V,))
    if dirichlet:
        fill_halos_dirichlet(Q, grid, dim, P, H, boundary_states(row, family))
    else:
        fill_halos_periodic(Q, grid, dim, P, H)
    return Q.reshape((n_patches,) + (S,) * dim + (V,))[:n or n_patches]


def assert_within_bound(got, Q, dt, h, row, centres, t, what, layout="halo", masked=None, **log):
    """`got` (fp64, the kernel's result for the input Q [n, S.., V]) against the long-double reference: every evolved variable of every interior
    volume within 2^-53 E, halo values, auxiliary variables and masked patches bit-equal to the input.  Returns the largest error / bound ratio."""
    from tests.util import log_fv_measurement
    _, name, dim, P, H, n_aux, n_patches, entry = row
    m = n_real(row)
    ref = R.user_update(Q, dt, h, dim, P, H, terms(name), n_aux, centres, t)
    sel = R.interior(dim, P, H)
    got = np.asarray(got)
    gi = got[sel] if layout == "halo" else got.reshape(Q[sel].shape)
    live = np.ones(len(Q), dtype=bool) if masked is None else ~np.asarray(masked)
    assert np.all(ref.E > 0)
    err = np.abs(gi[..., :m].astype(R.LD) - ref.new[sel][..., :m])
    worst = float(np.max((err / (R.U53 * ref.E))[live])) if live.any() else 0.0
    print("%s: err / bound %.3f" % (what, worst))
    log_fv_measurement(what=what, ratio=worst, primitives="ieee", **log)
    assert worst <= 1.0, (what, worst)
    assert np.array_equal(gi[..., m:], Q[sel][..., m:]), what + ": auxiliary variables changed"
    if layout == "halo":
        keep = np.ones(Q.shape[1:], dtype=bool)
        keep[sel[1:] + (slice(None),)] = False
        assert np.array_equal(got[:, keep], Q[:, keep]), what + ": halo values changed"
        assert np.array_equal(got[~live], Q[~live]), what + ": a masked patch was written"
    return worst

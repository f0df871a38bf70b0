"""The case table of the corrected FV Rusanov kernels, shared by the CPU check of the measure (tests/test_fv_reference.py), the dispatch check
(tests/test_fv_dispatch_table.py) and the GPU tests (tests/test_fv_kernels_hp.py).

A row is (branch, dim, P, H, n_real, n_aux, n_patches, pde, entry).  `branch` is the branch of `fv_dispatch` (exahype_amd/csrc/fv_rusanov.hip) the row
reaches in corrected mode, worked out from the dispatch conditions and restated by branch() below; tests/test_fv_dispatch_table.py asserts that
every row reaches the branch it names and that every branch has a row, so a later change of a threshold turns the table red instead of silently moving
a case.  With V = n_real + n_aux, S = P + 2 H, ncell = P^dim, pvol = S^dim:

  ncell <= 256 (ppb = 256 / ncell patches per workgroup, LDS image ppb pvol V 8 B):
    ref               2-D P = 4, H = 1, 5 + 5 variables (the reference's shape, compile-time shape), one pass
    ref-persistent    ... with n_patches >= 16 * 2048: the persistent form (32 805 patches: 2 051 blocks, the last one ragged with 5 patches, odd count)
    staged            image <= 64 KiB: 2-D P = 8 (16 KB); 3-D P = 4 (34.6 KB); 3-D P = 6, H = 2, 3 aux (64 000 B)
    unstaged          image > 64 KiB: 3-D P = 6, H = 2, V = 9 (72 000 B)
  ncell <= 1024 (one patch per 1024-thread workgroup, image pvol V 8 B):
    nt1024-staged     2-D P = 20 (19 KB), P = 24 with 3 aux (43 KB); 3-D P = 9 (53 KB)
    nt1024-unstaged   3-D P = 10, H = 2 (2 744 volumes x 5: 110 KB)
  3-D, P^2 <= 256, S^2 V <= 2048, in place or grid step (grid: 4 H P V <= 512): the plane-streaming kernel
    slab-cache        Euler (NFVAUX: cached 1 / rho, p, c from fast_rcp / fast_sqrt): 15^3; 16^3; 13^3 with 2 aux; 11^3 with H = 2; 12^3 with 2 aux
    slab-cache+lds    ... whose ring exceeds 64 KiB (the hipFuncSetAttribute path): 16^3 with H = 2 (S = 20: 67 248 B)
    slab-generic      advection, n_real = 5 (no NFVAUX, n_real != NV = 8): 15^3 with and without aux, 13^3
    slab-fitnv        advection, n_real = 8 = NV: 13^3 with and without aux (15^3 has S^2 V = 2 312 > 2 048: it cannot be FITNV)
  ncell <= 4096:
    cpt4              four volumes per thread: 2-D P = 40; 3-D P = 16 with 2 aux (S^2 V = 2 268 > 2 048); the out-of-place call of a 15^3 patch (the
                      plane-streaming kernel writes in place only)

Entries: "inplace" (time_step), "slot" (time_step(..., slot=) with SLOT_PATTERN), "oop" (time_step_oop), "grid:<periodic|dirichlet>:<g0>x<g1>[x<g2>]"
(FVPatchGrid(fused=True).step; n_patches = the product of the extents).  The grid rows include extents of 1 and a patch count (12) that is not a
multiple of eight workgroups (the plane-streaming kernel's fv_xcd_contiguous ranges).

State families (state()): benign (tests/util.py euler_patches), supersonic, Euler scaled by 2^-20 and 2^20, and riemann -- piecewise-constant Sod
data with the jump inside the patch (even patches) or at a patch face (odd ones) plus node-wise noise of 1e-3: many neighbours are (nearly) equal, the
increments are tiny and the flux difference cancels.  The step is the one a run takes at CFL 0.9 (dt = 0.9 h / (dim lambda_max)), h = 0.1.
"""
import numpy as np

from oracle import fv_reference as R
from tests.util import euler_patches, euler_scaled_state, euler_supersonic_state

E, A = R.PDE_EULER, R.PDE_ADVECTION
FAMILIES = ("benign", "supersonic", "scaled_2^-20", "scaled_2^20", "riemann")
BRANCHES = ("ref", "ref-persistent", "staged", "unstaged", "nt1024-staged", "nt1024-unstaged", "slab-cache", "slab-cache+lds", "slab-generic",
            "slab-fitnv", "cpt4")
H_VOLUME = 0.1
PERSISTENT_PATCHES = 16 * 2048 + 37

ROWS = [
    ("ref", 2, 4, 1, 5, 5, 37, E, "inplace"),
    ("ref", 2, 4, 1, 5, 5, 37, E, "slot"),
    ("ref", 2, 4, 1, 5, 5, 37, E, "oop"),
    ("ref-persistent", 2, 4, 1, 5, 5, PERSISTENT_PATCHES, E, "inplace"),
    ("staged", 2, 8, 1, 5, 0, 9, E, "inplace"),
    ("staged", 2, 8, 1, 5, 1, 9, A, "inplace"),
    ("staged", 3, 4, 1, 5, 0, 6, E, "inplace"),
    ("staged", 3, 6, 2, 5, 3, 3, E, "inplace"),
    ("staged", 3, 6, 2, 5, 3, 3, E, "oop"),
    ("unstaged", 3, 6, 2, 5, 4, 3, E, "inplace"),
    ("unstaged", 3, 6, 2, 5, 4, 3, E, "slot"),
    ("nt1024-staged", 2, 20, 1, 5, 0, 3, E, "inplace"),
    ("nt1024-staged", 2, 20, 1, 5, 0, 3, E, "slot"),
    ("nt1024-staged", 3, 9, 1, 5, 0, 2, E, "inplace"),
    ("nt1024-unstaged", 3, 10, 2, 5, 0, 2, E, "inplace"),
    ("nt1024-unstaged", 3, 10, 2, 5, 0, 2, E, "oop"),
    ("slab-cache", 3, 15, 1, 5, 0, 2, E, "inplace"),
    ("slab-cache", 3, 15, 1, 5, 0, 3, E, "slot"),
    ("slab-cache", 3, 16, 1, 5, 0, 1, E, "inplace"),
    ("slab-cache", 3, 13, 1, 5, 2, 3, E, "inplace"),
    ("slab-cache", 3, 11, 2, 5, 0, 2, E, "inplace"),
    ("slab-cache+lds", 3, 16, 2, 5, 0, 1, E, "inplace"),
    ("slab-generic", 3, 15, 1, 5, 0, 2, A, "inplace"),
    ("slab-generic", 3, 15, 1, 5, 2, 2, A, "inplace"),
    ("slab-fitnv", 3, 13, 1, 8, 0, 2, A, "inplace"),
    ("slab-fitnv", 3, 13, 1, 8, 1, 2, A, "inplace"),
    ("cpt4", 2, 40, 1, 5, 0, 2, E, "inplace"),
    ("cpt4", 3, 16, 1, 5, 2, 1, E, "inplace"),
    ("cpt4", 3, 15, 1, 5, 0, 2, E, "oop"),
    ("ref", 2, 4, 1, 5, 5, 15, E, "grid:periodic:5x3"),
    ("ref", 2, 4, 1, 5, 5, 7, E, "grid:dirichlet:1x7"),
    ("staged", 3, 4, 1, 5, 0, 12, E, "grid:dirichlet:2x3x2"),
    ("nt1024-staged", 2, 24, 1, 5, 3, 4, E, "grid:periodic:2x2"),
    ("slab-cache", 3, 12, 1, 5, 2, 2, E, "grid:periodic:1x2x1"),
    ("slab-cache", 3, 15, 1, 5, 0, 12, E, "grid:dirichlet:3x2x2"),
    ("slab-generic", 3, 13, 1, 5, 0, 6, A, "grid:periodic:2x1x3"),
    ("cpt4", 2, 40, 1, 5, 0, 4, E, "grid:periodic:2x2"),
]
SLOT_PATTERN = (0, -1, 5, -1, -1, 2, 9)                    # repeated over the patches: a negative entry masks the patch


def row_id(row):
    return "%s-%dd-P%d-H%d-%d+%d-n%d-%s-%s" % (row[0], row[1], row[2], row[3], row[4], row[5], row[6], "euler" if row[7] == E else "adv", row[8].replace(":", "_"))


def branch(dim, P, H, n_real, n_aux, n_patches, pde, entry):
    """fv_dispatch's conditions (fv_rusanov.hip), corrected mode, 16-byte aligned arrays"""
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
    if dim == 3 and P * P <= 256 and S * S * V <= 2048 and (not oop) and (not grid or 4 * H * P * V <= 512):
        cache = pde == E
        lds = (3 * ((S * S * V + 2) & ~1) + (2 * S * S * 3 if cache else 0)) * 8
        return ("slab-cache" if cache else ("slab-fitnv" if n_real == 8 else "slab-generic")) + ("+lds" if lds > 65536 else "")
    assert ncell <= 4096
    return "cpt4"


def uses_device_primitives(row):
    """the plane-streaming kernel with cached scalars is the one that evaluates 1 / rho and c with fast_rcp / fast_sqrt; every other branch (and the
    advection) runs IEEE arithmetic"""
    return branch(*row[1:]).startswith("slab-cache")


def primitives(row):
    return R.DEVICE if uses_device_primitives(row) else R.IEEE


def grid_of(row):
    kind, bc, ext = row[8].split(":")
    assert kind == "grid"
    g = tuple(int(x) for x in ext.split("x"))
    assert int(np.prod(g)) == row[6] and len(g) == row[1]
    return g, bc == "dirichlet"


def _riemann(n, dim, S, H, P, seed):
    """Sod data (1, 0, 0, 0, 2.5 | 0.125, 0, 0, 0, 0.25), jump normal to axis seed % dim: inside the patch (even patches) or at its low face (odd
    patches: between the halo layer and the first interior volume), plus noise of 1e-3 in every value"""
    rng = np.random.default_rng(seed)
    q = np.zeros((n,) + (S,) * dim + (5,))
    ax = seed % dim
    co = np.indices((S,) * dim)[ax]
    left, right = np.array([1.0, 0, 0, 0, 2.5]), np.array([0.125, 0, 0, 0, 0.25])
    for k in range(n):
        at = H + P // 2 if k % 2 == 0 else H
        q[k] = np.where((co < at)[..., None], left, right)
    return q + 1e-3 * rng.uniform(-1, 1, q.shape)


def state(family, n, dim, P, H, V, seed):
    """Q [n, S.., V] (H = 0: halo-less): variables 0..4 an admissible Euler state of the family, the others uniform in [-1, 1]"""
    S = P + 2 * H
    sh = (n,) + (S,) * dim
    if family == "benign":
        return euler_patches(n, dim, S, V, seed)
    Q = np.random.default_rng(seed).uniform(-1, 1, sh + (V,))
    if family == "supersonic":
        Q[..., :5] = euler_supersonic_state(sh, seed + 1)
    elif family.startswith("scaled"):
        Q[..., :5] = euler_scaled_state(sh, seed + 1, 2.0 ** (-20 if family == "scaled_2^-20" else 20))
    else:
        assert family == "riemann"
        Q[..., :5] = _riemann(n, dim, S, H, P, seed)
    return Q


def row_state(row, family, n=None):
    _, dim, P, H, n_real, n_aux, n_patches, pde, entry = row
    seed = 100 * dim + P + 7 * H + FAMILIES.index(family)
    return state(family, n or n_patches, dim, P, 0 if entry.startswith("grid") else H, n_real + n_aux, seed)


def cfl_step(Q, dim, pde, extra=None):
    """(dt, h): the step a run takes at CFL 0.9 on these states (extra: further states, e.g. the boundary's)"""
    if pde == A:
        lam = 1.0
    else:
        lam = max(float(np.max(R.max_eigenvalue(Q, d, pde))) for d in range(dim))
        if extra is not None:
            lam = max(lam, max(float(np.max(R.max_eigenvalue(extra, d, pde))) for d in range(dim)))
    return float(0.9 * H_VOLUME / (dim * lam)), H_VOLUME


def boundary_states(row, family):
    """prescribed states of the 2 dim domain faces: one state of the family each (all different)"""
    _, dim, P, H, n_real, n_aux, n_patches, pde, entry = row
    b = state(family, 2 * dim, dim, 1, 0, n_real + n_aux, 977 + FAMILIES.index(family)).reshape(2 * dim, -1)
    return {(a, s): b[2 * a + s] for a in range(dim) for s in range(2)}


def slot_of(n):
    return np.array([SLOT_PATTERN[k % len(SLOT_PATTERN)] for k in range(n)], dtype=np.int64)


def assert_within_bound(got, Q, dt, h, dim, P, H, n_real, n_aux, pde, prim, what, layout="halo", masked=None, **log):
    """The shared checker: `got` (fp64, the kernel's result for the input Q [n, S.., V]) against the long-double reference -- every evolved
    variable of every interior volume within 2^-53 E (oracle/fv_reference.py; prim: R.IEEE or R.DEVICE), halo and auxiliary values bit-equal to
    the input.  layout "halo": got has Q's layout; "dense": got is [n, P.., V] (time_step_oop).  masked: boolean per patch, True = the patch was
    skipped and must be bit-equal to the input.  Returns the largest error / bound ratio (logged with EXA_FV_ERR_LOG)."""
    from tests.util import log_fv_measurement
    ref = R.update(Q, dt, h, dim, P, H, n_real, n_aux, pde, prim=prim)
    sel = R.interior(dim, P, H)
    got = np.asarray(got)
    gi = got[sel] if layout == "halo" else got.reshape(Q[sel].shape)
    live = np.ones(len(Q), dtype=bool) if masked is None else ~np.asarray(masked)
    err = np.abs(gi[..., :n_real].astype(R.LD) - ref.new[sel][..., :n_real])
    worst = float(np.max((err / (R.U53 * ref.E))[live])) if live.any() else 0.0
    print("%s: err / bound %.3f" % (what, worst))
    log_fv_measurement(what=what, ratio=worst, primitives="device" if prim is R.DEVICE else "ieee", **log)
    assert worst <= 1.0, (what, worst)
    assert np.array_equal(gi[..., n_real:], Q[sel][..., n_real:]), what + ": auxiliary variables changed"
    if layout == "halo":
        keep = np.ones(Q.shape[1:], dtype=bool)
        keep[sel[1:] + (slice(None),)] = False
        assert np.array_equal(got[:, keep], Q[:, keep]), what + ": halo values changed"
        assert np.array_equal(got[~live], Q[~live]), what + ": a masked patch was written"
    return worst


def patches_with_halo(row, family, n=None):
    """The row's input as a patch array with halo [n, S.., V], the form the in-place update and the CPU statements of tests/test_fv_reference.py
    take.  A patch row: row_state (n: only the first n patches).  A grid row: its halo-less states stitched across the patches -- every halo layer
    filled from the face neighbour's interior (periodic wrap) or with the row's boundary states, as the two-pass driver fills them."""
    _, dim, P, H, n_real, n_aux, n_patches, pde, entry = row
    if not entry.startswith("grid"):
        return row_state(row, family, n)
    from exahype_amd.solvers import fill_halos_dirichlet, fill_halos_periodic
    grid, dirichlet = grid_of(row)
    S, V = P + 2 * H, n_real + n_aux
    Q = np.zeros(grid + (S,) * dim + (V,))
    Q[(slice(None),) * dim + (slice(H, H + P),) * dim] = row_state(row, family).reshape(grid + (P,) * dim + (V,))
    if dirichlet:
        fill_halos_dirichlet(Q, grid, dim, P, H, boundary_states(row, family))
    else:
        fill_halos_periodic(Q, grid, dim, P, H)
    return Q.reshape((n_patches,) + (S,) * dim + (V,))

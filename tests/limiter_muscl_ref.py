"""numpy restatement of the subcell limiter with the second-order patch update (SubcellLimiter(fv_mode=FV_MUSCL_HANCOCK)) -- TEST
INFRASTRUCTURE ONLY, never imported by the product.

The patch of a troubled cell has halo 2 and is DEFINED as a window of the ghost-extended global subcell array: the projected state of the
whole block, assembled into one array, extended by two layers axis by axis, in axis order, over the full transverse range
(tests/fv_muscl_ref.global_with_ghosts, the product's own halo fill restated).  build_patch2 cuts that window and replaces the entries the
update never reads (fv_muscl_ref.outside_stencil) by the nearest interior value, as the kernel writes them.

ghost_extend() is a second statement of global_with_ghosts with one switch per MUTANT (a single change each); with no mutant the two agree
bit for bit (tests/test_limiter_muscl_reference.py).

reference_patch2 / projection_bound2: the long-double form from the device's own P and its element-wise bound, as
oracle/limiter_reference.reference_patch and tests/limiter_cases.projection_bound are for halo 1: mirrors, signs and copies add nothing.

replace_troubled2 / step / run_tube: the limited step and the periodic double Sod tube through tests/limiter_ref.run, with the fp64 form
of the second-order update (fv_muscl_ref.fp64_update) in the troubled cells.
"""
import numpy as np

from exahype_amd.boundary import Dirichlet, Outflow, Wall
from oracle import aderdg_numpy as A
from oracle import fv_reference as R
from oracle import limiter_reference as L
from oracle.limiter_numpy import apply_all_axes, projection_matrix, reconstruction_matrix
from tests import fv_muscl_ref as F
from tests import limiter_mood_ref as M
from tests import limiter_ref as LR

MUTANTS = ("edge_from_face", "layer2_copy_of_layer1", "mirror_not_reversed", "wall_sign_dropped", "wrong_side", "layers_swapped",
           "wrong_axis_order")


def ghost_extend(G, dim, conditions=None, mutant=None):
    """G [n_0, .., V] with two ghost layers per side: axis by axis, in axis order, each over the full transverse range (the ghost layers of
    the earlier axes included).  A face without a condition wraps; Outflow / Wall: the mirror image times the signs; Dirichlet: its state."""
    assert mutant is None or mutant in MUTANTS, mutant
    conditions = conditions or {}
    A_ = np.pad(np.asarray(G), [(2, 2)] * dim + [(0, 0)])
    V = A_.shape[-1]
    axes = range(dim - 1, -1, -1) if mutant == "wrong_axis_order" else range(dim)
    for a in axes:
        n = A_.shape[a]
        at = lambda layers: tuple(layers if x == a else slice(None) for x in range(A_.ndim))      # noqa: E731
        lo_halo, hi_halo = slice(0, 2), slice(n - 2, n)
        lo_in, hi_in = slice(2, 4), slice(n - 4, n - 2)
        for side in range(2):
            halo = hi_halo if side else lo_halo
            bc = conditions.get((a, side))
            if bc is None:
                src = (lo_in if side else hi_in) if mutant != "wrong_side" else (hi_in if side else lo_in)
                val = A_[at(src)]
            elif isinstance(bc, (Outflow, Wall)):
                sign = np.ones(V)
                if isinstance(bc, Wall) and mutant != "wall_sign_dropped":
                    sign[:len(bc.sign)] = bc.sign
                src = (hi_in if side else lo_in) if mutant != "wrong_side" else (lo_in if side else hi_in)
                val = A_[at(src)]
                if mutant != "mirror_not_reversed":
                    val = np.flip(val, axis=a)
                val = val * sign
            else:
                val = np.broadcast_to(np.asarray(bc.state if isinstance(bc, Dirichlet) else bc, dtype=np.float64), A_[at(halo)].shape)
            if mutant == "layers_swapped":
                val = np.flip(val, axis=a)
            if mutant == "layer2_copy_of_layer1":
                near = np.take(val, [1, 1] if side == 0 else [0, 0], axis=a)        # the layer next to the interior, twice
                val = near
            A_[at(halo)] = val
    return A_


def _unread_by_nearest(patch, dim, Ns):
    out = patch.copy()
    unread = F.outside_stencil(dim, Ns, 2)
    near = np.pad(patch[(slice(2, -2),) * dim], [(2, 2)] * dim + [(0, 0)], mode="edge")
    out[unread] = near[unread]
    return out


def nearest_interior_index(dim, Ns):
    """[dim][S..]: for every patch entry the patch index of the nearest interior entry"""
    co = np.indices((Ns + 4,) * dim)
    return np.clip(co, 2, Ns + 1)


def build_patch2(proj, idx, conditions=None, mutant=None, extended=None):
    """patch [(N_s + 4).., V] of cell idx from the projected state proj [grid.., N_s.., V]: the window of the ghost-extended global subcell
    array, the unread entries replaced by the nearest interior value.  extended: ghost_extend(assemble(proj)) if the caller has it."""
    dim = (proj.ndim - 1) // 2
    Ns = proj.shape[dim]
    if extended is None:
        G = R.assemble(proj, dim)
        extended = F.global_with_ghosts(G, dim, conditions=conditions) if mutant in (None, "edge_from_face") else ghost_extend(G, dim, conditions, mutant)
    win = extended[tuple(slice(int(idx[a]) * Ns, int(idx[a]) * Ns + Ns + 4) for a in range(dim))]
    if mutant == "edge_from_face":
        win = _edges_from_faces(win, dim)
    return _unread_by_nearest(win, dim, Ns)


def _edges_from_faces(win, dim):
    """the mutant's patch: every edge entry (first halo layer along axes a < b) replaced by the face-halo entry of axis b next to it (the
    nearest interior coordinate along a) -- a value of the face neighbour, not of the diagonal cell"""
    out = win.copy()
    S = win.shape[0]
    for a in range(dim):
        for b in range(a + 1, dim):
            for ia in (1, S - 2):
                for ib in (1, S - 2):
                    dst, src = [slice(None)] * win.ndim, [slice(None)] * win.ndim
                    dst[a], dst[b] = ia, ib
                    src[a], src[b] = (2 if ia == 1 else S - 3), ib
                    out[tuple(dst)] = win[tuple(src)]
    return out


def abs_conditions(conditions):
    """the conditions the bound is assembled with: a mirror without signs, the magnitude of a state"""
    out = {}
    for k, bc in (conditions or {}).items():
        out[k] = Outflow() if isinstance(bc, (Outflow, Wall)) else Dirichlet(np.abs(bc.state))
    return out


def reference_patch2(u, cell, P, conditions=None, proj=None, mutant=None):
    """The patch [(N_s+4)..][nv] (long double) exa_lim_project_patches_halo2 builds for `cell` of the block u[grid.., N.., nv]"""
    dim, nc = L._grid(u, P)
    cc = tuple(int(c) for c in (np.unravel_index(cell, nc) if np.ndim(cell) == 0 else cell))
    if proj is None:
        proj = L.project_grid(u, P)
    return build_patch2(proj, cc, conditions, mutant)


def projection_bound2(u, cell, P, conditions=None, absproj=None):
    """dim (N + 1) 2^-53 (|P| x .. x |P|) |u|, assembled like the patch (mirror entries: the same products; state entries and copies are
    compared exactly by the tests)"""
    dim = (np.ndim(u) - 1) // 2
    return L.rounding_factor(dim, P.shape[1]) * reference_patch2(np.abs(u), cell, np.abs(P), abs_conditions(conditions), proj=absproj)


# ---- the limited step ----------------------------------------------------------------------------------------------------------------
def fv_update2(dim, nv=5, pde=R.PDE_EULER, terms=None):
    """fv(patch [S.., nv], dt, h) -> patch: the second-order update in fp64 (built-in term sets: fv_muscl_ref.fp64_update; a generated
    term set: fv_muscl_ref.update(terms=..., dtype=float64, track=False))"""
    def fv(patch, dt, h):
        Ns = patch.shape[0] - 4
        if terms is not None:
            return np.asarray(F.update(patch[None], dt, h, dim, Ns, 2, nv, 0, pde, terms=terms, track=False, dtype=np.float64).new[0], dtype=np.float64)
        return F.fp64_update(patch[None], dt, h, dim, Ns, 2, nv, pde)[0]
    return fv


def replace_troubled2(u, cand, mask, dt, dx, ops, fv, conditions=None):
    """cand with the cells of mask[grid..] replaced: u projected onto subcells, the patch with halo 2 (build_patch2), one update
    fv(patch, dt, h) with h = dx / N_s, reconstructed"""
    dim = (u.ndim - 1) // 2
    Ns = 2 * ops["N"] - 1
    P = projection_matrix(ops["xi"], Ns)
    Rm = reconstruction_matrix(P, ops["w"])
    out = cand.copy()
    mask = np.asarray(mask)
    if not mask.any():
        return out
    proj = apply_all_axes(P, u, dim, dim)
    ext = F.global_with_ghosts(R.assemble(proj, dim), dim, conditions=conditions)
    core = (slice(2, -2),) * dim
    for idx in zip(*np.nonzero(mask)):
        patch = fv(build_patch2(proj, idx, conditions, extended=ext), dt, dx[0] / Ns)
        out[idx] = apply_all_axes(Rm, patch[core], dim, 0)
    return out


def step(u, dt, dx, ops, pde=None, d0=LR.D0, eps=LR.EPS, floor=LR.FLOOR, scheme="muscl"):
    """One a-posteriori limited step on a periodic grid, Euler criterion: (u_new, mask)"""
    dim = (u.ndim - 1) // 2
    nv = u.shape[-1]
    with np.errstate(all="ignore"):
        cand = A.step(u, dt, dx, ops, pde or A.Euler())
        mask, _ = M.detect(cand, M.cell_bounds(u), d0, eps, floor)
        if scheme == "muscl":
            return replace_troubled2(u, cand, mask, dt, dx, ops, fv_update2(dim, nv)), mask

        def rusanov(patch, dt_, h):                                  # the first-order update of the same windows, for the comparison runs
            new = patch.copy()
            new[(slice(2, -2),) * dim] = F.fp64_block(patch[None], dt_, h, dim, nv, R.PDE_EULER, "rusanov")[0]
            return new
        return replace_troubled2(u, cand, mask, dt, dx, ops, rusanov), mask


def run_tube(N, nx, dim, t_end=0.1, cfl=0.4, max_steps=100000, scheme="muscl"):
    """The periodic double Sod tube (limiter_mood_ref.tube_initial) on nx x 1 (x 1) cells with the CFL step of SubcellLimiter.run.  Returns
    steps, l1, min_rho, min_p (over every step's result), max_troubled, cons -- or what it had and "failed"."""
    u0 = M.tube_initial(N, nx, dim)
    pde = A.Euler()
    out = dict(N=N, nx=nx, dim=dim)
    u, ops = LR.run(u0, pde, N, nx, t_end, cfl, max_steps, lambda u, dt, dx, ops: step(u, dt, dx, ops, pde, scheme=scheme), M.track_minima(out), out)
    if "failed" not in out:
        out.update(l1=M.tube_l1(u, ops["xi"], ops["w"], t_end), cons=M.defects(M.totals(u0, ops["w"]), M.totals(u, ops["w"])))
    return out

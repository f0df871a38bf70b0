"""Case tables and input builders of the limiter kernel tests, shared by the GPU tests (tests/test_limiter_kernels.py) and the CPU check of
their bound (tests/test_limiter_reference.py: a correct fp64 tensor product stays inside it, every mutant of the reference leaves it 100-fold).

Grids: every one has unequal extents on all axes; a single cell along an axis (the cell is its own neighbour there), two cells along an
axis (both neighbours are the same cell) and three (low and high neighbour differ) each occur on every axis, so no mistake in one axis's
neighbour arithmetic can hide behind the grid.  States: node-wise random (different in every cell, no symmetry under an exchange of
axes), one kind per grid in turn: sub- and supersonic Euler, Euler scaled by 2^20, plain Euler -- the magnitude differs by variable."""
import numpy as np

from oracle import limiter_reference as L
from tests.util import euler_dg_state, euler_scaled_state, euler_supersonic_state

LD = np.longdouble
KERNEL_CASES = [(dim, N) for dim in (2, 3) for N in L.ORDERS]
FORMS = ("all_variables", "per_variable")                  # five-variable systems: NV = 5, one round (default) | NV = 1, five rounds (EXA_LIM_PER_VARIABLE=1)
GRIDS = {2: [(1, 3), (3, 2), (2, 3), (3, 1)], 3: [(1, 2, 3), (3, 1, 2), (2, 3, 1)]}
STATE_KINDS = ("supersonic", "scaled_2^20", "plain")
SENTINEL = -8.765432101234567e+250                          # no result comes near it; compared bit for bit


def state(dim, N, nc, nv, which):
    """u[grid.., N.., nv]: nv = 5 Euler (kind STATE_KINDS[which % 3]); other counts: uniform in [-1, 1] times 2^(10 v) in variable v."""
    shape = tuple(nc) + (N,) * dim
    seed = 1000 * dim + 10 * N + which
    if nv != 5:
        return np.random.default_rng(seed).uniform(-1, 1, shape + (nv,)) * 2.0 ** (10 * np.arange(nv))
    kind = STATE_KINDS[which % 3]
    if kind == "supersonic":
        return euler_supersonic_state(shape, seed)
    return euler_scaled_state(shape, seed, 2.0 ** 20) if kind == "scaled_2^20" else euler_dg_state(shape, seed)


def inputs(dim, N, nv=5):
    """[(nc, kind, u)] for every grid of GRIDS[dim]."""
    return [(nc, STATE_KINDS[i % 3] if nv == 5 else "uniform", state(dim, N, nc, nv, i)) for i, nc in enumerate(GRIDS[dim])]


def cell_list(ncell, seed, subset=False):
    """Every cell of the grid (subset: about half of them, at least one) in a shuffled order, with -1 slots in between and at both ends."""
    rng = np.random.default_rng(seed)
    cells = rng.permutation(ncell)
    if subset:
        cells = cells[:max(1, (ncell + 1) // 2)]
    out = [-1]
    for i, c in enumerate(cells):
        out.append(int(c))
        if i == 0 or rng.random() < 0.4:
            out.append(-1)
    if out[-1] != -1:
        out.append(-1)
    return np.array(out, dtype=np.int64)


def ghost_faces(dim):
    """Faces that get a ghost buffer in the ghost-layer test: both sides of axis 0 in 3-D, only the low side of axis 0 in 2-D, only the
    high side of the last axis; the other faces keep the periodic wrap."""
    return [(0, 0), (0, 1), (2, 1)] if dim == 3 else [(0, 0), (1, 1)]


def ghost_buffers(dim, N, nc, nv, faces):
    """{(a, side): [transverse cells][N_s^(dim-1)][nv]} of values no cell of the block holds (distinct integers beyond 2^40)."""
    Ns = 2 * N - 1
    out = {}
    for a, side in faces:
        nt = int(np.prod(nc)) // nc[a]
        n = nt * Ns ** (dim - 1) * nv
        out[(a, side)] = (2.0 ** 40 * (1 + 2 * a + side) + np.arange(n, dtype=np.float64)).reshape(nt, Ns ** (dim - 1), nv)
    return out


def random_patches(dim, N, nv, n, seed):
    """Patches for the reconstruction: interior uniform in [-1, 1] times 2^(5 v) in variable v (no polynomial: every column of R matters),
    halo entries +-1e30 (a leak of one of them into the result is 1e30 against a bound of 1e-10)."""
    S = 2 * N + 1
    rng = np.random.default_rng(seed)
    p = np.where(rng.random((n,) + (S,) * dim + (nv,)) < 0.5, -1e30, 1e30)
    core = (slice(None),) + (slice(1, -1),) * dim
    p[core] = rng.uniform(-1, 1, p[core].shape) * 2.0 ** (5 * np.arange(nv))
    return p


def projection_bound(u, cell, P, ghosts=None, absproj=None):
    """Element-wise bound of an fp64 patch against reference_patch(u, cell, P, ghosts): dim (N + 1) 2^-53 (|P| x .. x |P|) |u|, assembled
    like the patch (ghost entries are copies: their bound is their rounding-free value times the same factor, and they are compared exactly
    by the tests that use them)."""
    dim = (np.ndim(u) - 1) // 2
    absg = None if ghosts is None else {k: np.abs(v) for k, v in ghosts.items()}
    return L.rounding_factor(dim, P.shape[1]) * L.reference_patch(np.abs(u), cell, np.abs(P), absg, proj=absproj)


def face_bound(u, d, side, P):
    dim = (np.ndim(u) - 1) // 2
    return L.rounding_factor(dim, P.shape[1]) * L.reference_face_layers(np.abs(u), d, side, np.abs(P))


def reconstruction_bound(patch, R):
    dim = np.ndim(patch) - 1
    return L.rounding_factor(dim, R.shape[1]) * L.reference_reconstruct(np.abs(patch), np.abs(R))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (inf where the bound is 0 and the values differ)."""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bound)
    return float(np.max(r))

"""Every limiter glue kernel of exahype_amd/csrc/limiter.hip against the long-double reference (oracle/limiter_reference.py), through the C
entry points: projection onto the FV patch with halo (periodic and with ghost layers), the face layers of a block face, the
reconstruction -- at every order N = 2 .. 8 in 2-D and 3-D, in both instantiations that serve five-variable systems (NV = 5: all
variables in a lane, one round | NV = 1: one variable at a time, EXA_LIM_PER_VARIABLE=1) and in the NV = 1 instantiation at one and two variables.

Operators: exa_lim_operators against tests/golden/limiter_operators_hp.json (mpmath, 40 digits) within 8 * 2^-53 * cond(K).
Kernels: against the reference built from the DEVICE's own P, R applied in long double, element by element within
dim * (C + 1) * 2^-53 * (|M| x .. x |M|) |input| (C = N for P, N_s for R) -- the rounding of a correct fp64 tensor product and nothing else;
tests/test_limiter_reference.py shows on the CPU that numpy's fp64 products stay inside that bound on these very inputs and that every
mutant of the reference (wrong side, axis, layer, neighbour, edge entry, operator row) leaves it 100-fold.  Grids and states:
tests/limiter_cases.py.  Nothing here imports mpmath.

Variable counts other than five: nv = 1 is the built-in advection, nv = 2 the generated term set `reaction_advection` of
tests/test_user_pde.py (built once, by whichever module needs it first; registered once here).  Both give a plan at every (dim, N) of the table: no case is left out.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import limiter_reference as L
from tests import limiter_cases as K
from tests.util import log_limiter_measurement

pytestmark = pytest.mark.gpu
LD = np.longdouble
HP = L.load_operators_file()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _two_variable_pde():
    """pde id of the generated two-variable term set: built (if no module has yet) and registered once, reused by every case."""
    from tests.test_user_pde import reaction_advection
    return reaction_advection().register()


def _solver(dim, N, nc, nv=5):
    from exahype_amd import solvers as exa
    if nv == 5:
        return exa.AderDgSolver(dim, N, nc)
    if nv == 1:
        return exa.AderDgSolver(dim, N, nc, pde=exa.PDE_ADVECTION, n_vars=1)
    assert nv == 2
    return exa.AderDgSolver(dim, N, nc, pde=_two_variable_pde(), n_vars=2)


def _operators(s):
    """The device library's P[N_s][N], R[N][N_s] (fp64) as long double."""
    from exahype_amd import solvers as exa
    N, Ns = s.N, 2 * s.N - 1
    P, R = np.zeros((Ns, N)), np.zeros((N, Ns))
    exa.check(s.lib.exa_lim_operators(s._plan, P.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p)))
    return P.astype(LD), R.astype(LD)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _project(s, u, cells, ghosts=None):
    """exa_dg_project_patches(_ghost) for the cell list over sentinel-filled patches -> [len(cells)][(N_s+2)..][nv]."""
    import torch
    from exahype_amd import solvers as exa
    S = 2 * s.N + 1
    s.upload(u)
    cd = torch.as_tensor(cells).cuda()
    n = len(cells)
    assert s.lib.exa_lim_patch_count(s._plan) == S ** s.dim * s.nv
    patches = torch.full((n, S ** s.dim * s.nv), K.SENTINEL, dtype=torch.float64, device="cuda")
    if ghosts is None:
        exa.check(s.lib.exa_dg_project_patches(s._plan, _ptr(s.u), _ptr(cd), n, _ptr(patches), None))
    else:
        keep = {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in ghosts.items()}
        arr = (C.c_void_p * 6)(*[keep[(f // 2, f % 2)].data_ptr() if (f // 2, f % 2) in keep else None for f in range(6)])
        exa.check(s.lib.exa_dg_project_patches_ghost(s._plan, _ptr(s.u), _ptr(cd), n, _ptr(patches), arr, None))
    torch.cuda.synchronize()
    return patches.cpu().numpy().reshape((n,) + (S,) * s.dim + (s.nv,))


def _face_layers(s, u, d, side, need=None):
    """exa_lim_face_layers over a sentinel-filled buffer -> [transverse cells][N_s^(dim-1)][nv]."""
    import torch
    from exahype_amd import solvers as exa
    Ns = 2 * s.N - 1
    s.upload(u)
    nt = int(np.prod(s.nc)) // s.nc[d]
    count = s.lib.exa_lim_face_layer_count(s._plan, d)
    assert count == nt * Ns ** (s.dim - 1) * s.nv
    out = torch.full((count,), K.SENTINEL, dtype=torch.float64, device="cuda")
    nd = None if need is None else torch.as_tensor(np.asarray(need, dtype=np.float64)).cuda()
    exa.check(s.lib.exa_lim_face_layers(s._plan, _ptr(s.u), d, side, None if nd is None else _ptr(nd), _ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(nt, Ns ** (s.dim - 1), s.nv)


def _reconstruct(s, patches, cells, u0):
    """exa_dg_reconstruct_patches of patches[len(cells)] into a block that holds u0 -> the block afterwards."""
    import torch
    from exahype_amd import solvers as exa
    s.upload(u0)
    cd = torch.as_tensor(cells).cuda()
    pd = torch.as_tensor(np.ascontiguousarray(patches)).cuda()
    exa.check(s.lib.exa_dg_reconstruct_patches(s._plan, _ptr(pd), _ptr(cd), len(cells), _ptr(s.u), None))
    torch.cuda.synchronize()
    return s.download()


def _check_patches(got, u, cells, P, ghosts=None):
    """Every listed cell's whole patch within the bound of the reference; the patches of -1 slots untouched.  Returns the worst ratio."""
    dim = (u.ndim - 1) // 2
    proj, absproj = L.project_grid(u, P), L.project_grid(np.abs(u), np.abs(P))
    worst = 0.0
    for i, cell in enumerate(cells):
        if cell < 0:
            assert np.all(_bits(got[i]) == _bits(np.float64(K.SENTINEL))), "patch %d of an empty slot was written" % i
            continue
        ref = L.reference_patch(u, cell, P, ghosts, proj=proj)
        bound = K.projection_bound(u, cell, P, ghosts, absproj=absproj)
        bad = np.argwhere(~(np.abs(got[i].astype(LD) - ref) <= bound))
        assert bad.size == 0, "cell %d (slot %d) of grid %s: %d entries outside the bound, first at patch index %s (dim %d): got %r, reference %r, bound %.3e" % (
            cell, i, u.shape[:dim], len(bad), tuple(bad[0]), dim, got[i][tuple(bad[0])], float(ref[tuple(bad[0])]), float(bound[tuple(bad[0])]))
        worst = max(worst, K.worst_ratio(got[i], ref, bound))
    return worst


def _set_form(monkeypatch, form):
    monkeypatch.setenv("EXA_LIM_PER_VARIABLE", "1" if form == "per_variable" else "0")


@pytest.mark.parametrize("N", L.ORDERS)
def test_device_operators_vs_reference(N):
    P, R = _operators(_solver(2, N, (1, 1)))
    h = HP[N]
    tol = L.operator_tolerance(h["condK"])
    eP, eR = float(np.max(np.abs(P - h["P"]))), float(np.max(np.abs(R - h["R"])))
    log_limiter_measurement("operators", N=N, err_P=eP, err_R=eR, tol=tol)
    assert eP <= tol and eR <= tol, (eP, eR, tol)
    P3, R3 = _operators(_solver(3, N, (1, 1, 1)))
    assert np.array_equal(P3, P) and np.array_equal(R3, R)


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("dim,N", K.KERNEL_CASES)
def test_projection_whole_patch(dim, N, form, monkeypatch):
    _set_form(monkeypatch, form)
    worst = 0.0
    for g, (nc, kind, u) in enumerate(K.inputs(dim, N)):
        s = _solver(dim, N, nc)
        P, _ = _operators(s)
        cells = K.cell_list(int(np.prod(nc)), seed=100 * N + g)
        worst = max(worst, _check_patches(_project(s, u, cells), u, cells, P))
    log_limiter_measurement("projection", dim=dim, N=N, form=form, nv=5, ratio=worst)


@pytest.mark.parametrize("nv", [1, 2])
@pytest.mark.parametrize("dim,N", K.KERNEL_CASES)
def test_other_variable_counts(dim, N, nv):
    """The NV = 1 instantiation at the strides of one and two variables (one round | two): projection (whole patch), face layers and
    reconstruction."""
    worst = [0.0, 0.0, 0.0]
    for g, (nc, kind, u) in enumerate(K.inputs(dim, N, nv)):
        s = _solver(dim, N, nc, nv)
        P, R = _operators(s)
        ncell = int(np.prod(nc))
        cells = K.cell_list(ncell, seed=200 * N + g)
        worst[0] = max(worst[0], _check_patches(_project(s, u, cells), u, cells, P))
        for d in range(dim):
            for side in (0, 1):
                worst[1] = max(worst[1], _check_face_layers(s, u, d, side, P, None))
        worst[2] = max(worst[2], _check_reconstruction(s, R, u, seed=300 * N + g))
    for kind, w in zip(("projection", "face_layers", "reconstruction"), worst):
        log_limiter_measurement(kind, dim=dim, N=N, form="per_variable", nv=nv, ratio=w)


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("dim,N", K.KERNEL_CASES)
def test_projection_with_ghost_layers(dim, N, form, monkeypatch):
    """Faces with a buffer take it at the cells of that block face, bit for bit, and nowhere else; faces without one keep the periodic wrap;
    edge and corner entries still come from the cell's own projection (all of that is reference_patch with ghosts)."""
    _set_form(monkeypatch, form)
    faces = K.ghost_faces(dim)
    worst = 0.0
    for g, (nc, kind, u) in enumerate(K.inputs(dim, N)):
        s = _solver(dim, N, nc)
        P, _ = _operators(s)
        gh = K.ghost_buffers(dim, N, nc, 5, faces)
        cells = K.cell_list(int(np.prod(nc)), seed=400 * N + g)
        got = _project(s, u, cells, gh)
        worst = max(worst, _check_patches(got, u, cells, P, gh))
        Ns, n_ghost = 2 * N - 1, 0
        for i, cell in enumerate(cells):
            if cell < 0:
                continue
            cc = np.unravel_index(cell, nc)
            for (a, side), buf in gh.items():
                sl = [slice(1, -1)] * dim
                sl[a] = Ns + 1 if side else 0
                face = got[i][tuple(sl)].reshape(-1, 5)
                if cc[a] == (nc[a] - 1 if side else 0):
                    assert np.array_equal(face, buf[L.transverse_index(cc, nc, a)]), (nc, cell, a, side)
                    n_ghost += 1
                else:
                    assert np.all(np.abs(face) < 2.0 ** 39), (nc, cell, a, side)         # (no ghost value away from the block face)
        assert n_ghost > 0
    log_limiter_measurement("ghost", dim=dim, N=N, form=form, nv=5, ratio=worst)


def _check_face_layers(s, u, d, side, P, need):
    got = _face_layers(s, u, d, side, need)
    ref, bound = L.reference_face_layers(u, d, side, P), K.face_bound(u, d, side, P)
    done = np.ones(len(got), bool) if need is None else np.asarray(need) != 0
    assert np.all(_bits(got[~done]) == _bits(np.float64(K.SENTINEL))), "face layer (%d, %d): a skipped entry was written" % (d, side)
    bad = np.argwhere(~(np.abs(got[done].astype(LD) - ref[done]) <= bound[done]))
    assert bad.size == 0, "face layer (%d, %d) of grid %s: %d entries outside the bound, first at [cell, subcell, var] %s of the computed ones" % (
        d, side, tuple(s.nc), len(bad), tuple(bad[0]))
    return K.worst_ratio(got[done], ref[done], bound[done]) if done.any() else 0.0


# (the cases of the default form keep the ids they had when the face-layer kernel had one form: [dim-N])
@pytest.mark.parametrize("dim,N,form", [(dim, N, form) for form in K.FORMS for dim, N in K.KERNEL_CASES],
                         ids=["%d-%d%s" % (dim, N, "" if form == K.FORMS[0] else "-" + form) for form in K.FORMS for dim, N in K.KERNEL_CASES])
def test_face_layers(dim, N, form, monkeypatch):
    """Every (d, side): all cells (need = NULL), then a mask of mixed zeros and non-zeros over a sentinel-filled output.  The layers of the
    two instantiations of the face-layer kernel are bit-equal.  Then the layers as ghost buffers of the opposite faces of the same block:
    the patches must equal the periodic ones bit for bit (the face-layer kernel and the halo part of the projection kernel compute the
    same sums in the same order), the projection in either form."""
    other = K.FORMS[1 - K.FORMS.index(form)]
    worst = 0.0
    for g, (nc, kind, u) in enumerate(K.inputs(dim, N)):
        s = _solver(dim, N, nc)
        P, _ = _operators(s)
        rng = np.random.default_rng(500 * N + g)
        layers = {}
        for d in range(dim):
            nt = int(np.prod(nc)) // nc[d]
            for side in (0, 1):
                _set_form(monkeypatch, form)
                worst = max(worst, _check_face_layers(s, u, d, side, P, None))
                need = rng.choice([0.0, 1.0, -2.5, 1e-300], size=nt)
                if nt > 1:
                    need[rng.integers(nt)] = 0.0
                    need[(np.flatnonzero(need == 0)[0] + 1) % nt] = 3.0
                worst = max(worst, _check_face_layers(s, u, d, side, P, need))
                mine = [_face_layers(s, u, d, side), _face_layers(s, u, d, side, need)]
                layers[(d, 1 - side)] = mine[0]                                # what the block across face (d, 1 - side) would send
                _set_form(monkeypatch, other)
                for got, nd in zip(mine, (None, need)):
                    assert np.array_equal(_bits(got), _bits(_face_layers(s, u, d, side, nd))), (nc, d, side, form, other)
        cells = K.cell_list(int(np.prod(nc)), seed=600 * N + g)
        for project_form in K.FORMS:
            _set_form(monkeypatch, project_form)
            periodic, ghosted = _project(s, u, cells), _project(s, u, cells, layers)
            assert np.array_equal(_bits(periodic), _bits(ghosted)), (nc, form, project_form)
    log_limiter_measurement("face_layers", dim=dim, N=N, form=form, nv=5, ratio=worst)


def _check_reconstruction(s, R, u0, seed):
    """Random patches with +-1e30 halos into about half of the cells of a block that holds u0; returns the worst ratio."""
    dim, N, nv, nc = s.dim, s.N, s.nv, tuple(s.nc)
    ncell = int(np.prod(nc))
    cells = K.cell_list(ncell, seed, subset=True)
    patches = K.random_patches(dim, N, nv, len(cells), seed)
    got = _reconstruct(s, patches, cells, u0).reshape((ncell,) + (N,) * dim + (nv,))
    want = np.ascontiguousarray(u0).reshape(got.shape)
    worst = 0.0
    for c in range(ncell):
        slots = np.flatnonzero(cells == c)
        if len(slots) == 0:
            assert np.array_equal(_bits(got[c]), _bits(want[c])), "cell %d is not in the list and was written" % c
            continue
        p = patches[slots[0]]
        ref, bound = L.reference_reconstruct(p, R), K.reconstruction_bound(p, R)
        bad = np.argwhere(~(np.abs(got[c].astype(LD) - ref) <= bound))
        assert bad.size == 0, "cell %d of grid %s: %d nodes outside the bound, first at %s: got %r, reference %r, bound %.3e" % (
            c, nc, len(bad), tuple(bad[0]), got[c][tuple(bad[0])], float(ref[tuple(bad[0])]), float(bound[tuple(bad[0])]))
        worst = max(worst, K.worst_ratio(got[c], ref, bound))
    return worst


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("dim,N", K.KERNEL_CASES)
def test_reconstruction(dim, N, form, monkeypatch):
    _set_form(monkeypatch, form)
    worst = 0.0
    for g, (nc, kind, u) in enumerate(K.inputs(dim, N)):
        s = _solver(dim, N, nc)
        _, R = _operators(s)
        worst = max(worst, _check_reconstruction(s, R, u, seed=700 * N + g))
    log_limiter_measurement("reconstruction", dim=dim, N=N, form=form, nv=5, ratio=worst)


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("dim,N", K.KERNEL_CASES)
def test_projection_then_reconstruction_returns_u(dim, N, form, monkeypatch):
    """project -> reconstruct returns u, node by node, to the sum of the two rounding bounds: the projection's, carried through |R| x .. x |R|,
    plus the reconstruction's on the patch it was given.  Nothing is allowed for the operators: what the device's R P misses the identity by
    has to fit into the rounding bounds as well."""
    _set_form(monkeypatch, form)
    worst = 0.0
    for g, (nc, kind, u) in enumerate(K.inputs(dim, N)):
        s = _solver(dim, N, nc)
        P, R = _operators(s)
        ncell = int(np.prod(nc))
        cells = K.cell_list(ncell, seed=800 * N + g)
        patches = _project(s, u, cells)
        got = _reconstruct(s, patches, cells, np.full(u.shape, K.SENTINEL)).reshape((ncell,) + (N,) * dim + (5,))
        want = u.reshape(got.shape).astype(LD)
        core = (slice(1, -1),) * dim
        for i, cell in enumerate(cells):
            if cell < 0:
                continue
            pb = np.zeros(patches[i].shape, LD)
            pb[core] = K.projection_bound(u, cell, P)[core]
            bound = L.reference_reconstruct(pb, np.abs(R)) + K.reconstruction_bound(patches[i], R)
            bad = np.argwhere(~(np.abs(got[cell].astype(LD) - want[cell]) <= bound))
            assert bad.size == 0, "cell %d of grid %s: %d nodes outside the bound, first at %s: got %r, u %r, bound %.3e" % (
                cell, nc, len(bad), tuple(bad[0]), got[cell][tuple(bad[0])], float(want[cell][tuple(bad[0])]), float(bound[tuple(bad[0])]))
            worst = max(worst, K.worst_ratio(got[cell], want[cell], bound))
    log_limiter_measurement("round_trip", dim=dim, N=N, form=form, nv=5, ratio=worst)

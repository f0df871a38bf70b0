"""SubcellLimiter(fv_mode=FV_MUSCL_HANCOCK): the second-order patch update in the troubled cells of the limited ADER-DG step, and the
three C entry points under it (exa_lim_patch_count_halo, exa_lim_project_patches_halo2, exa_lim_reconstruct_patches_halo).

  * the projection onto patches with halo 2 against the long-double reference from the device's own P (tests/limiter_muscl_ref.py
    reference_patch2), element by element over the WHOLE patch within rounding_factor(dim, N) (|P| x .. x |P|) |u| -- the bound
    tests/test_limiter_muscl_reference.py shows satisfiable and tight on these inputs; patches are filled with a sentinel first, -1 slots
    stay untouched, the entries the update never reads are bit-equal to the interior entry they copy; periodic grids at every order,
    one and two variables, and faces with conditions (state entries bit-equal);
  * the reconstruction from patches with halo 2 bit-equal to the existing entry point on the same interiors;
  * one step(dt, mask) against the restatement around the solver's own DG candidate to 1e-10 (the parity figure of DESIGN.md 2),
    untroubled cells bit-equal to the plain step; two step_a_posteriori steps against the restatement; the tube through run(track=True)
    against tests/golden/limiter_muscl_tube.json;
  * the refusals, and fv_mode=FV_RUSANOV equal to the default bit for bit.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from oracle import limiter_reference as L
from tests import fv_muscl_ref as F
from tests import limiter_cases as K
from tests import limiter_muscl_cases as KM
from tests import limiter_muscl_ref as M2
from tests.util import euler_dg_state

pytestmark = pytest.mark.gpu
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _two_variable_pde():
    from tests.test_user_pde import reaction_advection
    return reaction_advection().register()


def _solver(dim, N, nc, nv=5, **kw):
    from exahype_amd import solvers as exa
    if nv == 5:
        return exa.AderDgSolver(dim, N, nc, **kw)
    if nv == 1:
        return exa.AderDgSolver(dim, N, nc, pde=exa.PDE_ADVECTION, n_vars=1, **kw)
    assert nv == 2
    return exa.AderDgSolver(dim, N, nc, pde=_two_variable_pde(), n_vars=2, **kw)


def _operators(s):
    from exahype_amd import solvers as exa
    N, Ns = s.N, 2 * s.N - 1
    P, R = np.zeros((Ns, N)), np.zeros((N, Ns))
    exa.check(s.lib.exa_lim_operators(s._plan, P.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p)))
    return P.astype(LD), R.astype(LD)


def _faces(dim, nv, conditions):
    """(kinds ctypes array or None, data device tensor or None) of exa_lim_project_patches_halo2: the pair boundary.fv_faces resolves"""
    import torch
    from exahype_amd import _lib
    from exahype_amd.boundary import fv_faces
    if not conditions:
        return None, None
    kinds, data, _ = fv_faces(conditions, dim, nv, 0, _lib.PDE_EULER)
    return (C.c_int * len(kinds))(*kinds), torch.as_tensor(data).cuda()


def _project2(s, u, cells, conditions=None):
    """exa_lim_project_patches_halo2 for the cell list over sentinel-filled patches -> [len(cells)][(N_s+4)..][nv]"""
    import torch
    from exahype_amd import solvers as exa
    S = 2 * s.N + 3
    s.upload(u)
    cd = torch.as_tensor(cells).cuda()
    n = len(cells)
    assert s.lib.exa_lim_patch_count_halo(s._plan, 2) == S ** s.dim * s.nv
    assert s.lib.exa_lim_patch_count_halo(s._plan, 1) == s.lib.exa_lim_patch_count(s._plan)
    patches = torch.full((n, S ** s.dim * s.nv), K.SENTINEL, dtype=torch.float64, device="cuda")
    kinds, data = _faces(s.dim, s.nv, conditions)
    exa.check(s.lib.exa_lim_project_patches_halo2(s._plan, _ptr(s.u), _ptr(cd), n, _ptr(patches), kinds, None if data is None else _ptr(data), None))
    torch.cuda.synchronize()
    return patches.cpu().numpy().reshape((n,) + (S,) * s.dim + (s.nv,))


def _check_patches2(got, u, cells, P, conditions=None):
    """every listed cell's whole patch within the bound of the reference, the unread entries copies of the interior, state entries exact, the
    patches of -1 slots untouched -> the worst ratio"""
    from exahype_amd.boundary import Dirichlet
    dim = (u.ndim - 1) // 2
    nc = u.shape[:dim]
    Ns = P.shape[0]
    proj, absproj = L.project_grid(u, P), L.project_grid(np.abs(u), np.abs(P))
    unread = F.outside_stencil(dim, Ns, 2)
    near = tuple(M2.nearest_interior_index(dim, Ns))
    worst = 0.0
    for i, cell in enumerate(cells):
        if cell < 0:
            assert np.all(_bits(got[i]) == _bits(np.float64(K.SENTINEL))), "patch %d of an empty slot was written" % i
            continue
        ref = M2.reference_patch2(u, cell, P, conditions, proj=proj)
        bound = M2.projection_bound2(u, cell, P, conditions, absproj=absproj)
        bad = np.argwhere(~(np.abs(got[i].astype(LD) - ref) <= bound))
        assert bad.size == 0, "cell %d (slot %d) of grid %s: %d entries outside the bound, first at patch index %s (dim %d): got %r, reference %r, bound %.3e" % (
            cell, i, nc, len(bad), tuple(bad[0]), dim, got[i][tuple(bad[0])], float(ref[tuple(bad[0])]), float(bound[tuple(bad[0])]))
        assert np.array_equal(_bits(got[i][unread]), _bits(got[i][near][unread])), "cell %d: an unread entry is not the interior entry it copies" % cell
        cc = np.unravel_index(cell, nc)
        for (a, side), bc in (conditions or {}).items():
            if not (isinstance(bc, Dirichlet) and cc[a] == (nc[a] - 1 if side else 0)):
                continue
            # both layers beyond a state face are the state, bit for bit, over the transverse interior ...
            sl = [slice(2, -2)] * dim
            sl[a] = slice(Ns + 2, Ns + 4) if side else slice(0, 2)
            assert np.array_equal(_bits(got[i][tuple(sl)]), _bits(np.broadcast_to(bc.state, got[i][tuple(sl)].shape))), (cell, a, side)
            if a == dim - 1:
                # ... and the last axis is applied last: its state also fills the edge entries the update reads
                sl = [slice(1, -1)] * dim
                sl[a] = slice(Ns + 2, Ns + 4) if side else slice(0, 2)
                read = ~unread[tuple(sl)]
                assert np.array_equal(_bits(got[i][tuple(sl)][read]), _bits(np.broadcast_to(bc.state, got[i][tuple(sl)].shape)[read])), (cell, a, side)
        worst = max(worst, K.worst_ratio(got[i], ref, bound))
    return worst


@pytest.mark.parametrize("dim,N", KM.KERNEL_CASES)
def test_projection_halo2_whole_patch(dim, N):
    worst = 0.0
    for g, (nc, u) in enumerate(KM.inputs(dim, N)):
        s = _solver(dim, N, nc)
        P, _ = _operators(s)
        cells = K.cell_list(int(np.prod(nc)), seed=100 * N + g)
        worst = max(worst, _check_patches2(_project2(s, u, cells), u, cells, P))
    print("projection halo 2, dim %d N %d: err / bound %.3f" % (dim, N, worst))


@pytest.mark.parametrize("nv", [1, 2])
@pytest.mark.parametrize("dim,N", KM.OTHER_NV_CASES)
def test_projection_halo2_other_variable_counts(dim, N, nv):
    worst = 0.0
    for g, (nc, u) in enumerate(KM.inputs(dim, N, nv)):
        s = _solver(dim, N, nc, nv)
        P, _ = _operators(s)
        cells = K.cell_list(int(np.prod(nc)), seed=200 * N + g)
        worst = max(worst, _check_patches2(_project2(s, u, cells), u, cells, P))
    print("projection halo 2, dim %d N %d nv %d: err / bound %.3f" % (dim, N, nv, worst))


@pytest.mark.parametrize("dim,N", [(2, 2), (2, 5), (2, 8), (3, 2), (3, 3), (3, 5)])
def test_projection_halo2_faces_with_conditions(dim, N):
    """tests/limiter_muscl_cases.py BC_KINDS: wall / outflow with states on the last axis, wall-wall corners, states on the EARLIER axis under walls"""
    worst = 0.0
    for g, (kind, cond, nc, u) in enumerate(KM.bc_inputs(dim, N)):
        s = _solver(dim, N, nc)
        P, _ = _operators(s)
        cells = K.cell_list(int(np.prod(nc)), seed=300 * N + g)
        worst = max(worst, _check_patches2(_project2(s, u, cells, cond), u, cells, P, cond))
    print("projection halo 2 with conditions, dim %d N %d: err / bound %.3f" % (dim, N, worst))


@pytest.mark.parametrize("dim,N", [(2, 2), (2, 8), (3, 2), (3, 5)])
def test_reconstruction_halo2_equals_halo1(dim, N):
    import torch
    from exahype_amd import solvers as exa
    nc = KM.GRIDS[dim][0]
    ncell = int(np.prod(nc))
    s = _solver(dim, N, nc)
    u0 = K.state(dim, N, nc, 5, 0)
    cells = K.cell_list(ncell, seed=7 * N + dim, subset=True)
    p1 = K.random_patches(dim, N, 5, len(cells), seed=11 * N + dim)
    p2 = KM.repad(p1, dim)
    cd = torch.as_tensor(cells).cuda()
    res = []
    for patches, halo in ((p1, None), (p1, 1), (p2, 2)):
        s.upload(u0)
        pd = torch.as_tensor(np.ascontiguousarray(patches)).cuda()
        if halo is None:
            exa.check(s.lib.exa_dg_reconstruct_patches(s._plan, _ptr(pd), _ptr(cd), len(cells), _ptr(s.u), None))
        else:
            exa.check(s.lib.exa_lim_reconstruct_patches_halo(s._plan, _ptr(pd), _ptr(cd), len(cells), _ptr(s.u), halo, None))
        torch.cuda.synchronize()
        res.append(s.download())
    assert np.all(np.abs(res[0]) < 1e20)                           # (no halo entry leaked)
    assert not np.array_equal(res[0], np.asarray(u0).reshape(res[0].shape))
    assert np.array_equal(_bits(res[1]), _bits(res[0])) and np.array_equal(_bits(res[2]), _bits(res[0]))
    rc = s.lib.exa_lim_reconstruct_patches_halo(s._plan, _ptr(pd), _ptr(cd), len(cells), _ptr(s.u), 3, None)
    assert rc == -1 and b"halo" in s.lib.exa_last_error()
    assert s.lib.exa_lim_patch_count_halo(s._plan, 3) == -1


# ---- the limited step --------------------------------------------------------------------------------------------------------------------
def _cfl_dt(u, dim, N, dx):
    from oracle import aderdg_numpy as A
    lam = max(np.max(A.Euler().maxeig(u, d)) for d in range(dim))
    return 0.4 * dx / ((2 * N - 1) * dim * lam)


def _one_step(dim, N, nc, u0, dt, dx, mask, fv, boundary=None, conditions=None, nv=5, pde=None):
    """candidate of a plain solver step, the limited step of a second solver, the restatement around the candidate -> (cand, got, want)"""
    from exahype_amd import solvers as exa
    kw = dict(dx=[dx] * dim)
    if boundary:
        kw["boundary"] = boundary
    if pde is not None:
        kw.update(pde=pde, n_vars=nv)
    plain = exa.AderDgSolver(dim, N, nc, **kw)
    plain.upload(u0)
    plain.step(dt)
    cand = plain.download().reshape(u0.shape)
    s = exa.AderDgSolver(dim, N, nc, **kw)
    lim = exa.SubcellLimiter(s, capacity=int(np.prod(nc)), fv_mode=exa.FV_MUSCL_HANCOCK)
    s.upload(u0)
    count = lim.step(dt, mask)
    assert int(count) == int(mask.sum())
    got = lim.download().reshape(u0.shape)
    ops = s.operators()
    ops = dict(ops, N=N)
    want = M2.replace_troubled2(u0, cand, mask, dt, [dx] * dim, ops, fv, conditions)
    return cand, got, want


def _check_step(cand, got, want, mask):
    assert np.array_equal(_bits(got[~mask]), _bits(cand[~mask])), "an untroubled cell differs from the plain step"
    assert not np.array_equal(got[mask], cand[mask])
    dim = mask.ndim
    scale = np.max(np.abs(want).reshape(mask.shape + (-1,)), axis=-1).reshape(mask.shape + (1,) * (dim + 1))
    err = float(np.max(np.abs(got - want) / scale))
    print("limited step: rel err %.3e over %d troubled of %d cells" % (err, mask.sum(), mask.size))
    assert err < 1e-10, err


def _mask(nc, seed):
    rng = np.random.default_rng(seed)
    m = rng.random(nc) < 0.5
    m.flat[0], m.flat[-1] = True, False
    return m


@pytest.mark.parametrize("dim,N", [(2, 2), (2, 3), (2, 4), (2, 6), (2, 8), (3, 2), (3, 4), (3, 5)])
def test_one_step_against_the_restatement(dim, N):
    nc = (3, 4) if dim == 2 else (2, 3, 4)
    dx = 0.25
    u0 = euler_dg_state(nc + (N,) * dim, seed=40 + N)
    dt = _cfl_dt(u0, dim, N, dx)
    mask = _mask(nc, N)
    cand, got, want = _one_step(dim, N, nc, u0, dt, dx, mask, M2.fv_update2(dim))
    _check_step(cand, got, want, mask)


def test_one_step_outflow_wall_box():
    from exahype_amd.boundary import Outflow, Wall
    dim, N, nc, dx = 2, 3, (3, 4), 0.25
    boundary = {(0, 0): Wall(), (0, 1): Outflow(), (1, 0): Wall(), (1, 1): Wall()}
    cond = {(0, 0): Wall(KM.wall_sign(2, 0)), (0, 1): Outflow(), (1, 0): Wall(KM.wall_sign(2, 1)), (1, 1): Wall(KM.wall_sign(2, 1))}
    u0 = euler_dg_state(nc + (N,) * dim, seed=61)
    dt = _cfl_dt(u0, dim, N, dx)
    mask = np.ones(nc, dtype=bool)
    mask[1, 1] = mask[1, 2] = False                                # every boundary cell is troubled, the two inner ones are not
    cand, got, want = _one_step(dim, N, nc, u0, dt, dx, mask, M2.fv_update2(dim), boundary, cond)
    _check_step(cand, got, want, mask)


@functools.lru_cache(maxsize=None)
def _swe_muscl_lim():
    from exahype_amd.pde_codegen import SympyPDE
    from tests import user_term_sets as T
    base = T.swe()
    sub = lambda e, qq: e.subs(dict(zip(base.q, qq)), simultaneous=True)     # noqa: E731
    return SympyPDE(base.n_vars, flux=lambda qq, d: [sub(e, qq) for e in base.flux_exprs[d]], max_eigenvalue=lambda qq, d: sub(base.eig_exprs[d], qq),
                    max_dim=base.max_dim, name=base.name + "_muscl_lim", muscl_hancock=True, admissible=lambda q: [q[0]], dmp=(0,))


def test_one_step_generated_shallow_water():
    from oracle import fv_reference as R
    spde = _swe_muscl_lim()
    pid = spde.register()
    dim, N, nc, dx = 2, 3, (3, 3), 0.25
    rng = np.random.default_rng(5)
    shape = nc + (N,) * dim
    u0 = np.stack([1.0 + 0.3 * rng.random(shape), 0.3 * rng.random(shape) - 0.15, 0.3 * rng.random(shape) - 0.15], axis=-1)
    lam = float(np.max(np.abs(u0[..., 1:3] / u0[..., :1]) + np.sqrt(9.81 * u0[..., :1])))
    dt = 0.4 * dx / ((2 * N - 1) * dim * lam)
    mask = _mask(nc, 3)
    fv = M2.fv_update2(dim, 3, pid, terms=R.UserTerms(spde))
    cand, got, want = _one_step(dim, N, nc, u0, dt, dx, mask, fv, nv=3, pde=pid)
    _check_step(cand, got, want, mask)


@pytest.mark.parametrize("dim", [2, 3])
def test_two_a_posteriori_steps_equal_the_restatement(dim):
    from exahype_amd import solvers as exa
    from oracle import aderdg_numpy as A
    from tests import limiter_mood_ref as M
    from tests.test_limiter_a_posteriori import _oscillating_tube
    N, nc = 4, (16,) + (1,) * (dim - 1)
    u, ops = _oscillating_tube(dim, N, nc)
    dx = [1.0 / nc[0]] * dim
    dt = _cfl_dt(u, dim, N, dx[0])
    states, masks = [u], []
    for k in range(2):
        cand = A.step(states[-1], dt, dx, ops, A.Euler())
        mask, margin = M.detect(cand, M.cell_bounds(states[-1]))
        print("step %d: %d of %d troubled, smallest margin %.3e" % (k, mask.sum(), mask.size, margin.min()))
        assert margin.min() >= 1e-9
        states.append(M2.replace_troubled2(states[-1], cand, mask, dt, dx, ops, M2.fv_update2(dim)))
        masks.append(mask)
    assert 0 < masks[0].sum() < masks[0].size
    s = exa.AderDgSolver(dim, N, nc, dx=dx)
    lim = exa.SubcellLimiter(s, capacity=16, fv_mode=exa.FV_MUSCL_HANCOCK)
    s.upload(states[0])
    for k in range(2):
        n = lim.step_a_posteriori(dt)
        assert np.array_equal(lim._mask.cpu().numpy(), masks[k]) and int(n) == int(masks[k].sum())
        got = lim.download()
        err = np.max(np.abs(got - states[k + 1])) / np.max(np.abs(states[k + 1]))
        print("step", k, "rel err %.3e" % err)
        assert err < 1e-10


@pytest.mark.parametrize("dim", [2, 3])
def test_double_sod_tube_through_run_second_order(dim):
    """as tests/test_limiter_a_posteriori.py test_double_sod_tube_through_run, against tests/golden/limiter_muscl_tube.json; the error is below
    the first-order run's of the same case (2-D: tests/golden/limiter_mood_tube.json; 3-D N = 4 is not in that file: "rusanov_l1" of the new one)"""
    import torch
    from exahype_amd import solvers as exa
    from tests import limiter_mood_ref as M
    N, nx = 4, 16
    key = "dim%d_N%d_nx%d" % (dim, N, nx)
    with open(os.path.join(ROOT, "tests", "golden", "limiter_muscl_tube.json")) as f:
        want = json.load(f)["cases"][key]
    with open(os.path.join(ROOT, "tests", "golden", "limiter_mood_tube.json")) as f:
        first = json.load(f)["cases"].get(key, {}).get("l1", want["rusanov_l1"])
    nc = (nx,) + (1,) * (dim - 1)
    s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / nx] * dim)
    lim = exa.SubcellLimiter(s, capacity=16, fv_mode=exa.FV_MUSCL_HANCOCK)
    ops = s.operators()
    u0 = M.tube_initial(N, nx, dim)
    s.upload(u0)
    steps = lim.run(0.1, cfl=0.4, track=True)
    torch.cuda.synchronize()
    st = {k: v.item() for k, v in lim.stats.items()}
    u = lim.download()
    l1 = M.tube_l1(u, ops["xi"], ops["w"], 0.1)
    print("dim %d N %d nx %d: steps %d (restatement %d) L1 %.8f (%.8f; first order %.8f) min rho %.6f (%.6f) min p %.6f (%.6f) troubled <= %d (%d)"
          % (dim, N, nx, steps, want["steps"], l1, want["l1"], first, st["min_rho"], want["min_rho"], st["min_p"], want["min_p"],
             st["max_troubled"], want["max_troubled"]))
    assert st["finite"] and np.isfinite(u).all()
    assert st["min_rho"] > 0 and st["min_p"] > 0
    assert st["max_troubled"] <= 12
    assert abs(s.time - 0.1) < 1e-12
    assert abs(l1 - want["l1"]) <= 0.01 * want["l1"]
    cons = M.defects(M.totals(u0, ops["w"]), M.totals(u, ops["w"]))
    print("cons %s (%s)" % (cons, want["cons"]))
    for v in (0, 4):                                               # mass, energy: the level the DG <-> FV interface allows
        assert abs(cons[v] - want["cons"][v]) <= 0.01 * want["cons"][v], (v, cons[v], want["cons"][v])
    assert max(cons[1:4]) < 1e-12
    assert l1 < first


# ---- refusals, the default ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from exahype_amd import solvers as exa
    from exahype_amd.boundary import Dirichlet
    from tests import user_term_sets as T
    with pytest.raises(ValueError, match="plane streaming"):
        exa.SubcellLimiter(exa.AderDgSolver(3, 6, (2, 1, 1)), capacity=1, fv_mode=exa.FV_MUSCL_HANCOCK)
    s = exa.AderDgSolver(2, 3, (2, 2), one_kernel_step=False)
    lim = exa.SubcellLimiter(s, capacity=4, fv_mode=exa.FV_MUSCL_HANCOCK)
    s.upload(euler_dg_state((2, 2, 3, 3), seed=1))
    for call in (lambda: lim.step(1e-3, np.ones((2, 2), bool), conservative=True), lambda: lim.step_a_posteriori(1e-3, conservative=True),
                 lambda: lim.run(1e-3, conservative=True)):
        with pytest.raises(ValueError, match="fv_mode=FV_RUSANOV"):
            call()
    f = lambda x, t: x[:, :1] * 0 + x.new_tensor([1.0, 0.0, 0.0, 0.0, 2.5])     # noqa: E731
    with pytest.raises(ValueError, match="constant Dirichlet"):
        exa.SubcellLimiter(exa.AderDgSolver(2, 3, (2, 2), boundary={(0, 0): Dirichlet(f)}), capacity=4, fv_mode=exa.FV_MUSCL_HANCOCK)
    pid = T.swe().register()
    with pytest.raises(ValueError, match=r"SympyPDE\(muscl_hancock=True\)"):
        exa.SubcellLimiter(exa.AderDgSolver(2, 3, (2, 2), pde=pid, n_vars=3), capacity=4, fv_mode=exa.FV_MUSCL_HANCOCK)
    with pytest.raises(ValueError, match="fv_mode"):
        exa.SubcellLimiter(s, capacity=4, fv_mode=7)


def test_explicit_rusanov_is_the_default():
    from exahype_amd import solvers as exa
    dim, N, nc = 2, 4, (3, 4)
    u0 = euler_dg_state(nc + (N,) * dim, seed=9)
    dt = _cfl_dt(u0, dim, N, 0.25)
    mask = _mask(nc, 1)
    res = []
    for kw in ({}, dict(fv_mode=exa.FV_RUSANOV)):
        s = exa.AderDgSolver(dim, N, nc, dx=[0.25] * dim)
        lim = exa.SubcellLimiter(s, capacity=12, **kw)
        assert lim.fv_halo == 1
        s.upload(u0)
        lim.step(dt, mask)
        res.append(lim.download())
    assert np.array_equal(_bits(res[0]), _bits(res[1]))

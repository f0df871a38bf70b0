"""A-posteriori (MOOD) subcell limiting: exa_lim_snapshot / exa_lim_detect, SubcellLimiter.detect_candidate / step_a_posteriori / run.

CPU: the two entries exist and fail loudly; the numpy restatement (tests/limiter_mood_ref.py) of the loop keeps a periodic double Sod
tube admissible where the a-priori loop does not, and the committed values of tests/golden/limiter_mood_tube.json come from it.
GPU: snapshot bit for bit, the detector's mask equal to the restatement's in every cell (the inputs keep every decision quantity 1e-9
away from its threshold; asserted on the numpy side), two limited steps to 1e-10, and the tube through run() against the committed
restatement values."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import limiter_mood_ref as M
from tests.test_gpu_distributed import _run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "limiter_mood_tube.json")
MARGIN = 1e-9
gpu = pytest.mark.gpu


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_entries_exported_declared_and_fail_loudly(tmp_path):
    import torch
    from exahype_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "exa_lim_snapshot") and hasattr(lib, "exa_lim_detect")
    src = tmp_path / "use.c"
    src.write_text('#include "exahype_hip.h"\n'
                   'int probe(exa_dg_plan* p, double* u, double* b, unsigned char* m) {\n'
                   '    int kinds[6] = {EXA_LIM_FACE_PERIODIC, EXA_LIM_FACE_GHOST, EXA_LIM_FACE_NONE, 0, 0, 0};\n'
                   '    const double* ghosts[6] = {0, 0, 0, 0, 0, 0};\n'
                   '    return exa_lim_snapshot(p, u, 0, b, 0) + exa_lim_detect(p, u, b, ghosts, kinds, 1e-4, 1e-3, 1e-12, m, 0); }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    buf = (C.c_double * 64)()
    mask = (C.c_ubyte * 64)()
    plan = C.create_string_buffer(4096)                          # stands in for a plan on a machine that cannot create one (device 0, no cells)
    P, B, K = C.cast(plan, C.c_void_p), C.cast(buf, C.c_void_p), C.cast(mask, C.c_void_p)
    for args in ((None, B, None, B, None), (P, None, None, B, None), (P, B, None, None, None), (P, B, B, B, None)):
        assert lib.exa_lim_snapshot(*args) == -1                 # EXA_ERR_INVALID
        assert b"exa_lim_snapshot" in lib.exa_last_error()
    for args in ((None, B, B, K), (P, None, B, K), (P, B, None, K), (P, B, B, None)):
        assert lib.exa_lim_detect(args[0], args[1], args[2], None, None, 1e-4, 1e-3, 1e-12, args[3], None) == -1
        assert b"exa_lim_detect" in lib.exa_last_error()
    if not torch.cuda.is_available():
        assert lib.exa_lim_snapshot(P, B, None, B, None) == -3   # EXA_ERR_NO_DEVICE
        assert lib.exa_lim_detect(P, B, B, None, None, 1e-4, 1e-3, 1e-12, K, None) == -3
        assert b"no CPU fallback" in lib.exa_last_error()


def test_solver_surface():
    from exahype_amd import solvers as exa
    for name in ("step_a_posteriori", "detect_candidate", "run"):
        assert callable(getattr(exa.SubcellLimiter, name))


# the issue's table (CPU probe of the restatement, 2-D): L1(rho), min rho, min p
TABLE = {(4, 16): (0.01895, 0.118, 0.092), (4, 32): (0.01065, 0.118, 0.092), (6, 16): (0.01386, 0.117, 0.090)}


def test_restatement_keeps_the_tube_admissible():
    res = {k: M.run_tube(k[0], k[1], 2) for k in TABLE}
    for (N, nx), r in res.items():
        l1, rho, p = TABLE[(N, nx)]
        print(N, nx, r)
        assert "failed" not in r, r                              # finite after every step
        assert r["min_rho"] > 0 and r["min_p"] > 0
        assert abs(r["l1"] - l1) < 6e-6 and abs(r["min_rho"] - rho) < 1e-3 and abs(r["min_p"] - p) < 1e-3
        assert r["max_troubled"] <= 8
        assert r["cons"][1] < 1e-12 and r["cons"][2] < 1e-12 and r["cons"][3] < 1e-12
    assert res[(4, 32)]["l1"] < res[(4, 16)]["l1"]


def test_a_priori_loop_leaves_the_admissible_states():
    """Why the feature exists: detect(u^n) -> step at p = 5 on 16 cells ends with negative density (the issue's probe: min rho = -0.73)."""
    r = M.run_tube(6, 16, 2, a_priori=True)
    print(r)
    assert r["min_rho"] < 0 or "failed" in r
    assert r["min_rho"] < 0


def test_golden_values_come_from_the_restatement():
    g = _golden()
    assert sorted(g) == sorted("dim%d_N%d_nx%d" % c for c in [(2, 4, 16), (2, 4, 32), (2, 4, 64), (3, 6, 16), (3, 6, 32), (3, 8, 16), (3, 8, 32)])
    r = M.run_tube(4, 16, 2)
    want = g["dim2_N4_nx16"]
    assert r["steps"] == want["steps"] and r["max_troubled"] == want["max_troubled"]
    for k in ("l1", "min_rho", "min_p"):
        assert abs(r[k] - want[k]) <= 1e-9 * abs(want[k]), k
    for v in g.values():
        assert "failed" not in v and v["min_rho"] > 0 and v["min_p"] > 0 and v["max_troubled"] <= 8


def test_example_exact_solution_is_the_restatements():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import importlib
        ex = importlib.import_module("sod_tube_limited")
    finally:
        sys.path.pop(0)
    x = np.linspace(0.0, 1.0, 977, endpoint=False)
    assert np.allclose(ex.exact_density(x, 0.1), M.exact_double(x, 0.1), rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _level_state(dim, N, nc, seed, noise=0.01):
    """Admissible Euler state, different level per cell (rho in [0.5, 2], p in [0.5, 2]) with node-wise noise"""
    rng = np.random.default_rng(seed)
    shape = tuple(nc) + (N,) * dim
    cell = tuple(nc) + (1,) * dim
    rho = rng.uniform(0.5, 2.0, cell) + noise * rng.random(shape)
    p = rng.uniform(0.5, 2.0, cell) + noise * rng.random(shape)
    vel = [rng.uniform(-0.3, 0.3, cell) + noise * rng.random(shape) for _ in range(3)]
    u = np.zeros(shape + (5,))
    u[..., 0] = rho
    for a in range(3):
        u[..., 1 + a] = rho * vel[a]
    u[..., 4] = p / 0.4 + 0.5 * rho * sum(v * v for v in vel)
    return u


def _perturbed(old, dim, seed):
    """candidate = old + per-cell amplitude x node noise on rho and E, amplitudes from far below to far above the DMP slack"""
    rng = np.random.default_rng(seed)
    nc = old.shape[:dim]
    amp = rng.choice([0.0, 1e-5, 3e-4, 0.02, 0.3], size=nc).reshape(nc + (1,) * dim)
    cand = old.copy()
    cand[..., 0] += amp * rng.uniform(-1, 1, old.shape[:-1])
    cand[..., 4] += amp * rng.uniform(-1, 1, old.shape[:-1])
    return cand


def _gpu_mask(dim, N, nc, old, cand, boundary=None, **kw):
    from exahype_amd import solvers as exa
    s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / nc[0]] * dim, boundary=boundary)
    lim = exa.SubcellLimiter(s, capacity=4)
    s.upload(cand)
    return lim.detect_candidate(old, **kw).cpu().numpy()


def _check_mask(dim, N, nc, old, cand, boundary=None, no_neighbour=(), expect=None):
    want, margin = M.detect(cand, M.cell_bounds(old), no_neighbour=no_neighbour)
    print("dim %d N %d nc %s: %d of %d troubled, smallest margin %.3e" % (dim, N, nc, want.sum(), want.size, margin.min()))
    assert margin.min() >= MARGIN                                # no cell may be excused
    if expect is not None:
        assert np.array_equal(want, expect), "the case does not decide what it was built to decide"
    got = _gpu_mask(dim, N, nc, old, cand, boundary)
    assert got.dtype == np.bool_ and got.shape == tuple(nc)
    assert np.array_equal(got, want), np.argwhere(got != want)
    return want


DETECT_SHAPES = [(2, 3, (5, 3)), (2, 4, (3, 4)), (2, 8, (2, 3)), (3, 3, (3, 2, 4)), (3, 4, (2, 3, 2)), (3, 6, (3, 1, 2)), (3, 8, (2, 3, 1))]


@gpu
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("N", [3, 4, 6, 8])
def test_snapshot_bit_for_bit(dim, N):
    import torch
    from exahype_amd import solvers as exa
    nc = (5, 3) if dim == 2 else (3, 2, 3)
    u = _level_state(dim, N, nc, 100 * dim + N, noise=0.3)
    s = exa.AderDgSolver(dim, N, nc)
    s.upload(u)
    ncell = int(np.prod(nc))
    for with_copy in (True, False):
        old = torch.full_like(s.u, -7.25)
        bounds = torch.full((ncell + 1, 4), -7.25, dtype=torch.float64, device=s.dev)
        exa.check(s.lib.exa_lim_snapshot(s._plan, C.c_void_p(s.u.data_ptr()), C.c_void_p(old.data_ptr()) if with_copy else None,
                                         C.c_void_p(bounds.data_ptr()), None))
        torch.cuda.synchronize()
        b = bounds.cpu().numpy()
        assert np.array_equal(b[:ncell].reshape(tuple(nc) + (4,)), M.cell_bounds(u))
        assert np.all(b[ncell] == -7.25)                           # nothing beyond the last cell
        assert np.array_equal(s.u.cpu().numpy(), u)
        o = old.cpu().numpy()
        assert np.array_equal(o, u) if with_copy else np.all(o == -7.25)


@gpu
@pytest.mark.parametrize("dim,N,nc", DETECT_SHAPES)
def test_detector_smooth_state_is_clean(dim, N, nc):
    old = _level_state(dim, N, (1,) * dim, 7, noise=0.0)           # one level everywhere ...
    old = np.broadcast_to(old, tuple(nc) + old.shape[dim:]).copy()
    x = np.linspace(0, 1, old[..., 0].size, endpoint=False).reshape(old.shape[:-1])
    old[..., 0] *= 1 + 0.05 * np.sin(2 * np.pi * x)                # ... with a smooth variation
    cand = old * (1 + 1e-6 * np.cos(2 * np.pi * x))[..., None]
    _check_mask(dim, N, nc, old, cand, expect=np.zeros(nc, dtype=bool))


@gpu
@pytest.mark.parametrize("dim,N,nc", DETECT_SHAPES)
def test_detector_random_perturbations(dim, N, nc):
    old = _level_state(dim, N, nc, 11 * N + dim)
    want = _check_mask(dim, N, nc, old, _perturbed(old, dim, 5 * N + dim))
    assert 0 < want.sum() < want.size or want.size < 4


@gpu
@pytest.mark.parametrize("dim,N,nc", DETECT_SHAPES)
def test_detector_single_defects(dim, N, nc):
    """one defect in one cell each: a single-node overshoot, negative pressure, a NaN, an inf; every other cell stays clean"""
    old = _level_state(dim, N, (1,) * dim, 3, noise=0.0)
    old = np.broadcast_to(old, tuple(nc) + old.shape[dim:]).copy()
    cells = [tuple(int(i) for i in np.unravel_index(k, nc)) for k in np.linspace(0, np.prod(nc) - 1, 5).astype(int)]
    last, mid = (N - 1,) * dim, (N // 2,) * dim
    for k, name in enumerate(("overshoot", "undershoot E", "negative pressure", "NaN", "inf")):
        cand = old.copy()
        c = cells[k]
        if name == "overshoot":
            cand[c + last + (0,)] += 0.01                          # rho at one node (the last of the cell)
        elif name == "undershoot E":
            cand[c + mid + (4,)] -= 0.01
        elif name == "negative pressure":
            cand[c + (0,) * dim + (1,)] = 3.0 * np.sqrt(cand[c + (0,) * dim + (0,)] * cand[c + (0,) * dim + (4,)])    # |m|^2 / (2 rho) = 4.5 E
        elif name == "NaN":
            cand[c + last + (2,)] = np.nan                         # in a momentum: only the finiteness check and p see it
        else:
            cand[c + mid + (3,)] = -np.inf
        expect = np.zeros(nc, dtype=bool)
        expect[c] = True
        _check_mask(dim, N, nc, old, cand, expect=expect)


@gpu
@pytest.mark.parametrize("dim,N,nc", [(2, 4, (4, 3)), (3, 3, (3, 2, 4)), (3, 6, (2, 5, 3))])
def test_detector_jump_at_the_periodic_wrap(dim, N, nc):
    """Old state: high density in the LAST layer of an axis (every axis in turn), a quarter of it elsewhere.  A candidate value between the two
    levels is inside the bounds only in cells with the high layer across a face: the layer before it, and the FIRST layer -- across the wrap."""
    for axis in range(dim):
        base = _level_state(dim, N, (1,) * dim, 3, noise=0.0)
        old = np.broadcast_to(base, tuple(nc) + base.shape[dim:]).copy()
        rho_hi = float(base[(0,) * (2 * dim) + (0,)])
        low = [slice(None)] * dim
        low[axis] = slice(0, nc[axis] - 1)
        old[tuple(low)] *= 0.25                                     # every variable: the same velocity, a quarter of the pressure
        cand = old.copy()
        cand[tuple(low) + (0,) * dim + (0,)] = 0.6 * rho_hi         # one node of every low cell
        expect = np.zeros(nc, dtype=bool)
        if nc[axis] > 3:
            mid = [slice(None)] * dim
            mid[axis] = slice(1, nc[axis] - 2)
            expect[tuple(mid)] = True
        _check_mask(dim, N, nc, old, cand, expect=expect)


@gpu
@pytest.mark.parametrize("dim,N,nc", [(2, 4, (4, 3)), (3, 3, (3, 3, 4)), (3, 8, (3, 4, 3))])
def test_detector_outflow_wall_dirichlet_faces(dim, N, nc):
    """A face with a condition has no neighbour: the cells of the last layer, raised at one node towards the level of the first layer, are
    within bounds on the periodic grid (the first layer is their neighbour across the wrap) and troubled with conditions at both ends."""
    from exahype_amd.boundary import Dirichlet, Outflow, Wall
    for axis in range(dim):
        old = _level_state(dim, N, nc, 17 + axis)
        first, lastl = [slice(None)] * dim, [slice(None)] * dim
        first[axis], lastl[axis] = 0, nc[axis] - 1
        old[tuple(first)] *= 8.0                                    # rho >= 4 there, <= 2.01 elsewhere
        cand = _perturbed(old, dim, 23 + axis)
        cand[tuple(lastl)] = old[tuple(lastl)]
        cand[tuple(lastl) + (0,) * dim + (0,)] = 3.0
        far = np.array([1.0, 0.0, 0.0, 0.0, 2.5])
        conds = [(Outflow(), Wall()), (Wall(), Dirichlet(far)), (Dirichlet(far), Outflow())][axis]
        boundary = {(axis, 0): conds[0], (axis, 1): conds[1]}
        per = _check_mask(dim, N, nc, old, cand)
        bc = _check_mask(dim, N, nc, old, cand, boundary=boundary, no_neighbour={(axis, 0), (axis, 1)})
        assert bc[tuple(lastl)].all() and not per[tuple(lastl)].any()


DETECT_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from exahype_amd import solvers as exa
from tests import limiter_mood_ref as M
from tests.test_limiter_a_posteriori import _level_state, _perturbed
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
dim, N, nc, pdims = %(dim)d, %(N)d, %(nc)r, %(pdims)r
part = exa.CartesianPartition(world, rank, dim, pdims)
Gr = tuple(nc[a] * part.pdims[a] for a in range(dim))
old = _level_state(dim, N, Gr, 31)
cand = _perturbed(old, dim, 37)
# troubled cells on the block face: the layers either side of it are raised / lowered beyond what their own block allows
ax = [a for a in range(dim) if part.pdims[a] > 1][0]
lo_layer, hi_layer = [slice(None)] * dim, [slice(None)] * dim
lo_layer[ax], hi_layer[ax] = nc[ax], nc[ax] - 1
cand[tuple(lo_layer) + (0,) * dim + (0,)] = 1.5 * old[..., 0].max()
cand[tuple(hi_layer) + (0,) * dim + (4,)] = 0.5 * old[..., 4].min()
want, margin = M.detect(cand, M.cell_bounds(old))
assert margin.min() >= 1e-9, margin.min()
assert want[tuple(lo_layer)].all() and want[tuple(hi_layer)].all() and not want.all()
s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / Gr[0]] * dim, part=part, backend_is_gloo=True)
lim = exa.SubcellLimiter(s, capacity=4)
sl = tuple(slice(part.coords[a] * nc[a], (part.coords[a] + 1) * nc[a]) for a in range(dim))
s.upload(cand[sl])
got = lim.detect_candidate(old[sl]).cpu().numpy()
assert np.array_equal(got, want[sl]), (rank, np.argwhere(got != want[sl]))
# the block alone, periodic in itself, decides differently: the exchange is what the comparison saw
alone, _ = M.detect(cand[sl], M.cell_bounds(old[sl]))
print("rank", rank, "troubled", int(got.sum()), "of", got.size, "differs from the block alone in", int((alone != want[sl]).sum()), "cells")
dist.barrier(); dist.destroy_process_group()
'''


@gpu
@pytest.mark.parametrize("dim,N,nc,pdims", [(2, 4, (3, 3), [2, 1]), (3, 3, (2, 2, 3), [1, 2, 1]), (3, 8, (2, 2, 2), [2, 1, 1])])
def test_detector_on_two_ranks(tmp_path, dim, N, nc, pdims):
    _run_ranks(tmp_path, DETECT_WORKER % dict(root=ROOT, dim=dim, N=N, nc=nc, pdims=pdims), 2)


def _oscillating_tube(dim, N, nc):
    """Sod-like: the tube's two levels along x with a cell-internal oscillation of density and pressure, so that the DG candidate of the first
    step already leaves the bounds next to the jumps"""
    ops = M.operators(N)
    u = M.tube_initial(N, nc[0], dim)
    u = np.broadcast_to(u, tuple(nc) + u.shape[dim:]).copy()
    xi = np.asarray(ops["xi"])
    osc = 1.0
    for a in range(dim):
        sh = [1] * (2 * dim)
        sh[dim + a] = N
        osc = osc * (1 + 0.03 * np.sin(2 * np.pi * (xi + 0.1 * a))).reshape(sh)
    cellph = np.cos(1.7 * np.arange(int(np.prod(nc)))).reshape(tuple(nc) + (1,) * dim)
    u[..., 0] *= 1 + (osc - 1) * cellph
    u[..., 4] *= 1 + 0.5 * (osc - 1) * cellph
    return u, ops


def _step_parity_reference(dim, N, G):
    u, ops = _oscillating_tube(dim, N, G)
    dx = [1.0 / G[0]] * dim
    lam = max(np.max(M.A.Euler().maxeig(u, d)) for d in range(dim))
    dt = 0.4 * dx[0] / ((2 * N - 1) * dim * lam)
    states, masks = [u], []
    for k in range(2):
        cand = M.A.step(states[-1], dt, dx, ops, M.A.Euler())
        mask, margin = M.detect(cand, M.cell_bounds(states[-1]))
        print("step %d: %d of %d troubled, smallest margin %.3e" % (k, mask.sum(), mask.size, margin.min()))
        assert margin.min() >= MARGIN
        states.append(M.replace_troubled(states[-1], cand, mask, dt, dx, ops))
        masks.append(mask)
    assert 0 < masks[0].sum() < masks[0].size                      # non-trivial in step 1
    return states, masks, dt, dx


@gpu
@pytest.mark.parametrize("dim,N,nc", [(2, 4, (8, 2)), (3, 4, (8, 1, 2)), (3, 8, (8, 2, 1))])
def test_two_steps_equal_the_restatement(dim, N, nc):
    from exahype_amd import solvers as exa
    states, masks, dt, dx = _step_parity_reference(dim, N, nc)
    s = exa.AderDgSolver(dim, N, nc, dx=dx)
    lim = exa.SubcellLimiter(s, capacity=int(np.prod(nc)))
    s.upload(states[0])
    for k in range(2):
        n = lim.step_a_posteriori(dt)
        assert np.array_equal(lim._mask.cpu().numpy(), masks[k])
        assert int(n) == int(masks[k].sum())
        got = lim.download()
        err = np.max(np.abs(got - states[k + 1])) / np.max(np.abs(states[k + 1]))
        print("step", k, "rel err %.3e" % err)
        assert err < 1e-10
    assert abs(s.time - 2 * dt) < 1e-15


STEP_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from exahype_amd import solvers as exa
from tests.test_limiter_a_posteriori import _step_parity_reference
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
dim, N, nc, pdims = %(dim)d, %(N)d, %(nc)r, %(pdims)r
part = exa.CartesianPartition(world, rank, dim, pdims)
Gr = tuple(nc[a] * part.pdims[a] for a in range(dim))
states, masks, dt, dx = _step_parity_reference(dim, N, Gr)
s = exa.AderDgSolver(dim, N, nc, dx=dx, part=part, backend_is_gloo=True)
lim = exa.SubcellLimiter(s, capacity=int(np.prod(nc)))
sl = tuple(slice(part.coords[a] * nc[a], (part.coords[a] + 1) * nc[a]) for a in range(dim))
s.upload(states[0][sl])
for k in range(2):
    n = lim.step_a_posteriori(dt)
    assert np.array_equal(lim._mask.cpu().numpy(), masks[k][sl]), (rank, k)
    assert int(n) == int(masks[k][sl].sum())
    got, want = lim.download(), states[k + 1][sl]
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    assert err < 1e-10, (rank, k, err)
    print("rank", rank, "step", k, "troubled", int(n), "rel err", err)
dist.barrier(); dist.destroy_process_group()
'''


@gpu
def test_two_steps_on_two_ranks(tmp_path):
    """8 x 2 cells as two blocks of 4 x 2: the tube's jumps (x = 0.25, 0.75) lie inside the blocks, their troubled neighbourhoods reach the block faces"""
    _run_ranks(tmp_path, STEP_WORKER % dict(root=ROOT, dim=2, N=4, nc=(4, 2), pdims=[2, 1]), 2)


@gpu
def test_refuses_the_fused_solver_modes():
    from exahype_amd import solvers as exa
    s = exa.AderDgSolver(3, 6, (2, 2, 2), stage_a="reg", one_kernel_step=True)
    lim = exa.SubcellLimiter(s, capacity=4)
    with pytest.raises(ValueError, match="two-kernel"):
        lim.step_a_posteriori(1e-3)
    s = exa.AderDgSolver(2, 4, (4, 4), n_picard=0)
    if s._fused:
        with pytest.raises(ValueError, match="two-kernel"):
            exa.SubcellLimiter(s, capacity=4).run(1e-3)


TUBE_CASES = {(2, 4): (16, 32, 64), (3, 6): (16, 32), (3, 8): (16, 32)}


@gpu
@pytest.mark.parametrize("dim,N", sorted(TUBE_CASES))
def test_double_sod_tube_through_run(dim, N):
    """Periodic double Sod tube along x on nx x 1 (x 1) cells, t_end = 0.1, CFL 0.4, against the restatement's committed values (3-D: the
    restatement ran on nx x 1 x 1 cells as well)."""
    import torch
    from exahype_amd import solvers as exa
    golden = _golden()
    l1s = []
    for nx in TUBE_CASES[(dim, N)]:
        want = golden["dim%d_N%d_nx%d" % (dim, N, nx)]
        nc = (nx,) + (1,) * (dim - 1)
        s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / nx] * dim)
        lim = exa.SubcellLimiter(s, capacity=16)                   # an overflow fails the run
        ops = s.operators()
        u0 = M.tube_initial(N, nx, dim)
        s.upload(u0)
        steps = lim.run(0.1, cfl=0.4, track=True)
        torch.cuda.synchronize()
        st = {k: v.item() for k, v in lim.stats.items()}
        u = lim.download()
        l1 = M.tube_l1(u, ops["xi"], ops["w"], 0.1)
        cons = M.defects(M.totals(u0, ops["w"]), M.totals(u, ops["w"]))
        print("dim %d N %d nx %d: steps %d (restatement %d) L1 %.8f (%.8f) min rho %.6f (%.6f) min p %.6f (%.6f) troubled <= %d (%d) cons %s (%s)"
              % (dim, N, nx, steps, want["steps"], l1, want["l1"], st["min_rho"], want["min_rho"], st["min_p"], want["min_p"],
                 st["max_troubled"], want["max_troubled"], cons, want["cons"]))
        assert st["finite"] and np.isfinite(u).all()               # every step
        assert st["min_rho"] > 0 and st["min_p"] > 0               # every step, every node
        assert st["max_troubled"] <= 12
        assert abs(s.time - 0.1) < 1e-12
        assert abs(l1 - want["l1"]) <= 0.01 * want["l1"]
        for v in (0, 4):                                           # mass, energy: the level the DG <-> FV interface allows
            assert abs(cons[v] - want["cons"][v]) <= 0.01 * want["cons"][v], (v, cons[v], want["cons"][v])
        assert max(cons[1:4]) < 1e-12
        l1s.append(l1)
    assert all(b < a for a, b in zip(l1s, l1s[1:])), l1s


@gpu
def test_example_runs(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "sod_tube_limited.py"), "16", "4", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    l1 = float(r.stdout.strip().splitlines()[-1].split("=")[1])
    want = _golden()["dim2_N4_nx16"]["l1"]
    assert abs(l1 - want) <= 0.01 * want

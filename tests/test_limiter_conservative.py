"""Conservative DG / FV interface of the a-posteriori subcell limiter: exa_lim_face_flux / exa_lim_interface_correct,
SubcellLimiter.step(conservative=True), step_a_posteriori(conservative=True, rounds=) and run.

CPU: the reconstruction keeps the mean (w R = 1 / Ns); the numpy restatement (tests/limiter_conservative_ref.py) holds the tube's totals to
the rounding bound where the unmodified loop loses 1e-3; one round is not enough at p = 7, three are; the entries exist and fail loudly.
GPU: the FV face fluxes element by element and one conservative step against the restatement (1e-10), the totals of that step against the
bound, a step of three rounds with the cumulative mask equal in every cell, and the tube through run() against the committed values.

The conservation bound is 16 steps 2^-53 in the normalisation of limiter_mood_ref.defects: a step changes each total by roundings of order
2^-53 of it, 16 is the margin.  The totals of the one-step tests are summed in long double, so that the measurement adds none of its own."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from tests import limiter_conservative_ref as K
from tests import limiter_mood_ref as M
from tests.test_gpu_distributed import _run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "limiter_conservative_tube.json")
MARGIN = 1e-9
gpu = pytest.mark.gpu


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", range(2, 9))
def test_reconstruction_keeps_the_mean(N):
    """w R = 1 / Ns: the face mean of (R x R) g is the mean of g, which is what makes the lifted correction conservative"""
    ops = M.operators(N)
    P, R = K.limiter_matrices(ops)
    Ns = 2 * N - 1
    assert R.shape == (N, Ns)
    assert np.max(np.abs(np.asarray(ops["w"]) @ R - 1.0 / Ns)) <= 8 * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _tube(N, nx, dim, rounds):
    return K.run_tube(N, nx, dim, rounds=rounds)


def test_restatement_conserves_the_tube_to_rounding():
    r = _tube(4, 16, 2, 3)
    print(r, "bound %.3e" % K.bound(r["steps"]))
    assert "failed" not in r and r["steps"] == 118
    assert r["cons"][0] <= K.bound(r["steps"]) and r["cons"][4] <= K.bound(r["steps"])
    assert max(r["cons"]) <= K.bound(r["steps"])
    assert r["min_rho"] > 0 and r["min_p"] > 0 and r["unresolved"] == 0


def test_unmodified_loop_loses_mass_and_energy():
    """the same case through limiter_mood_ref.run_tube as it stands: the bound can fail"""
    r = M.run_tube(4, 16, 2)
    print(r)
    assert r["cons"][0] > 1e-3 and r["cons"][4] > 1e-3


def test_one_round_is_not_enough_at_p7():
    one, three = _tube(8, 16, 2, 1), _tube(8, 16, 2, 3)
    print(one, three, sep="\n")
    assert one["unresolved"] > 0
    assert "failed" not in three and three["unresolved"] == 0 and three["min_p"] > 0 and three["min_rho"] > 0


def test_golden_values_come_from_the_restatement():
    g = _golden()
    assert {"dim2_N4_nx16", "dim2_N8_nx16", "dim3_N6_nx16"} <= set(g)
    for name, r in (("dim2_N4_nx16", _tube(4, 16, 2, 3)), ("dim2_N8_nx16", _tube(8, 16, 2, 3))):
        want = g[name]
        assert r["steps"] == want["steps"] and r["max_troubled"] == want["max_troubled"] and r["unresolved"] == want["unresolved"]
        for k in ("l1", "min_rho", "min_p"):
            assert abs(r[k] - want[k]) <= 1e-9 * abs(want[k]), k
    for name, v in g.items():
        assert "failed" not in v and v["min_rho"] > 0 and v["min_p"] > 0, name
        assert max(v["cons"]) <= K.bound(v["steps"]), name           # at rounding level in every committed case
        assert len(v["cons"]) == 5


def test_entries_exported_and_fail_loudly():
    import torch
    from exahype_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "exa_lim_face_flux") and hasattr(lib, "exa_lim_interface_correct") and hasattr(lib, "exa_lim_face_flux_count")
    buf = (C.c_double * 64)()
    cells = (C.c_long * 8)()
    mask = (C.c_ubyte * 64)()
    plan = C.create_string_buffer(4096)                          # stands in for a plan on a machine that cannot create one (device 0, no cells)
    P, B, L, K_ = C.cast(plan, C.c_void_p), C.cast(buf, C.c_void_p), C.cast(cells, C.c_void_p), C.cast(mask, C.c_void_p)
    dx = (C.c_double * 3)(1.0, 1.0, 1.0)
    for args in ((None, B, L, 1, B), (P, None, L, 1, B), (P, B, None, 1, B), (P, B, L, 1, None), (P, B, L, -1, B)):
        assert lib.exa_lim_face_flux(*args, None) == -1          # EXA_ERR_INVALID
        assert b"exa_lim_face_flux" in lib.exa_last_error()
    for args in ((None, B, B, L, 1, K_, None, B, 0.1, dx), (P, None, B, L, 1, K_, None, B, 0.1, dx), (P, B, None, L, 1, K_, None, B, 0.1, dx),
                 (P, B, B, None, 1, K_, None, B, 0.1, dx), (P, B, B, L, 1, None, None, B, 0.1, dx), (P, B, B, L, 1, K_, None, None, 0.1, dx),
                 (P, B, B, L, 1, K_, None, B, 0.1, None)):
        assert lib.exa_lim_interface_correct(*args, None) == -1
        assert b"exa_lim_interface_correct" in lib.exa_last_error()
    if not torch.cuda.is_available():
        assert lib.exa_lim_face_flux(P, B, L, 1, B, None) == -3  # EXA_ERR_NO_DEVICE
        assert b"no CPU fallback" in lib.exa_last_error()
        assert lib.exa_lim_interface_correct(P, B, B, L, 1, K_, None, B, 0.1, dx, None) == -3
        assert b"no CPU fallback" in lib.exa_last_error()


def test_solver_surface():
    import inspect
    from exahype_amd import solvers as exa
    for name, args in (("step", ("conservative",)), ("step_a_posteriori", ("conservative", "rounds")), ("run", ("conservative", "rounds"))):
        sig = inspect.signature(getattr(exa.SubcellLimiter, name))
        for a in args:
            assert a in sig.parameters, (name, a)
        assert sig.parameters["conservative"].default is False
    assert inspect.signature(exa.SubcellLimiter.run).parameters["rounds"].default == 3


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
GRIDS = {2: (3, 2), 3: (2, 2, 3)}
ORDERS = [2, 3, 4, 6, 8]


def _masks(dim):
    """name -> (grid, troubled cells)"""
    g = GRIDS[dim]
    if dim == 2:
        return {"single": (g, [(1, 0)]), "adjacent": (g, [(0, 1), (1, 1)]), "same_neighbour": ((2, 3), [(1, 2)]),
                "all": (g, list(np.ndindex(*g)))}
    return {"single": (g, [(0, 1, 1)]), "adjacent": (g, [(1, 0, 1), (1, 0, 2)]), "same_neighbour": (g, [(1, 0, 0)]),
            "all": (g, list(np.ndindex(*g)))}


def _mask_array(grid, cells):
    m = np.zeros(grid, dtype=bool)
    for c in cells:
        m[c] = True
    return m


def _state(dim, N, nc, seed):
    """A smooth positive Euler state with node-wise noise and one jump: the layer c_0 = 0 holds 0.4 times the density and pressure"""
    rng = np.random.default_rng(seed)
    ops = M.operators(N)
    xi = np.asarray(ops["xi"])
    shape = tuple(nc) + (N,) * dim
    ph = 0.0
    for a in range(dim):
        cs, ns = [1] * (2 * dim), [1] * (2 * dim)
        cs[a], ns[dim + a] = nc[a], N
        ph = ph + (a + 1) * (np.arange(nc[a]).reshape(cs) + xi.reshape(ns)) / nc[a]
    rho = 1.0 + 0.2 * np.sin(2 * np.pi * ph) + 0.02 * rng.random(shape)
    p = 1.0 + 0.1 * np.cos(2 * np.pi * ph) + 0.02 * rng.random(shape)
    rho[0] *= 0.4
    p[0] *= 0.4
    vel = [0.3 * np.cos(2 * np.pi * ph + a) + 0.02 * rng.random(shape) for a in range(3)]
    u = np.zeros(shape + (5,))
    u[..., 0] = rho
    for a in range(3):
        u[..., 1 + a] = rho * vel[a]
    u[..., 4] = p / 0.4 + 0.5 * rho * sum(v * v for v in vel)
    return u, ops


def _dt(u, dx, dim, N):
    lam = max(np.max(M.A.Euler().maxeig(u, d)) for d in range(dim))
    return 0.4 * dx[0] / ((2 * N - 1) * dim * lam)


EULER_SIGN = {0: np.array([1.0, -1, 1, 1, 1]), 1: np.array([1.0, 1, -1, 1, 1]), 2: np.array([1.0, 1, 1, -1, 1])}
BOX = {(0, 0): "outflow", (0, 1): "wall", (1, 0): "wall", (1, 1): "outflow"}          # (axis 2, if any: periodic)


def _bcs(box):
    """(the solver's boundary dict, the restatement's)"""
    from exahype_amd.boundary import Outflow, Wall
    if not box:
        return None, None
    return ({k: Outflow() if v == "outflow" else Wall() for k, v in BOX.items()},
            {k: ("outflow",) if v == "outflow" else ("wall", EULER_SIGN[k[0]]) for k, v in BOX.items()})


@functools.lru_cache(maxsize=None)
def _reference(dim, N, name, box, conservative=True):
    """(u, mask, dt, dx, u_new, F~ per (cell, axis, side)) of one step with the given mask, computed once and shared"""
    grid, cells = _masks(dim)[name]
    u, ops = _state(dim, N, grid, 100 * dim + N)
    dx = [1.0 / grid[0]] * dim
    dt = _dt(u, dx, dim, N)
    mask = _mask_array(grid, cells)
    fluxes = {}
    new = K.step_with_mask(u, mask, dt, dx, ops, _bcs(box)[1], conservative=conservative, fluxes=fluxes)
    for a in (mask, new):
        a.setflags(write=False)
    return u, mask, dt, dx, new, fluxes


def _limiter(dim, N, grid, dx, box=False, extra=2):
    from exahype_amd import solvers as exa
    s = exa.AderDgSolver(dim, N, grid, dx=dx, boundary=_bcs(box)[0])
    return s, exa.SubcellLimiter(s, capacity=int(np.prod(grid)) + extra)


@gpu
@pytest.mark.parametrize("name", ["single", "adjacent", "same_neighbour", "all"])
@pytest.mark.parametrize("N", ORDERS)
@pytest.mark.parametrize("dim", [2, 3])
def test_face_flux_equals_the_restatement(dim, N, name):
    """every element of fvflux[slot][d*2+side][var][node] of the listed slots; the -1 slots behind them keep the sentinel"""
    import torch
    u, mask, dt, dx, _, fluxes = _reference(dim, N, name, False)
    s, lim = _limiter(dim, N, mask.shape, dx)
    s.upload(u)
    lim._conservative_setup("step")
    m = torch.as_tensor(np.array(mask.reshape(-1))).to(s.dev)
    lim._compact(m)
    lim._project(m, s.u, s.time)
    lim._fvflux.fill_(-7.25)
    lim._face_flux()
    torch.cuda.synchronize()
    got = lim._fvflux.cpu().numpy().reshape(lim.capacity, 2 * dim, 5, N ** (dim - 1))
    cells = list(zip(*np.nonzero(mask)))                           # the compacted list is in the order of the flat cell index
    scale = max(np.max(np.abs(f)) for f in fluxes.values())
    worst = 0.0
    for slot, idx in enumerate(cells):
        for a in range(dim):
            for side in range(2):
                want = np.moveaxis(fluxes[(idx, a, side)].reshape(-1, 5), -1, 0)
                worst = max(worst, float(np.max(np.abs(got[slot, a * 2 + side] - want))))
    print("dim %d N %d %s: %d slots, max |g| %.3e, worst error %.3e" % (dim, N, name, len(cells), scale, worst))
    assert worst <= 1e-10 * scale
    assert np.all(got[len(cells):] == -7.25)                       # empty slots: nothing written
    assert lim.capacity > len(cells) or name == "all"             # (every other mask leaves -1 slots)


@gpu
@pytest.mark.parametrize("box", [False, True], ids=["periodic", "outflow_wall"])
@pytest.mark.parametrize("name", ["single", "adjacent", "same_neighbour", "all"])
@pytest.mark.parametrize("N", ORDERS)
@pytest.mark.parametrize("dim", [2, 3])
def test_one_conservative_step_equals_the_restatement(dim, N, name, box):
    u, mask, dt, dx, want, _ = _reference(dim, N, name, box)
    s, lim = _limiter(dim, N, mask.shape, dx, box)
    s.upload(u)
    n = lim.step(dt, mask, conservative=True)
    got = lim.download()
    assert int(n) == int(mask.sum())
    err = np.max(np.abs(got - want), axis=tuple(range(dim, 2 * dim + 1)))
    print("dim %d N %d %s box %s: worst cell error %.3e of max |u| %.3e" % (dim, N, name, box, err.max(), np.max(np.abs(want))))
    assert np.all(err <= 1e-10 * np.max(np.abs(want))), np.argwhere(err > 1e-10 * np.max(np.abs(want)))
    if name != "all":
        # the correction is what was compared: without it the same step differs from the restatement by far more than the tolerance
        plain = K.step_with_mask(u, mask, dt, dx, M.operators(N), _bcs(box)[1], conservative=False)
        assert np.max(np.abs(plain - want)) > 1e-6 * np.max(np.abs(want))


def _totals_ld(u, w):
    dim = M._dim(u)
    v = u.astype(np.longdouble)
    wl = np.asarray(w).astype(np.longdouble)
    for _ in range(dim):
        v = np.tensordot(v, wl, axes=([dim], [0]))
    return v.reshape(-1, u.shape[-1]).sum(0)


def _defects_ld(m0, m1):
    return [float(abs(a - b) / max(abs(a), 1.0)) for a, b in zip(m0, m1)]


@gpu
@pytest.mark.parametrize("name", ["single", "adjacent", "same_neighbour", "all"])
@pytest.mark.parametrize("N", ORDERS)
@pytest.mark.parametrize("dim", [2, 3])
def test_one_conservative_step_keeps_the_totals(dim, N, name):
    """Periodic box: the relative defect of every variable stays within the bound of one step; the same call without the correction loses
    more than 1e-6 (the single-cell mask)."""
    u, mask, dt, dx, _, _ = _reference(dim, N, name, False)
    w = M.operators(N)["w"]
    s, lim = _limiter(dim, N, mask.shape, dx)
    s.upload(u)
    lim.step(dt, mask, conservative=True)
    d = _defects_ld(_totals_ld(u, w), _totals_ld(lim.download(), w))
    print("dim %d N %d %s: defects %s, bound %.3e" % (dim, N, name, ["%.2e" % x for x in d], K.bound(1)))
    assert max(d) <= K.bound(1), d
    if name == "single":
        s.upload(u)
        s.time = 0.0
        lim.step(dt, mask)
        d0 = _defects_ld(_totals_ld(u, w), _totals_ld(lim.download(), w))
        print("   without the correction: %s" % ["%.2e" % x for x in d0])
        assert max(d0) > 1e-6, d0


@gpu
@pytest.mark.parametrize("dim,N,nc", [(2, 4, (8, 2)), (3, 6, (8, 1, 2))])
def test_rounds_equal_the_restatement(dim, N, nc):
    """two tube steps of three rounds each: the cumulative mask equal in every cell, u to 1e-10"""
    from tests.test_limiter_a_posteriori import _oscillating_tube
    u, ops = _oscillating_tube(dim, N, nc)
    dx = [1.0 / nc[0]] * dim
    dt = _dt(u, dx, dim, N)
    s, lim = _limiter(dim, N, nc, dx, extra=0)
    s.upload(u)
    later = 0
    for k in range(2):
        info = {}
        u, cum, _ = K.step(u, dt, dx, ops, rounds=3, info=info)
        print("step %d: new cells per round %s, smallest margins %s" % (k, info["new"], ["%.2e" % x for x in info["margin"]]))
        assert min(info["margin"]) >= MARGIN                       # no cell may be excused
        assert 0 < cum.sum() < cum.size
        later += sum(info["new"][1:])
        n = lim.step_a_posteriori(dt, conservative=True, rounds=3)
        assert np.array_equal(lim._mask_cum.cpu().numpy(), cum), np.argwhere(lim._mask_cum.cpu().numpy() != cum)
        assert int(n) == int(cum.sum())
        got = lim.download()
        err = np.max(np.abs(got - u)) / np.max(np.abs(u))
        print("   rel err %.3e" % err)
        assert err < 1e-10
    if dim == 3:
        assert later > 0, "the case was built to need a second round"


TUBE_CASES = [(2, 4, 16), (3, 6, 16)]


@gpu
@pytest.mark.parametrize("dim,N,nx", TUBE_CASES)
def test_double_sod_tube_conserves_through_run(dim, N, nx):
    import torch
    want = _golden()["dim%d_N%d_nx%d" % (dim, N, nx)]
    nc = (nx,) + (1,) * (dim - 1)
    s, lim = _limiter(dim, N, nc, [1.0 / nx] * dim, extra=0)
    ops = s.operators()
    u0 = M.tube_initial(N, nx, dim)
    s.upload(u0)
    steps = lim.run(0.1, cfl=0.4, track=True, conservative=True, rounds=3)
    torch.cuda.synchronize()
    st = {k: v.item() for k, v in lim.stats.items()}
    u = lim.download()
    l1 = M.tube_l1(u, ops["xi"], ops["w"], 0.1)
    cons = M.defects(M.totals(u0, ops["w"]), M.totals(u, ops["w"]))
    print("dim %d N %d nx %d: steps %d (restatement %d) L1 %.8f (%.8f) min rho %.6f (%.6f) min p %.6f (%.6f) troubled <= %d (%d) unresolved %d (%d)"
          % (dim, N, nx, steps, want["steps"], l1, want["l1"], st["min_rho"], want["min_rho"], st["min_p"], want["min_p"], st["max_troubled"],
             want["max_troubled"], st["unresolved"], want["unresolved"]))
    print("   cons %s (restatement %s), bound %.3e" % (cons, want["cons"], K.bound(steps)))
    assert st["finite"] and np.isfinite(u).all()                   # every step
    assert st["min_rho"] > 0 and st["min_p"] > 0                   # every step, every node
    assert abs(s.time - 0.1) < 1e-12
    assert abs(steps - want["steps"]) <= 0.01 * want["steps"]
    assert abs(l1 - want["l1"]) <= 0.01 * want["l1"]
    assert cons[0] <= K.bound(steps) and cons[4] <= K.bound(steps), cons
    assert max(cons) <= K.bound(steps), cons
    assert st["unresolved"] == want["unresolved"]


PARTITION_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from exahype_amd import solvers as exa
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
part = exa.CartesianPartition(world, rank, 2, [2, 1])
s = exa.AderDgSolver(2, 4, (4, 2), dx=[1.0 / 8] * 2, part=part, backend_is_gloo=True)
lim = exa.SubcellLimiter(s, capacity=8)
for call in (lambda: lim.step_a_posteriori(1e-3, conservative=True), lambda: lim.run(1e-3, conservative=True),
             lambda: lim.step(1e-3, np.zeros((4, 2), dtype=bool), conservative=True)):
    try:
        call()
    except ValueError as e:
        assert "partitioned" in str(e) and "out of scope" in str(e), e
    else:
        raise AssertionError("a partitioned grid was accepted")
print("rank", rank, "refused")
dist.barrier(); dist.destroy_process_group()
'''


@gpu
def test_refuses_a_partitioned_axis(tmp_path):
    _run_ranks(tmp_path, PARTITION_WORKER % dict(root=ROOT), 2)


@gpu
def test_refuses_a_term_set_with_a_non_conservative_product():
    from exahype_amd import solvers as exa
    from tests.test_dg_hard_states import euler_ncp
    s = exa.AderDgSolver(2, 3, (4, 2), pde=euler_ncp().register(), n_vars=5, dx=[0.25] * 2)
    lim = exa.SubcellLimiter(s, capacity=4)
    with pytest.raises(ValueError, match="non-conservative product"):
        lim.step_a_posteriori(1e-3, conservative=True)
    with pytest.raises(ValueError, match="non-conservative product"):
        lim.step(1e-3, np.zeros((4, 2), dtype=bool), conservative=True)
    buf = (C.c_double * 8)()
    cells = (C.c_long * 1)(-1)
    assert s.lib.exa_lim_face_flux(s._plan, C.cast(buf, C.c_void_p), C.cast(cells, C.c_void_p), 1, C.cast(buf, C.c_void_p), None) == -1
    assert b"non-conservative" in s.lib.exa_last_error()


@gpu
def test_default_mode_is_unchanged_bit_for_bit():
    """conservative=False launches nothing new: step_a_posteriori with and without the keyword give the same bits"""
    from tests.test_limiter_a_posteriori import _oscillating_tube
    dim, N, nc = 2, 4, (8, 2)
    u, _ = _oscillating_tube(dim, N, nc)
    dx = [1.0 / nc[0]] * dim
    dt = _dt(u, dx, dim, N)
    out = []
    for kw in ({}, {"conservative": False, "rounds": 3}):
        s, lim = _limiter(dim, N, nc, dx, extra=0)
        s.upload(u)
        lim.step_a_posteriori(dt, **kw)
        out.append(lim.download())
        assert getattr(lim, "_fvflux", None) is None
    assert np.array_equal(out[0], out[1])


@gpu
@pytest.mark.parametrize("dim,N,nc", [(2, 4, (8, 2)), (3, 4, (8, 1, 2))])
def test_a_posteriori_step_is_the_step_with_its_own_mask(dim, N, nc):
    """One pipeline behind both entries: step_a_posteriori(dt) finds a mask m, and step(dt, m) from the same state gives the same bits; so
    does one conservative round against step(dt, cumulative mask, conservative=True)."""
    from exahype_amd import solvers as exa
    from tests.test_limiter_a_posteriori import _oscillating_tube
    u, _ = _oscillating_tube(dim, N, nc)
    dx = [1.0 / nc[0]] * dim
    dt = _dt(u, dx, dim, N)
    ncells = int(np.prod(nc))
    s = exa.AderDgSolver(dim, N, nc, dx=dx, one_kernel_step=False)
    lim = exa.SubcellLimiter(s, capacity=ncells)

    def fresh():
        s.upload(u)
        s.time = 0.0

    for kw, found in (({}, "_mask"), ({"conservative": True, "rounds": 1}, "_mask_cum")):
        fresh()
        lim.step_a_posteriori(dt, **kw)
        m = getattr(lim, found).clone()
        u_found = lim.download()
        fresh()
        lim.step(dt, m, conservative=bool(kw))
        u_given = lim.download()
        print("dim %d N %d nc %s %s: %d of %d troubled" % (dim, N, nc, "conservative" if kw else "plain", int(m.sum()), ncells))
        assert 0 < int(m.sum()) < ncells
        assert np.array_equal(u_found, u_given)

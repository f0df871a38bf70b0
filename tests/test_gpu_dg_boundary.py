"""ADER-DG domain boundaries on the GPU (exa_dg_boundary_ghost, AderDgSolver(boundary=...)): stage B with boundary ghosts against the numpy
restatement for every kind, the outflow ghost against exa_dg_pack_face, walls against the mirrored periodic box, a closed box, exact
boundary data at full order, sharded blocks, the subcell limiter and the CFL step of run()."""
import ctypes as CT
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import aderdg_numpy as A
from oracle.dg_operators import operators
from tests import dg_boundary_numpy as B
from tests.util import cfl_dt, dg_err, euler_dg_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EULER_SIGN = {a: np.where(np.arange(5) == 1 + a, -1.0, 1.0) for a in range(3)}
Q_IN = np.array([1.3, 0.4, -0.2, 0.1, 3.1])                      # a constant Dirichlet state


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available()
    from exahype_amd import solvers
    return solvers


def smooth_state(X, t):
    """An admissible Euler state that varies in space and time; numpy arrays or device tensors [..., 3] -> [..., 5]."""
    import torch
    lib = torch if isinstance(X, torch.Tensor) else np
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    rho = 1.0 + 0.2 * lib.sin(2.0 * x + y - 0.5 * z + 3.0 * t)
    vx, vy, vz = 0.3 * lib.cos(x - y + t), 0.2 * lib.sin(y + z - t), -0.1 + 0.05 * x
    p = 1.0 + 0.1 * lib.cos(x + z + 2.0 * t)
    return lib.stack([rho, rho * vx, rho * vy, rho * vz, p / 0.4 + 0.5 * rho * (vx * vx + vy * vy + vz * vz)], -1)


def density_wave(X, t, d=3):
    """rho = 1 + 0.2 sin(2 pi (x + y + z - 3 t)), velocity (1, 1, 1), p = 1: pure advection (tests/test_gpu_parity.py's exact solution)."""
    import torch
    lib = torch if isinstance(X, torch.Tensor) else np
    rho = 1 + 0.2 * lib.sin(2 * np.pi * (X[..., 0] + X[..., 1] + X[..., 2] - d * t))
    return lib.stack([rho, rho, rho, rho, 1 / 0.4 + 0.5 * rho * d], -1)


def _solver_bc(exa, kinds):
    """kinds {(axis, side): name} -> the solver's boundary dict"""
    out = {}
    for key, k in kinds.items():
        out[key] = {"outflow": exa.Outflow(), "wall": exa.Wall(), "const": exa.Dirichlet(Q_IN), "func": exa.Dirichlet(smooth_state)}[k]
    return out


def _oracle_bc(kinds, nc, N, ops, dx, dt):
    out = {}
    for (a, side), k in kinds.items():
        if k == "outflow":
            out[(a, side)] = ("outflow",)
        elif k == "wall":
            out[(a, side)] = ("wall", EULER_SIGN[a])
        else:
            X = B.face_positions(nc, N, ops, dx, a, side)
            out[(a, side)] = ("dirichlet", B.dirichlet_ghost(Q_IN if k == "const" else smooth_state, A.Euler(), X, a, 0.0, dt, ops,
                                                             constant=k == "const"))
    return out


KIND_SETS = {
    "outflow": lambda dim: {(a, s): "outflow" for a in range(dim) for s in range(2)},
    "wall": lambda dim: {(a, s): "wall" for a in range(dim) for s in range(2)},
    "const": lambda dim: {(a, s): "const" for a in range(dim) for s in range(2)},
    "func": lambda dim: {(a, s): "func" for a in range(dim) for s in range(2)},
    "mixed": lambda dim: {(0, 0): "func", (0, 1): "outflow", (1, 0): "wall", (1, 1): "const"},     # (axis 2, if any: periodic)
}
PARITY_CASES = [(2, 4, (4, 3), "auto"), (3, 3, (3, 2, 2), "auto"), (3, 6, (2, 3, 2), "lds"), (3, 6, (2, 3, 2), "reg"), (3, 8, (2, 2, 2), "auto")]


@pytest.mark.parametrize("kind", sorted(KIND_SETS))
@pytest.mark.parametrize("dim,N,nc,stage_a", PARITY_CASES)
def test_stage_b_with_boundary_ghosts_vs_numpy(exa, dim, N, nc, stage_a, kind):
    ops = operators(N)
    u = euler_dg_state(tuple(nc) + (N,) * dim, seed=5)
    dx = [0.7 / c for c in nc]
    dt = cfl_dt(u, dx, dim, N, cfl=0.6)
    kinds = KIND_SETS[kind](dim)
    s = exa.AderDgSolver(dim, N, nc, dx=dx, stage_a=stage_a, boundary=_solver_bc(exa, kinds))
    s.upload(u)
    s.step(dt)
    want = B.step(u, dt, dx, ops, A.Euler(), _oracle_bc(kinds, nc, N, ops, dx, dt))
    e = dg_err(s.download(), want, u)
    assert e <= 1e-10, (kind, e)
    # the same data periodic differs from it by far more than the tolerance: the ghosts were used
    assert dg_err(A.step(u, dt, dx, ops, A.Euler()), want, u) > 1e-6


@pytest.mark.parametrize("dim,N,nc", [(2, 4, (4, 3)), (3, 6, (2, 3, 4)), (3, 5, (3, 2, 2))])
def test_outflow_ghost_is_the_packed_face_bit_for_bit(exa, dim, N, nc):
    import torch
    u = euler_dg_state(tuple(nc) + (N,) * dim, seed=2)
    s = exa.AderDgSolver(dim, N, nc, boundary={(a, side): exa.Outflow() for a in range(dim) for side in range(2)})
    s.upload(u)
    s.predictor_volume(1e-3)
    s.fill_boundary(1e-3)
    for d, side, _, _, buf in s._bc:
        packed = torch.full_like(buf, np.nan)
        from exahype_amd._lib import check
        check(s.lib.exa_dg_pack_face(s._plan, CT.c_void_p(s.trace.data_ptr()), d, side, CT.c_void_p(packed.data_ptr()), None))
        torch.cuda.synchronize()
        assert torch.equal(buf, packed), (d, side)


def test_boundary_ghost_rejects_bad_arguments(exa):
    from exahype_amd._lib import darr
    s = exa.AderDgSolver(3, 3, (2, 2, 2), boundary={(0, 0): exa.Wall()})
    buf, tr = CT.c_void_p(s._bc[0][4].data_ptr()), CT.c_void_p(s.trace.data_ptr())
    ones = darr([1.0] * 10)
    assert s.lib.exa_dg_boundary_ghost(s._plan, tr, 3, 0, 1, ones, None, 0.1, buf, None, None) == -1                   # d outside 3-D
    assert b"outside" in s.lib.exa_last_error()
    assert s.lib.exa_dg_boundary_ghost(s._plan, tr, 0, 2, 1, ones, None, 0.1, buf, None, None) == -1                   # side 2
    assert s.lib.exa_dg_boundary_ghost(s._plan, tr, 0, 0, 4, ones, None, 0.1, buf, None, None) == -1                   # kind 4
    assert s.lib.exa_dg_boundary_ghost(s._plan, tr, 0, 0, 2, None, None, 0.1, buf, None, None) == -1                   # wall without factors
    assert s.lib.exa_dg_boundary_ghost(s._plan, tr, 0, 0, 3, None, None, 0.1, buf, None, None) == -1                   # Dirichlet without a state
    assert s.lib.exa_dg_boundary_ghost(s._plan, tr, 0, 0, 1, ones, None, 0.1, None, None, None) == -1                  # no ghost buffer
    assert s.lib.exa_dg_boundary_ghost(s._plan, tr, 0, 0, 1, ones, None, 0.1, buf, None, None) == 0


def _mirror_pair(exa, N, nc, steps, stage_a="auto"):
    import torch
    dx = [1.0 / 16] * 3
    walled = exa.AderDgSolver(3, N, nc, dx=dx, stage_a=stage_a, boundary={(0, 0): exa.Wall(), (0, 1): exa.Wall()})
    u = smooth_state(walled.node_positions(), 0.0).reshape(walled.u.shape).cpu().numpy()
    dt = cfl_dt(u, dx, 3, N, cfl=0.6)
    walled.upload(u)
    big = exa.AderDgSolver(3, N, (2 * nc[0],) + tuple(nc[1:]), dx=dx, stage_a=stage_a)
    big.upload(np.concatenate([u, B.mirror_x(u)], axis=0))
    for _ in range(steps):
        walled.step(dt)
        big.step(dt)
    torch.cuda.synchronize()
    return walled.download(), big.download()


@pytest.mark.parametrize("N,stage_a", [(6, "lds"), (6, "reg"), (8, "auto")])
def test_walls_equal_the_mirrored_periodic_box(exa, N, stage_a):
    got, big = _mirror_pair(exa, N, (8, 4, 4), 10, stage_a)
    assert np.isfinite(got).all() and np.isfinite(big).all()
    rel = np.max(np.abs(got - big[:8])) / np.max(np.abs(big))
    assert rel <= 1e-11, rel
    assert np.max(np.abs(big[8:] - B.mirror_x(big[:8]))) <= 1e-11 * np.max(np.abs(big))     # (the periodic run kept its symmetry)


def _w_integral(torch, u, w, dim):
    spec = {2: "abij,i,j->", 3: "abcijk,i,j,k->"}[dim]
    return np.array([float(torch.einsum(spec, u[..., v], *([w] * dim))) for v in range(5)])


@pytest.mark.parametrize("dim,N,nc", [(3, 4, (4, 3, 3)), (3, 6, (3, 3, 2)), (2, 5, (5, 4))])
def test_closed_box_conserves_mass_and_energy(exa, dim, N, nc):
    import torch
    s = exa.AderDgSolver(dim, N, nc, boundary={(a, side): exa.Wall() for a in range(dim) for side in range(2)})
    X = s.node_positions().reshape(tuple(nc) + (N,) * dim + (3,))
    s.u = smooth_state(X, 0.0).contiguous()
    w = torch.as_tensor(s.operators()["w"], device="cuda")
    m0 = _w_integral(torch, s.u, w, dim)
    s.run(0.05, cfl=0.6, max_steps=20)
    torch.cuda.synchronize()
    m1 = _w_integral(torch, s.u, w, dim)
    assert bool(torch.isfinite(s.u).all())
    for v in (0, 4):
        assert abs(m1[v] - m0[v]) / abs(m0[v]) < 1e-12, (v, m0, m1)
    # a gas at rest in the box stays at rest
    r = exa.AderDgSolver(dim, N, nc, boundary={(a, side): exa.Wall() for a in range(dim) for side in range(2)})
    rest = np.zeros(tuple(nc) + (N,) * dim + (5,))
    rest[..., 0], rest[..., 4] = 1.0, 2.5
    r.upload(rest)
    for _ in range(20):
        r.step(2e-3)
    assert np.max(np.abs(r.download() - rest)) <= 1e-13


def _wave_errors(exa, p, meshes, boundary_of, pde=None):
    import torch
    d, N = 3, p + 1
    w = operators(N)["w"]
    errs = []
    for nc in meshes:
        kw = dict(pde=pde) if pde is not None else {}
        s = exa.AderDgSolver(d, N, (nc,) * d, boundary=boundary_of(exa), **kw)
        X = s.node_positions()
        s.u = density_wave(X, 0.0).reshape(s.u.shape).contiguous()
        T = 0.04
        s.run(T, cfl=0.3)
        exact = density_wave(X, T).reshape(s.u.shape)
        torch.cuda.synchronize()
        e = (s.u - exact)[..., 0].cpu().numpy()
        errs.append(np.sqrt(np.einsum("abcijk,i,j,k->", e ** 2, w, w, w) / nc ** d))
    return errs, np.log2(errs[0] / errs[1])


ALL_DIRICHLET = lambda exa: {(a, s): exa.Dirichlet(density_wave) for a in range(3) for s in range(2)}      # noqa: E731
INFLOW_OUTFLOW = lambda exa: {(0, 0): exa.Dirichlet(density_wave), (0, 1): exa.Outflow()}                 # noqa: E731


@pytest.mark.parametrize("p,meshes", [(3, (3, 6)), (5, (2, 4))])
@pytest.mark.parametrize("which", ["dirichlet_everywhere", "inflow_outflow"])
def test_exact_boundary_data_keeps_the_order(exa, p, meshes, which):
    errs, order = _wave_errors(exa, p, meshes, ALL_DIRICHLET if which == "dirichlet_everywhere" else INFLOW_OUTFLOW)
    assert order >= p + 0.7, (errs, order)


def test_exact_boundary_data_through_a_generated_term_set(exa):
    """The SymPy-generated Euler set: its JIT side library carries the boundary entry of the launch table."""
    sys.path.insert(0, ROOT)
    import bench
    pid = bench.sympy_euler().register()
    errs, order = _wave_errors(exa, 3, (3, 6), ALL_DIRICHLET, pde=pid)
    assert order >= 3.7, (errs, order)
    with pytest.raises(ValueError, match="needs sign"):
        exa.AderDgSolver(3, 4, (2, 2, 2), pde=pid, boundary={(0, 0): exa.Wall()})


def test_boundary_refuses_the_one_kernel_step_and_skips_the_fused_2d_step(exa):
    with pytest.raises(ValueError, match="one_kernel_step"):
        exa.AderDgSolver(3, 6, (2, 2, 2), stage_a="reg", one_kernel_step=True, boundary={(0, 0): exa.Outflow()})
    assert exa.AderDgSolver(2, 4, (4, 4), n_picard=0)._fused
    s = exa.AderDgSolver(2, 4, (4, 4), n_picard=0, boundary={(1, 1): exa.Outflow()})
    assert not s._fused
    u = euler_dg_state((4, 4, 4, 4), seed=3)
    s.upload(u)
    dt = cfl_dt(u, s.dx, 2, 4, cfl=0.3)
    s.step(dt)
    ops = operators(4)
    # single stage: qbar := u, Fbar := f(u), then the boundary Riemann solve
    Fbar = [A.Euler().flux(u, a) for a in range(2)]
    tr = A.traces(u, Fbar, ops)
    Ff = [B.riemann_faces(tr[a], A.Euler(), a, 2, {(1, 1): ("outflow",)}) for a in range(2)]
    want = B.corrector(A.volume(u, Fbar, dt, s.dx, ops), Ff, dt, s.dx, ops)
    assert dg_err(s.download(), want, u) <= 1e-10


def test_run_takes_the_dirichlet_eigenvalue(exa):
    """A constant Dirichlet state faster than anything inside shortens the CFL step of run()."""
    N, nc = 4, (4, 3, 3)
    u = euler_dg_state(tuple(nc) + (N,) * 3, seed=4)
    fast = np.array([1.0, 6.0, 0.0, 0.0, 2.5 + 18.0])
    lam_in = max(np.max(A.Euler().maxeig(u.reshape(-1, 5), d)) for d in range(3))
    lam_bc = 6.0 + np.sqrt(1.4 * 1.0)
    assert lam_bc > 2 * lam_in
    periodic = exa.AderDgSolver(3, N, nc)
    periodic.upload(u)
    walled = exa.AderDgSolver(3, N, nc, boundary={(0, 0): exa.Dirichlet(fast)})
    walled.upload(u)
    T = 0.02
    n_p, n_b = periodic.run(T, cfl=0.5), walled.run(T, cfl=0.5)
    assert n_b > 1.5 * n_p, (n_p, n_b)
    # a time-dependent datum: its eigenvalue enters through the boundary kernel's scalar
    fn = exa.AderDgSolver(3, N, nc, boundary={(0, 0): exa.Dirichlet(lambda X, t: fast_state(X, fast))})
    fn.upload(u)
    assert fn.run(T, cfl=0.5) == n_b


def fast_state(X, q):
    import torch
    return torch.as_tensor(q, device=X.device).expand(X.shape[0], 5)


def test_limiter_with_walls_equals_the_mirrored_periodic_box(exa):
    import torch
    for dim, N, nc in ((2, 4, (3, 3)), (3, 3, (3, 2, 2))):
        u = euler_dg_state(tuple(nc) + (N,) * dim, seed=21, amp=0.4)
        dx = [0.25] * dim
        dt = cfl_dt(u, dx, dim, N, cfl=0.3)
        mask = np.zeros(nc, dtype=bool)
        mask[0] = True                                      # cells touching the low wall ...
        mask[nc[0] - 1, 0] = True                           # ... and the high one
        mask[1, -1] = True
        half = exa.AderDgSolver(dim, N, nc, dx=dx, boundary={(0, 0): exa.Wall(), (0, 1): exa.Wall()})
        half.upload(u)
        big = exa.AderDgSolver(dim, N, (2 * nc[0],) + tuple(nc[1:]), dx=dx)
        big.upload(np.concatenate([u, B.mirror_x(u)], axis=0))
        lh, lb = exa.SubcellLimiter(half), exa.SubcellLimiter(big)
        dh, db = lh.detect(), lb.detect()
        assert torch.equal(dh, db[:nc[0]]), (dim, dh, db)
        lh.step(dt, mask)
        lb.step(dt, np.concatenate([mask, np.flip(mask, axis=0)], axis=0))
        got, want = lh.download(), lb.download()
        rel = np.max(np.abs(got - want[:nc[0]])) / np.max(np.abs(want))
        assert rel <= 1e-11, (dim, rel)
        # the troubled cells at the walls did take the FV update: the plain DG step differs there
        plain = exa.AderDgSolver(dim, N, nc, dx=dx, boundary={(0, 0): exa.Wall(), (0, 1): exa.Wall()})
        plain.upload(u)
        plain.step(dt)
        assert np.max(np.abs(plain.download()[0] - got[0])) > 1e-8


def _run_ranks(tmp_path, text, world, timeout=600):
    import socket
    script = tmp_path / "worker.py"
    script.write_text(text)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, o[-3000:])


SHARD_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from exahype_amd import solvers as exa
from tests.util import assert_shard_equals_whole_block, euler_dg_state
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group(%(backend)r, rank=rank, world_size=world)
dim, N, nc = 3, %(N)d, %(nc)r
part = exa.CartesianPartition(world, rank, dim, %(pdims)r, exchange_self=%(selfx)r)
G = tuple(nc[a] * part.pdims[a] for a in range(3))
u = euler_dg_state(G + (N,) * dim, seed=42)
dx = [1.0 / g for g in G]
bc = lambda: {(0, 0): exa.Wall(), (0, 1): exa.Wall(), (1, 0): exa.Outflow(), (1, 1): exa.Outflow()}
s = exa.AderDgSolver(dim, N, nc, dx=dx, part=part, backend_is_gloo=%(gloo)r, boundary=bc())
assert s.halo is not None
sl = tuple(slice(part.coords[a] * nc[a], (part.coords[a] + 1) * nc[a]) for a in range(3))
s.upload(u[sl])
whole = exa.AderDgSolver(dim, N, G, dx=dx, boundary=bc())
whole.upload(u)
dt = 0.3 * min(dx) / ((2 * N - 1) * 3 * 1.5)
for k in range(3):
    s.step(dt * (1.0 - 0.1 * k))
    whole.step(dt * (1.0 - 0.1 * k))
torch.cuda.synchronize()
got, want = s.download(), whole.download()[sl]
err = np.max(np.abs(got - want)) / np.max(np.abs(want))
failed = None
try:
    assert err <= 1e-13, err
    # the same stage-A kernel on shard and block (its name depends on N, n_picard and the variant alone): equal bit for bit
    assert_shard_equals_whole_block(got, want, u[sl], s, whole, "walls N %%d %%s, rank %%d" %% (N, nc, rank))
except AssertionError as e:
    failed = e
dist.barrier(); dist.destroy_process_group()                    # (leave together: a rank that failed alone would keep the others waiting)
print("rank", rank, "rel err", err, "bit-equal", np.array_equal(got, want))
if failed is not None:
    raise failed
'''


@pytest.mark.parametrize("N,nc", [(4, (2, 3, 2)), (6, (2, 2, 2))])
def test_sharded_walls_equal_the_single_block(tmp_path, N, nc):
    """two ranks over gloo sharing cuda:0, walls on the partitioned axis (each rank has one), outflow on the other"""
    _run_ranks(tmp_path, SHARD_WORKER % dict(root=ROOT, N=N, nc=nc, pdims=[2, 1, 1], selfx=(), backend="gloo", gloo=True), 2)


def test_sharded_walls_over_rccl_send_recv_to_self(tmp_path):
    """one rank on RCCL, its own neighbour along the walled axis: the wrap layers travel, the boundary ghosts are what stage B reads"""
    _run_ranks(tmp_path, SHARD_WORKER % dict(root=ROOT, N=6, nc=(3, 2, 2), pdims=[1, 1, 1], selfx=(0,), backend="nccl", gloo=False), 1)

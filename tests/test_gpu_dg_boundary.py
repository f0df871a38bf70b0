"""ADER-DG domain boundaries on the GPU (exa_dg_boundary_ghost, AderDgSolver(boundary=...)): stage B with boundary ghosts against the numpy
restatement for every kind at DG_TOL of the increment (Euler rows, and rows whose terms see x and t with an ncp; tables and references in
tests/dg_boundary_cases.py, their CPU check in tests/test_dg_boundary_reference.py), run() against its replay, the outflow ghost against
exa_dg_pack_face, walls against the mirrored periodic box, a closed box, exact boundary data at full order, sharded blocks, the subcell
limiter and the CFL step of run()."""
import ctypes as CT
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import aderdg_numpy as A
from oracle.dg_operators import operators
from tests import dg_boundary_cases as BC
from tests import dg_boundary_numpy as B
from tests.dg_boundary_cases import smooth_state
from tests.util import DG_TOL, assert_dg_parity, cfl_dt, dg_err, euler_dg_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available()
    from exahype_amd import solvers
    return solvers


def density_wave(X, t, d=3):
    """rho = 1 + 0.2 sin(2 pi (x + y + z - 3 t)), velocity (1, 1, 1), p = 1: pure advection (tests/test_gpu_parity.py's exact solution)."""
    import torch
    lib = torch if isinstance(X, torch.Tensor) else np
    rho = 1 + 0.2 * lib.sin(2 * np.pi * (X[..., 0] + X[..., 1] + X[..., 2] - d * t))
    return lib.stack([rho, rho, rho, rho, 1 / 0.4 + 0.5 * rho * d], -1)


def _solver(exa, c, **kw):
    """the AderDgSolver of a tests/dg_boundary_cases.py Case: its box, origin, start time and boundary dict"""
    cond = {"outflow": lambda a: exa.Outflow(), "wall": lambda a: exa.Wall() if c.table == "euler" else exa.Wall(c.sign(a)),
            "const": lambda a: exa.Dirichlet(c.const), "func": lambda a: exa.Dirichlet(c.func)}
    if c.table == "xt":
        kw = dict(dict(pde=c.sympy_pde.register(), n_vars=3), **kw)
    return exa.AderDgSolver(c.dim, c.N, c.nc, dx=c.dx, stage_a=c.stage_a, n_picard=c.n_picard, origin=c.origin, time=c.t0,
                            boundary={key: cond[k](key[0]) for key, k in c.kinds.items()}, **kw)


def _euler_params():
    """(the five rows that were here before the tables keep their ids)"""
    out = []
    for row, kind in BC.EULER_CASES:
        i = BC.EULER_ROWS.index(row)
        old = i < len(BC.PARITY_CASES)
        out.append(pytest.param(row, kind, id="%d-%d-nc%d-%s-%s" % (row[0], row[1], i, row[3] if old else "%s%d" % (row[3], row[4]), kind)))
    return out


@pytest.mark.parametrize("row,kind", _euler_params())
def test_stage_b_with_boundary_ghosts_vs_numpy(exa, row, kind):
    """One step at CFL 0.9 of every Euler row and kind set against the restatement, to DG_TOL of the increment; the restatement with one Picard
    iteration less is seen (tests/test_dg_boundary_reference.py: and so is every other mutant of the row)."""
    c = BC.get_case("euler", row, kind)
    s = _solver(exa, c)
    s.upload(c.u)
    s.step(c.dt)
    want = c.state()
    got = s.download()
    e = dg_err(got, want, c.u)
    print("euler %s: dg_err %.3e" % (BC.case_id((row, kind)), e))
    assert_dg_parity(got, want, c.u, c.state("picard") if c.n_it > 0 else None, tol=DG_TOL, what="euler " + BC.case_id((row, kind)))
    assert e <= 1e-10, (kind, e)
    # the same data periodic differs from it by far more than the tolerance: the ghosts were used
    ops = operators(c.N)
    periodic = A.step_single_stage(c.u, c.dt, c.dx, ops, A.Euler()) if c.n_it == 0 else A.step(c.u, c.dt, c.dx, ops, A.Euler())
    assert dg_err(periodic, want, c.u) > 1e-6


@pytest.mark.parametrize("row,kind", [pytest.param(r, k, id=BC.case_id((r, k))) for r, k in BC.XT_CASES])
def test_xt_term_set_with_boundary_ghosts_vs_numpy(exa, row, kind):
    """Term sets whose flux, eigenvalue and ncp see x and t, on a bounded box away from the origin: two steps of different size from t = 0.4.  The
    boundary kernel places the face nodes itself (transverse axes, normal coordinate, level times) for the flux of the Dirichlet data -- of a
    function and of a constant state -- and for the eigenvalue it leaves to run(); stage B reads q+ of the ncp's jump term from the ghost."""
    c = BC.get_case("xt", row, kind)
    s = _solver(exa, c)
    assert s.lib.exa_pde_flags(s.pde) == (1 if c.with_xt else 0) + (2 if c.with_ncp else 0)
    s.upload(c.u)
    t = c.t0
    for dt in c.dts:
        s.step(dt)
        t += dt
    assert abs(s.time - t) < 1e-15
    what = "xt " + BC.case_id((row, kind))
    e, em = assert_dg_parity(s.download(), c.state(dts=c.dts), c.u, c.state("picard", dts=c.dts), tol=DG_TOL, what=what)
    # the eigenvalue the boundary kernel left: of the Dirichlet states of the LAST step, over levels, face nodes and directions (a constant
    # state's too where the eigenvalue sees x / t; elsewhere it is a host clamp).  test_cfl_launch_same_u_and_exact_maximum compares two device
    # evaluations and can ask for equal bits; this one compares the device with numpy, whose sine and whose roundings are not the device's: the
    # eigenvalue |a_d + 3/10 sin(2 x + t)| + |q0| / 5 is eight rounded operations on terms no larger than the result (the datum's own sine included;
    # the device may contract 2 x + t and the products into FMAs), each within one unit in the last place -- 8 ulp.  Measured: equal in 11 of 12 cases,
    # one ulp (2.2e-16) in the twelfth.  The levels of the step before, the midpoint alone or the origin left out move it by 2e-5 to 0.15.
    want_lam = c.dirichlet_eigenvalue(c.t0 + c.dts[0], c.dts[1], kinds=("func", "const") if c.with_xt else ("func",))
    got_lam = float(s._lam_bc[0])
    print("%s: dg_err %.3e, mutant %.3e, lam_bc %.17g, restatement %.17g, diff %.3e" % (what, e, em, got_lam, want_lam, got_lam - want_lam))
    assert abs(got_lam - want_lam) <= 8 * np.finfo(np.float64).eps * want_lam, (got_lam, want_lam)


@pytest.mark.parametrize("table,row,kind", BC.RUN_CASES)
def test_run_on_a_bounded_box_equals_the_replay(exa, table, row, kind):
    """run(t_end, cfl) for about 2.5 steps against the loop replayed on the restatement: the eigenvalue of the state and of the Dirichlet data, then
    the step (tests/dg_boundary_cases.py Case.replay).  In the x / t row the constant state's eigenvalue at the face nodes sets every step."""
    c = BC.get_case(table, row, kind)
    t_end = c.t_end()
    steps, t, want = c.replay(t_end)
    s = _solver(exa, c)
    s.upload(c.u)
    n = s.run(t_end, cfl=BC.RUN_CFL)
    print("run %s %s: steps %d (replay %d), time - replay %.3e" % (table, BC.case_id((row, kind)), n, steps, s.time - t))
    assert n == steps, (n, steps)
    assert abs(s.time - t) <= 1e-14, (s.time, t)
    assert_dg_parity(s.download(), want, c.u, c.replay(t_end, mutant="picard")[2], tol=DG_TOL, what="run %s %s" % (table, BC.case_id((row, kind))))


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


SHARD_XT_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from exahype_amd import solvers as exa
from tests import dg_boundary_cases as BC
from tests.util import assert_dg_parity, assert_shard_equals_whole_block
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
dim, N, nc, pdims = BC.SHARDED_XT_BC_CASE
c = BC.sharded_xt_bc_case()                                     # the WHOLE block: c.nc = nc * pdims
part = exa.CartesianPartition(world, rank, dim, pdims)
pid = c.sympy_pde.register()
bc = lambda: {key: exa.Dirichlet(c.func if k == "func" else c.const) for key, k in c.kinds.items()}
s = exa.AderDgSolver(dim, N, nc, pde=pid, n_vars=3, dx=c.dx, part=part, backend_is_gloo=True, origin=c.origin, time=c.t0, boundary=bc())
assert s.halo is not None
sl = tuple(slice(part.coords[a] * nc[a], (part.coords[a] + 1) * nc[a]) for a in range(3))
s.upload(c.u[sl])
whole = exa.AderDgSolver(dim, N, c.nc, pde=pid, n_vars=3, dx=c.dx, origin=c.origin, time=c.t0, boundary=bc())
whole.upload(c.u)
for dt in c.dts:
    s.step(dt)
    whole.step(dt)
torch.cuda.synchronize()
got, block = s.download(), whole.download()
failed = None
try:
    assert abs(s.time - whole.time) < 1e-15
    assert_shard_equals_whole_block(got, block[sl], c.u[sl], s, whole, "x/t Dirichlet faces N %%d, rank %%d" %% (N, rank))
    assert_dg_parity(block, c.state(dts=c.dts), c.u, c.state("picard", dts=c.dts), what="x/t Dirichlet faces, whole block (rank %%d)" %% rank)
except AssertionError as e:
    failed = e
dist.barrier(); dist.destroy_process_group()                    # (leave together: a rank that failed alone would keep the others waiting)
print("rank", rank, "bit-equal", np.array_equal(got, block[sl]))
if failed is not None:
    raise failed
'''


def test_sharded_dirichlet_faces_of_an_xt_term_set_equal_the_single_block(tmp_path):
    """two ranks over gloo sharing cuda:0, the x / t + ncp set: the Dirichlet function on both x faces (one per rank) and on the low y face, whose
    nodes on rank 1 lie at that shard's offset, the constant state on the high z face; three steps of different size.  Every shard against the
    whole block, the whole block against the restatement to DG_TOL."""
    _run_ranks(tmp_path, SHARD_XT_WORKER % dict(root=ROOT), 2)

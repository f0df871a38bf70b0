"""Stage B (Riemann solve + corrector) after its per-workgroup chain was shortened: the cells of a workgroup decoded once (one cell: scalar
registers; several: a table in LDS), the u* loads of the update requested together in front of the barrier, the lift coefficients from one
select chain.

3-D Euler: `predictor_volume(dt)`, then `riemann_corrector(dt)`, u against the oracle's step at DG_TOL (tests/util.py assert_dg_parity through
DgRef.check_stage_b) at every order / cells-per-workgroup combination that takes another path; the traversal (tiled, lexicographic, sub-boxes)
must not change a bit; ghost pointers (walls, outflow) against the numpy restatement as tests/test_gpu_dg_boundary.py does; the launch that
carries the CFL scan leaves the same u and exactly max_eigenvalue() of it.

The 32-bit / 64-bit choice of the slot decode is made by the launcher from the box's slot count (dg_inst.hip launch_b) and is no argument of
the C API: the 64-bit path needs a box of 2^31 cells and is not run here."""
import numpy as np
import pytest

from oracle import aderdg_numpy as A
from oracle.dg_operators import operators
from tests import dg_boundary_numpy as B
from tests.dg_cases import DgRef
from tests.util import cfl_dt, dg_err, euler_dg_state

pytestmark = pytest.mark.gpu
DIM = 3
EULER_SIGN = {a: np.where(np.arange(5) == 1 + a, -1.0, 1.0) for a in range(3)}


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available()
    from exahype_amd import solvers
    return solvers


def _input(N, nc, seed):
    u = euler_dg_state(tuple(nc) + (N,) * DIM, seed=seed)
    dx = [1.0 / nc[0], 0.8 / nc[1], 1.3 / nc[2]]             # anisotropic: the lift coefficient of a lane depends on its direction
    return u, dx, cfl_dt(u, dx, DIM, N)


def _predicted(exa, N, nc, seed, **kw):
    u, dx, dt = _input(N, nc, seed)
    s = exa.AderDgSolver(DIM, N, nc, dx=dx, **kw)
    s.upload(u)
    s.predictor_volume(dt)
    return s, u, dx, dt


# N: 3 dense, Nf = 9, four cells per workgroup (27 cells: the last workgroup holds three, its fourth slot is clamped); 4 power-of-two faces, two
# cells per workgroup; 6 dense, Nf = 36, one cell per workgroup: 8 x 8 x 8 is the tiled order, 5 x 3 x 2 the lexicographic one; 8 power-of-two,
# Nf = 64; 5 and 7 dense, Nf = 25 and 49 (three and seven passes of the update); 2 power-of-two faces, ten cells per workgroup, the last one with two
ORDER_CASES = [(3, (3, 3, 3)), (4, (2, 3, 4)), (6, (8, 8, 8)), (6, (5, 3, 2)), (8, (2, 2, 3)), (5, (3, 2, 2)), (7, (2, 1, 2)), (2, (3, 2, 2))]


@pytest.fixture(scope="module")
def tiled_p5(exa):
    """p = 5 on 8 x 8 x 8 cells: the solver with u* and the traces of one predictor, u* itself, and u after ONE launch over the block (tiled)."""
    N, nc = 6, (8, 8, 8)
    s, u, dx, dt = _predicted(exa, N, nc, seed=600 + N)
    ustar = s.u.clone()
    s.riemann_corrector(dt)
    return dict(s=s, u=u, dx=dx, dt=dt, N=N, nc=nc, ustar=ustar, got=s.u.clone())


@pytest.mark.parametrize("N,nc", ORDER_CASES)
def test_stage_b_vs_oracle(exa, tiled_p5, N, nc):
    if (N, nc) == (6, (8, 8, 8)):
        t = tiled_p5
        got, u, dx, dt = t["got"].cpu().numpy(), t["u"], t["dx"], t["dt"]
    else:
        s, u, dx, dt = _predicted(exa, N, nc, seed=600 + N)
        s.riemann_corrector(dt)
        got = s.download()
    DgRef(u, dt, dx, DIM, N, nc, N).check_stage_b(got, what="stage B N=%d %s" % (N, "x".join(map(str, nc))))


def _relaunch(t, boxes):
    """u* restored, stage B over the boxes (the traces are read only)."""
    s = t["s"]
    s.u.copy_(t["ustar"])
    for lo, hi in boxes:
        s.riemann_corrector(t["dt"], lo, hi)
    return s.u.clone()


def test_traversal_does_not_change_a_bit(tiled_p5):
    """one tiled launch == two lexicographic launches over 8 x 8 x 4 halves == a sub-box whose origin is off zero in every axis"""
    import torch
    t = tiled_p5
    halves = _relaunch(t, [((0, 0, 0), (8, 8, 4)), ((0, 0, 4), (8, 8, 8))])
    assert torch.equal(halves, t["got"])
    lo = (1, 2, 3)
    part = _relaunch(t, [(lo, (8, 8, 8))])
    inside = (slice(lo[0], None), slice(lo[1], None), slice(lo[2], None))
    assert torch.equal(part[inside], t["got"][inside])
    outside = torch.ones(t["nc"], dtype=torch.bool, device=part.device)
    outside[inside] = False
    assert torch.equal(part[outside], t["ustar"][outside])              # ... and nothing outside the box was touched


@pytest.mark.parametrize("kind", ["wall", "outflow"])
def test_ghost_pointers_vs_numpy(exa, kind):
    N, nc = 6, (3, 2, 2)
    ops = operators(N)
    u = euler_dg_state(tuple(nc) + (N,) * DIM, seed=5)
    dx = [0.7 / c for c in nc]
    dt = cfl_dt(u, dx, DIM, N, cfl=0.6)
    faces = [(a, side) for a in range(DIM) for side in range(2)]
    s = exa.AderDgSolver(DIM, N, nc, dx=dx, boundary={f: exa.Wall() if kind == "wall" else exa.Outflow() for f in faces})
    s.upload(u)
    s.predictor_volume(dt)
    s.fill_boundary(dt)
    s.riemann_corrector(dt)
    want = B.step(u, dt, dx, ops, A.Euler(), {(a, side): ("wall", EULER_SIGN[a]) if kind == "wall" else ("outflow",) for a, side in faces})
    e = dg_err(s.download(), want, u)
    print("ghost pointers, %s: dg_err %.3e" % (kind, e))
    assert e <= 1e-10, (kind, e)
    assert dg_err(A.step(u, dt, dx, ops, A.Euler()), want, u) > 1e-6     # (periodic data would differ: the ghosts were read)


@pytest.mark.parametrize("N,nc", [(6, (8, 8, 8)), (6, (5, 3, 2)), (8, (2, 2, 3)), (3, (3, 3, 3)), (4, (2, 3, 4))])
def test_cfl_launch_same_u_and_exact_maximum(exa, tiled_p5, N, nc):
    import torch
    if (N, nc) == (6, (8, 8, 8)):
        s, dt, plain = tiled_p5["s"], tiled_p5["dt"], tiled_p5["got"]
        s.u.copy_(tiled_p5["ustar"])
    else:
        s, _, _, dt = _predicted(exa, N, nc, seed=600 + N)
        ustar = s.u.clone()
        s.riemann_corrector(dt)
        plain = s.u.clone()
        s.u.copy_(ustar)
    lam = torch.zeros(1, dtype=torch.float64, device=s.u.device)
    s.riemann_corrector(dt, lam_out=lam)
    assert torch.equal(s.u, plain)
    want = s.max_eigenvalue()
    assert float(want) > 0.0
    assert torch.equal(lam, want.reshape(1)), (float(lam), float(want))

"""ADER-DG on generated term sets of 4, 6, 7 and 8 variables (tests/wide_term_sets.py) against oracle/aderdg_numpy.py with the same expressions.

Every other ADER-DG case of the suite has 1, 2, 3 or 5 variables; which stage-A kernel runs depends on the variable count (dg_inst.hip
stage_a_kind): with 8 variables the level-streamed kernel serves N = 3 to 7 in 3-D (LS = 2, 3; fractions of a wave per direction group; the
masked last level of odd N), with 6 variables and a cached scalar N = 5 to 7, and N = 8 has no kernel.  Every row asserts the kernel family
it launches, holds one step at the CFL-0.9 step and three at CFL 0.6 to DG_TOL of the per-variable increment, and must see its last Picard
iteration (tests/util.py assert_dg_parity).  Stage B, the fused 2-D single-stage step, the CFL scan and the boundary ghosts run with the same
variable counts.  tests/test_dg_wide_reference.py pins the oracle, the visibility of every row and the selection on the CPU."""
import numpy as np
import pytest

from tests import wide_term_sets as W
from tests.dg_cases import n_it_of, steps_dt
from tests.util import DG_TOL, assert_dg_parity

pytestmark = pytest.mark.gpu
CASES = [(dim, name, N, nc, n_picard, family, three) for dim, name, N, nc, n_picards, family, three in W.all_rows() for n_picard in n_picards]


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available()
    from exahype_amd import solvers
    return solvers


def _solver(exa, name, dim, N, nc, dx, **kw):
    p = W.ring(name)
    return exa.AderDgSolver(dim, N, nc, pde=p.register(), n_vars=p.n_vars, dx=dx, **kw)


@pytest.mark.parametrize("dim,name,N,nc,n_picard,family,three", CASES)
def test_wide_set_steps_vs_numpy_oracle(exa, dim, name, N, nc, n_picard, family, three):
    u, dx, dt = W.wide_input(name, dim, N, nc)
    s = _solver(exa, name, dim, N, nc, dx, n_picard=n_picard, fused_single_stage=False)
    want_family = W.family_of(name, dim, N, n_picard, family)
    assert s.stage_a_kernel_name().startswith(want_family) and "exa::UserPDE" in s.stage_a_kernel_name(), (s.stage_a_kernel_name(), want_family)
    # the CFL scan: the lambdified bound over every node and direction
    s.upload(u)
    lam = max(float(np.max(W.numpy_pde(name).maxeig(u, d))) for d in range(dim))
    assert abs(float(s.max_eigenvalue()[0]) - lam) <= 1e-12
    for steps in (1, 3) if three else (1,):
        want, mut = W.want_and_mutant(name, dim, N, nc, n_picard, steps)
        s.upload(u)
        h = dt if steps == 1 else steps_dt(dt, single_stage=n_it_of(N, n_picard) == 0)
        for _ in range(steps):
            s.step(h)
        assert_dg_parity(s.download(), want, u, mut, tol=DG_TOL, what="%s %d-D N %d %s n_picard %d, %d step(s)" % (name, dim, N, nc, n_picard, steps))


@pytest.mark.parametrize("name,N,nc", W.FUSED_ROWS)
def test_wide_set_fused_single_stage_step_vs_numpy_oracle(exa, name, N, nc):
    u, dx, dt = W.wide_input(name, 2, N, nc)
    s = _solver(exa, name, 2, N, nc, dx, n_picard=0, fused_single_stage=True)
    assert s._fused
    s.upload(u)
    for _ in range(3):
        s.step(steps_dt(dt, single_stage=True))
    assert_dg_parity(s.download(), W.reference(name, 2, N, nc, 0, 3, single_stage=True), u, None, tol=DG_TOL, what="%s fused N %d %s, 3 steps" % (name, N, nc))


@pytest.mark.parametrize("name,N,nc", W.SWAP_ROWS)
def test_wide_set_kernel_sees_which_variable_is_which(exa, name, N, nc):
    """The oracle with the flux components 1 and 2 exchanged is far from what the streamed kernel produced."""
    u, dx, dt = W.wide_input(name, 3, N, nc)
    s = _solver(exa, name, 3, N, nc, dx)
    assert s.stage_a_kernel_name().startswith(W.STREAM)
    s.upload(u)
    s.step(dt)
    got = s.download()
    assert np.max(np.abs(got - W.reference(name, 3, N, nc, N, 1, swap=(1, 2)))) > 1e-7
    assert_dg_parity(got, W.reference(name, 3, N, nc, N, 1), u, None, tol=DG_TOL, what="%s N %d %s" % (name, N, nc))


@pytest.mark.parametrize("name,dim,N", W.REFUSED)
def test_wide_set_without_a_kernel_is_refused(exa, name, dim, N):
    """6 and 8 variables at N = 8: the streamed kernel would need 165 888 / 221 184 B of LDS (3-D), the LDS kernel's image does not fit (2-D).  The plan
    names no kernel -- asked first, on the host, so nothing over-size is ever launched -- and the step raises with the reason."""
    from exahype_amd._lib import ExaHypeHipError
    nc = (1,) * dim
    u, dx, dt = W.wide_input(name, dim, N, nc)
    for n_picard in W.ALL_PICARD:
        s = _solver(exa, name, dim, N, nc, dx, n_picard=n_picard, fused_single_stage=False)
        assert s.stage_a_kernel_name() == ""
        s.upload(u)
        with pytest.raises(ExaHypeHipError, match=r"N = 8.*LDS" if dim == 3 else r"dim 2, N = 8"):
            s.step(dt)


def test_wide_set_boundary_ghosts_vs_numpy(exa):
    """Outflow, a wall (sign -1 on variables 1 to 3) and a constant Dirichlet state on three faces of an 8-variable block: the ghost kernels' NV-wide
    coefficient blocks and stage B, against tests/dg_boundary_numpy.py."""
    from oracle.dg_operators import operators
    from tests import dg_boundary_numpy as B
    name, N, nc = W.BOUNDARY_ROW
    u, dx, dt = W.wide_input(name, 3, N, nc)
    pde, ops = W.numpy_pde(name), operators(N)
    sign = np.where((np.arange(8) >= 1) & (np.arange(8) <= 3), -1.0, 1.0)
    q_in = 1.0 + 0.05 * np.arange(8)
    s = _solver(exa, name, 3, N, nc, dx, boundary={(0, 1): exa.Outflow(), (1, 0): exa.Wall(sign=sign), (2, 1): exa.Dirichlet(q_in)})
    s.upload(u)
    s.step(dt)
    X = B.face_positions(nc, N, ops, dx, 2, 1)
    bcs = {(0, 1): ("outflow",), (1, 0): ("wall", sign), (2, 1): ("dirichlet", B.dirichlet_ghost(q_in, pde, X, 2, 0.0, dt, ops, constant=True))}
    want, mut = B.step(u, dt, dx, ops, pde, bcs), B.step(u, dt, dx, ops, pde, bcs, n_it=N - 1)
    assert_dg_parity(s.download(), want, u, mut, tol=DG_TOL, what="%s boundary ghosts N %d %s" % (name, N, nc))
    # the periodic step, and the same faces with the wall's signs left out, are far from it: the ghosts and their signs were used
    assert np.max(np.abs(W.reference(name, 3, N, nc, N, 1) - want)) > 1e-6
    unsigned = dict(bcs)
    unsigned[(1, 0)] = ("wall", np.ones(8))
    assert np.max(np.abs(B.step(u, dt, dx, ops, pde, unsigned) - want)) > 1e-6

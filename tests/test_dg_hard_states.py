"""ADER-DG stage-A kernels on harder states, and a negative control per kernel.

States (tests/util.py): supersonic flow (velocities up to +-2, c ~ 1.2: both flow directions, both eigenvalue branches) and the whole state
scaled by 2^-20 and 2^20 (the device's fast reciprocal of rho far outside [0.05, 20]).  One case per stage-A kernel: the LDS kernel (3-D
N = 4), the register-resident kernel (N = 6), the level-streamed kernel (N = 7), the matrix-pipe kernel (N = 8), the plain kernel of a
generated term set (Euler + a non-conservative product, 3-D N = 4) and the fused 2-D single stage (N = 4).  All at the CFL-0.9 step against
the oracle, with assert_dg_parity.

Negative control: the same kernels run with N - 1 Picard iterations must be rejected against the oracle's N (dg_err > 100 * DG_TOL) --
on the real kernels, the measure sees the last iteration.
"""
import numpy as np
import pytest
import sympy

from tests import dg_cases as C
from tests.dg_cases import DgRef
from tests.util import DG_TOL, assert_dg_parity, cfl_dt, dg_err, euler_scaled_state, euler_supersonic_state

STATES = {"supersonic": lambda sh, seed: euler_supersonic_state(sh, seed),
          "tiny": lambda sh, seed: euler_scaled_state(sh, seed, 2.0 ** -20),
          "huge": lambda sh, seed: euler_scaled_state(sh, seed, 2.0 ** 20)}
PLAIN = ("plain_ncp_n4", 3, 4, (2, 1, 2))


def hard_input(dim, N, nc, family):
    u = STATES[family](tuple(nc) + (N,) * dim, 1000 * dim + 10 * N + len(family))
    dx = [(1.0, 0.8, 1.3)[a] / nc[a] for a in range(dim)]
    return u, dx


def hard_dt(u, dx, dim, N, family, **kw):
    """CFL 0.9; the supersonic family at CFL 0.6 (tests/dg_cases.py STEPS_CFL): at 0.9 its Picard loop no longer contracts at N = 8 (N - 1 and
    N iterations differ by the whole increment), and the result is as sensitive to rounding as the iteration is to its count."""
    dt = cfl_dt(u, dx, dim, N, **kw)
    return C.steps_dt(dt) if family == "supersonic" else dt


def euler_ncp():
    """Euler with a constant non-conservative coupling B = 0.1 e_rho e_rho^T in every direction: a generated term set the plain stage-A kernel
    serves (homogeneous of degree 1 like Euler, so the scaled states are the same flow)."""
    from exahype_amd.pde_codegen import SympyPDE
    from tests.test_user_pde import euler_sympy
    base = euler_sympy()
    q = base.q
    tenth = sympy.Rational(1, 10)

    def eig(qq, d):                           # |u_n| + c with |p| as the built-in Euler takes it (the face traces of a rough state can dip below 0)
        irho = 1 / qq[0]
        p = sympy.Float(0.4) * (qq[4] - sympy.Rational(1, 2) * irho * (qq[1] ** 2 + qq[2] ** 2 + qq[3] ** 2))
        return sympy.Abs(qq[d + 1] * irho) + sympy.sqrt(sympy.Float(1.4) * sympy.Abs(p) * irho) + tenth
    return SympyPDE(5, flux=lambda qq, d: [e.subs(dict(zip(q, qq))) for e in base.flux_exprs[d]],
                    max_eigenvalue=eig,
                    ncp=lambda qq, dq, d: [tenth * dq[0], 0, 0, 0, 0], max_dim=3, name="euler_ncp")


def plain_reference(u, dt, dx, N, n_it, p):
    from oracle import aderdg_numpy as A
    from oracle.dg_operators import operators
    from tests.test_user_pde import OracleXtPDE
    return A.step_xt(u, dt, dx, operators(N), OracleXtPDE(p), n_it=n_it, stages=True)


def plain_dt(u, dx, N, p, family):
    from tests.test_user_pde import NumpyPDE
    return hard_dt(u, dx, 3, N, family, pde=NumpyPDE(p))


# ---- CPU: the cases see their last iteration, and stay admissible at the CFL-0.9 step ------------------------------------------------------------
@pytest.mark.parametrize("family", list(STATES))
@pytest.mark.parametrize("label,dim,N,nc,stage_a,fused", C.HARD_KERNELS)
def test_hard_state_cases_see_the_last_iteration(label, dim, N, nc, stage_a, fused, family):
    u, dx = hard_input(dim, N, nc, family)
    dt = hard_dt(u, dx, dim, N, family)
    r = DgRef(u, dt, dx, dim, N, nc, 0 if fused else N)
    assert np.isfinite(r.steps(1)).all()
    if not fused:
        r.check_ustar(r.stage_a()[0])
        r.check_traces(r.stage_a()[1])
    r.check_steps(r.steps(1), 1)


@pytest.mark.parametrize("family", list(STATES))
def test_hard_state_plain_case_sees_the_last_iteration(family):
    _, dim, N, nc = PLAIN
    p = euler_ncp()
    u, dx = hard_input(dim, N, nc, family)
    dt = plain_dt(u, dx, N, p, family)
    ref, mut = plain_reference(u, dt, dx, N, N, p), plain_reference(u, dt, dx, N, N - 1, p)
    assert np.isfinite(ref["unew"]).all()
    assert_dg_parity(ref["ustar"], ref["ustar"], u, mut["ustar"], what="u*")
    assert_dg_parity(ref["unew"], ref["unew"], u, mut["unew"], what="step")


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from exahype_amd import solvers
    return solvers


def _solver(exa, dim, N, nc, stage_a, fused, dx, n_picard):
    if fused:
        s = exa.AderDgSolver(dim, N, nc, n_picard=0, dx=dx, fused_single_stage=True)
        assert s._fused
        return s
    return exa.AderDgSolver(dim, N, nc, n_picard=n_picard, dx=dx, stage_a=stage_a)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(STATES))
@pytest.mark.parametrize("label,dim,N,nc,stage_a,fused", C.HARD_KERNELS)
def test_hard_states_vs_oracle(exa, label, dim, N, nc, stage_a, fused, family):
    u, dx = hard_input(dim, N, nc, family)
    dt = hard_dt(u, dx, dim, N, family)
    r = DgRef(u, dt, dx, dim, N, nc, 0 if fused else N)
    s = _solver(exa, dim, N, nc, stage_a, fused, dx, -1)
    s.upload(u)
    if not fused:
        s.predictor_volume(dt)
        r.check_ustar(s.download())
        r.check_traces(s.trace.cpu().numpy())
        s.upload(u)
    s.step(dt)
    r.check_steps(s.download(), 1)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(STATES))
def test_hard_states_plain_generated_set_vs_numpy_oracle(exa, family):
    _, dim, N, nc = PLAIN
    p = euler_ncp()
    u, dx = hard_input(dim, N, nc, family)
    dt = plain_dt(u, dx, N, p, family)
    s = exa.AderDgSolver(dim, N, nc, pde=p.register(), n_vars=5, dx=dx)
    assert "plain" in s.stage_a_kernel_name()
    ref, mut = plain_reference(u, dt, dx, N, N, p), plain_reference(u, dt, dx, N, N - 1, p)
    s.upload(u)
    s.predictor_volume(dt)
    assert_dg_parity(s.download(), ref["ustar"], u, mut["ustar"], what="u*")
    s.upload(u)
    s.step(dt)
    assert_dg_parity(s.download(), ref["unew"], u, mut["unew"], what="step")


@pytest.mark.gpu
@pytest.mark.parametrize("label,dim,N,nc,stage_a,fused", [k for k in C.HARD_KERNELS if not k[5]])   # (the fused single stage has no Picard loop)
def test_negative_control_one_picard_iteration_short_is_rejected(exa, label, dim, N, nc, stage_a, fused):
    u, dx, dt = C.parity_input(dim, N, nc)
    r = DgRef(u, dt, dx, dim, N, nc, N)
    s = _solver(exa, dim, N, nc, stage_a, False, dx, N - 1)
    s.upload(u)
    s.predictor_volume(dt)
    e_us = dg_err(s.download().reshape(-1, 5), r.stage_a()[0].reshape(-1, 5), u.reshape(-1, 5))
    s.upload(u)
    s.step(dt)
    e_step = dg_err(s.download().reshape(-1, 5), r.steps(1).reshape(-1, 5), u.reshape(-1, 5))
    assert min(e_us, e_step) > 100 * DG_TOL, (label, e_us, e_step)


@pytest.mark.gpu
def test_negative_control_plain_generated_set(exa):
    _, dim, N, nc = PLAIN
    p = euler_ncp()
    u, dx = hard_input(dim, N, nc, "supersonic")
    dt = plain_dt(u, dx, N, p, "supersonic")
    ref = plain_reference(u, dt, dx, N, N, p)
    s = exa.AderDgSolver(dim, N, nc, pde=p.register(), n_vars=5, dx=dx, n_picard=N - 1)
    s.upload(u)
    s.step(dt)
    assert dg_err(s.download(), ref["unew"], u) > 100 * DG_TOL

"""The register-resident stage A (exa_dg_reg.hpp) when ONE workgroup walks every cell: the LDS of a cell in flight is then reused by the next cell of
the same half, which is where the closing schedule could go wrong -- the closing image lies in the arrays of the sums, and u* shares an interval
with the next cell's put of iteration 0: no barrier ends a cell.  The other small cases of the suite give every workgroup one trip; here
`set_reserve_cus(1 << 20)` clamps the persistent grid to one workgroup (dg_inst.hip persistent_grid; the constructor's `reserve_cus` argument is
read only by a partitioned solver, so every case sets the reserve after construction and checks that it holds).

Oracle cases (cells), built-in Euler against oracle/exa_oracle.c, tests/util.py dg_err, bound 1e-10, on u*, the traces and the stepped u:
    (1, 1, 5)  three trips, the late half idles through its last one
    (2, 2, 3)  six trips for each half
    (1, 1, 1)  the late half is never active
each with n_picard 6, 2 and 1 (1: the averages follow the fold of iteration 0) and anisotropic cells.  The same inputs on the default grid must
give the same bits (same arithmetic, different reuse of LDS).  Then a box launch, the one-kernel step (the FUSE instantiation keeps the barrier)
and generated term sets without put_fast, with a source, with an ncp and with x, t terms -- each against the reference and bound of its existing
test (tests/test_dg_wide_sets.py, tests/test_user_pde.py).
"""
import functools

import numpy as np
import pytest

from tests import dg_cases as C
from tests.test_stage_a_primitive_put import BLOCK, BOUND, BOX_HI, BOX_LO, N, errors, reference
from tests.util import DG_TOL, assert_dg_parity, cfl_dt, dg_err

pytestmark = pytest.mark.gpu
ONE_WORKGROUP = 1 << 20
CELLS = [(1, 1, 5), (2, 2, 3), (1, 1, 1)]
N_PICARD = [6, 2, 1]
NC = (2, 2, 3)                                                        # the other instantiations: six trips for each half


def clamp(s, reserve=ONE_WORKGROUP):
    """the persistent grid of solver s clamped by `reserve` workgroups (1 << 20: one workgroup walks every cell; 0: the default grid)"""
    s.set_reserve_cus(reserve)
    assert s.reserve_cus == reserve
    return s


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from exahype_amd import solvers
    return solvers


@functools.lru_cache(maxsize=None)
def stage_a_and_step(nc, n_picard, reserve):
    """(kernel name, u*, traces, stepped u) of one case on a grid clamped by `reserve`: run once, shared, never written"""
    from exahype_amd import solvers as exa
    u, dx, dt, _ = reference(nc, n_picard)
    s = clamp(exa.AderDgSolver(3, N, nc, n_picard=n_picard, dx=dx, stage_a="reg"), reserve)
    s.upload(u)
    s.predictor_volume(dt)
    ustar, trace = s.download().copy(), s.trace.cpu().numpy().copy()
    s.upload(u)
    s.step(dt)
    out = (s.stage_a_kernel_name(), ustar, trace, s.download().copy())
    for a in out[1:]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("n_picard", N_PICARD)
@pytest.mark.parametrize("nc", CELLS)
def test_one_workgroup_walks_every_cell_vs_oracle(exa, nc, n_picard):
    r = reference(nc, n_picard)[3]
    name, ustar, trace, unew = stage_a_and_step(nc, n_picard, ONE_WORKGROUP)
    assert "reg" in name
    e = errors(r, ustar, trace, unew, ("one workgroup", nc, n_picard))
    assert max(e.values()) < BOUND, e


@pytest.mark.parametrize("n_picard", N_PICARD)
@pytest.mark.parametrize("nc", CELLS)
def test_trip_count_does_not_change_a_bit(exa, nc, n_picard):
    one, default = stage_a_and_step(nc, n_picard, ONE_WORKGROUP), stage_a_and_step(nc, n_picard, 0)
    assert np.array_equal(one[1], default[1]), "u* depends on how many cells a workgroup walks"
    assert np.array_equal(one[2], default[2]), "the traces depend on how many cells a workgroup walks"


def test_one_workgroup_box_inside_a_block_vs_oracle(exa):
    u, dx, dt, r = reference(BLOCK, 6)
    s = clamp(exa.AderDgSolver(3, N, BLOCK, n_picard=6, dx=dx, stage_a="reg"))
    s.upload(u)
    s.predictor_volume(dt, BOX_LO, BOX_HI)
    us = s.download().reshape(BLOCK + (N ** 3, 5))
    want = r.stage_a()[0].reshape(BLOCK + (N ** 3, 5))
    inside = np.zeros(BLOCK, dtype=bool)
    inside[tuple(slice(l, h) for l, h in zip(BOX_LO, BOX_HI))] = True
    assert inside.sum() == 12
    assert np.array_equal(us[~inside], u.reshape(us.shape)[~inside]), "the box launch wrote outside its box"
    e_box = dg_err(us[inside].reshape(-1, 5), want[inside].reshape(-1, 5), u.reshape(us.shape)[inside].reshape(-1, 5))
    print("one workgroup, box: u* inside the box %.3e" % e_box)
    assert e_box < BOUND, e_box


def test_one_workgroup_one_kernel_step_vs_oracle(exa):
    """[A] [B o A] B with two different dt: the second step's launch is the FUSE instantiation"""
    u, dx, dt0, r = reference(NC, 6)
    dts = [C.steps_dt(dt0), 0.7 * C.steps_dt(dt0)]
    s = clamp(exa.AderDgSolver(3, N, NC, n_picard=6, dx=dx, stage_a="reg", one_kernel_step=True))
    assert s._one_kernel
    s.upload(u)
    for d in dts:
        s.step(d)
    e = dg_err(s.download().reshape(-1, 5), r.steps(2, dts=dts).reshape(-1, 5), u.reshape(-1, 5))
    print("one workgroup, one-kernel step: 2 steps %.3e" % e)
    assert e < BOUND, e


def test_one_workgroup_generated_set_without_put_fast_vs_numpy_oracle(exa):
    """tests/test_dg_wide_sets.py's ring4 (4 variables, the image q | aux): one CFL-0.9 step, DG_TOL, last Picard iteration visible"""
    from tests import wide_term_sets as W
    p = W.ring("ring4")
    u, dx, dt = W.wide_input("ring4", 3, N, NC)
    s = clamp(exa.AderDgSolver(3, N, NC, pde=p.register(), n_vars=p.n_vars, dx=dx, fused_single_stage=False))
    assert s.stage_a_kernel_name().startswith(W.REG) and "exa::UserPDE" in s.stage_a_kernel_name()
    s.upload(u)
    s.step(dt)
    want, mut = W.want_and_mutant("ring4", 3, N, NC, -1, 1)
    assert_dg_parity(s.download(), want, u, mut, tol=DG_TOL, what="ring4, one workgroup")


def test_one_workgroup_generated_set_with_a_source_vs_numpy_oracle(exa):
    """tests/test_user_pde.py's Euler + gravity (five variables and a source): two steps at CFL 0.7"""
    from oracle import aderdg_numpy as A
    from oracle.dg_operators import operators
    from tests.test_user_pde import NumpyPDE
    from tests.user_term_sets import euler_gravity
    from tests.util import euler_dg_state
    p = euler_gravity()
    u = euler_dg_state(NC + (N,) * 3, seed=60 + N)
    dx = [1.0 / c for c in NC]
    dt = cfl_dt(u, dx, 3, N, pde=NumpyPDE(p), cfl=0.7)
    s = clamp(exa.AderDgSolver(3, N, NC, pde=p.register(), n_vars=5, dx=dx))
    assert "reg_kernel" in s.stage_a_kernel_name()
    s.upload(u)
    ref, mut = u.copy(), u.copy()
    for _ in range(2):
        s.step(dt)
        ref = A.step(ref, dt, dx, operators(N), NumpyPDE(p))
        mut = A.step(mut, dt, dx, operators(N), NumpyPDE(p), n_it=N - 1)
    assert_dg_parity(s.download(), ref, u, mut, what="Euler + gravity, one workgroup, two steps")


@pytest.mark.parametrize("with_ncp,with_xt", [(True, True), (True, False), (False, True)])
def test_one_workgroup_ncp_and_position_time_terms_vs_numpy_oracle(exa, with_ncp, with_xt):
    """tests/test_user_pde.py's coupled system: an ncp runs phases of its own around iteration 0 and in front of the averages, x, t terms keep the
    barrier at the end of the cell; three steps with a non-zero origin and start time against oracle/aderdg_numpy.py step_xt"""
    from oracle import aderdg_numpy as A
    from oracle.dg_operators import operators
    from tests.test_user_pde import OracleXtPDE, coupled_xt_ncp_system
    p = coupled_xt_ncp_system(max_dim=3, with_ncp=with_ncp, with_xt=with_xt)
    o = OracleXtPDE(p)
    u = 1.0 + 0.3 * np.random.default_rng(306).random(NC + (N,) * 3 + (3,))
    dx = [(0.9, 1.1, 0.7)[a] / NC[a] for a in range(3)]
    origin = [0.25, -0.5, 1.0]
    x3 = A._coords(NC, N, operators(N), dx, origin)
    dt = cfl_dt(u, dx, 3, N, lam=max(float(np.max(o.maxeig(u, x3, 0.4, a) * np.ones(u.shape[:-1]))) for a in range(3)))
    s = clamp(exa.AderDgSolver(3, N, NC, pde=p.register(), n_vars=3, dx=dx, origin=origin, time=0.4))
    assert "reg_kernel" in s.stage_a_kernel_name()
    s.upload(u)
    ref, mut, t = u.copy(), u.copy(), 0.4
    for k in range(3):
        h = dt * (1 + 0.1 * k)
        s.step(h)
        ref = A.step_xt(ref, h, dx, operators(N), o, t=t, origin=origin, n_it=N)
        mut = A.step_xt(mut, h, dx, operators(N), o, t=t, origin=origin, n_it=N - 1)
        t += h
    assert_dg_parity(s.download(), ref, u, mut, what="coupled system ncp %s x,t %s, one workgroup" % (with_ncp, with_xt))

"""ADER-DG domain boundaries without a GPU: the boundary dict's validation, which block faces of a process grid are domain faces, and the
numpy restatement of the non-periodic step (a box between two walls is the mirrored periodic box of twice its length)."""
import re

import numpy as np
import pytest

from exahype_amd import Dirichlet, Outflow, Wall
from exahype_amd.boundary import coefficients, validate_boundary
from exahype_amd.solvers import CartesianPartition
from oracle import aderdg_numpy as A
from oracle.dg_operators import operators
from tests import dg_boundary_numpy as B
from tests.util import cfl_dt, euler_dg_state

PDE_EULER_REF2D, PDE_EULER, PDE_ADVECTION = 0, 1, 2


def test_validate_resolves_wall_signs_and_keeps_the_rest():
    f = lambda x, t: x      # noqa: E731
    out = validate_boundary({(0, 0): Wall(), (0, 1): Outflow(), (2, 1): Dirichlet(np.arange(5.0)), (1, 0): Dirichlet(f)}, 3, 5, PDE_EULER)
    assert np.array_equal(out[(0, 0)].sign, [1, -1, 1, 1, 1])
    assert isinstance(out[(0, 1)], Outflow) and out[(1, 0)].state is f and not out[(1, 0)].constant
    assert np.array_equal(coefficients(out[(0, 0)], 5), [1, -1, 1, 1, 1, -1, 1, -1, -1, -1])
    assert np.array_equal(coefficients(out[(0, 1)], 5), np.ones(10))
    assert np.array_equal(coefficients(out[(2, 1)], 5), np.arange(5.0))
    assert coefficients(out[(1, 0)], 5) is None
    assert np.array_equal(validate_boundary({(1, 1): Wall()}, 2, 5, PDE_EULER_REF2D)[(1, 1)].sign, [1, 1, -1, 1, 1])
    assert validate_boundary(None, 3, 5, PDE_EULER) == {} and validate_boundary({}, 2, 5, PDE_EULER) == {}
    s = validate_boundary({(0, 0): Wall(sign=[1, -1])}, 2, 2, PDE_ADVECTION)[(0, 0)].sign
    assert np.array_equal(s, [1, -1])


@pytest.mark.parametrize("bad,dim,nv,pde,what", [
    ({(3, 0): Outflow()}, 3, 5, PDE_EULER, "axis 3"),
    ({(2, 0): Outflow()}, 2, 5, PDE_EULER, "axis 2"),
    ({(-1, 0): Outflow()}, 2, 5, PDE_EULER, "axis -1"),
    ({(0, 2): Outflow()}, 2, 5, PDE_EULER, "side 2"),
    ({0: Outflow()}, 2, 5, PDE_EULER, "not (axis, side)"),
    ({(0, 0): "wall"}, 2, 5, PDE_EULER, "is not Outflow"),
    ({(0, 0): Dirichlet([1.0, 0, 0, 2.5])}, 3, 5, PDE_EULER, "shape"),
    ({(0, 0): Dirichlet([1.0, 0, 0, np.nan, 2.5])}, 3, 5, PDE_EULER, "not finite"),
    ({(0, 0): Wall()}, 3, 1, PDE_ADVECTION, "needs sign"),
    ({(0, 0): Wall()}, 3, 5, 100, "needs sign"),
    ({(0, 0): Wall(sign=[1, -1, 1])}, 3, 5, PDE_EULER, "3 entries"),
    ({(0, 0): Wall(sign=[1, -1, 1, 1, 0.5])}, 3, 5, PDE_EULER, "+1 / -1"),
    ([(0, 0)], 3, 5, PDE_EULER, "a dict"),
])
def test_validate_rejects(bad, dim, nv, pde, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        validate_boundary(bad, dim, nv, pde)


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_domain_face_of_every_rank(world):
    for rank in range(world):
        p = CartesianPartition(world, rank, 3)
        for d in range(3):
            for side in range(2):
                want = p.pdims[d] == 1 or p.coords[d] == (0 if side == 0 else p.pdims[d] - 1)
                assert p.domain_face(d, side) == want
        # a face is a domain face of exactly one rank of its pencil, or of every rank where the grid has extent 1
        for d in range(3):
            if p.pdims[d] == 1:
                assert p.domain_face(d, 0) and p.domain_face(d, 1)
    if world == 2:
        lo, hi = CartesianPartition(2, 0, 3), CartesianPartition(2, 1, 3)
        assert lo.pdims[0] == 2
        assert lo.domain_face(0, 0) and not lo.domain_face(0, 1) and hi.domain_face(0, 1) and not hi.domain_face(0, 0)
    if world == 8:
        for rank in range(8):
            p = CartesianPartition(8, rank, 3)
            assert sum(p.domain_face(d, s) for d in range(3) for s in range(2)) == 3      # a 2x2x2 grid: every rank touches 3 faces


def test_domain_face_exchange_self():
    """The RCCL-to-self rehearsal: the direction goes through the exchange, but it is still the whole domain along it."""
    p = CartesianPartition(1, 0, 3, exchange_self=(0, 2))
    assert p.partitioned(0) and p.partitioned(2) and not p.partitioned(1)
    assert all(p.domain_face(d, s) for d in range(3) for s in range(2))


def _run(u, dt, dx, ops, bcs, steps=1):
    for _ in range(steps):
        u = B.step(u, dt, dx, ops, A.Euler(), bcs)
    return u


@pytest.mark.parametrize("dim,N,nc", [(2, 4, (3, 2)), (3, 3, (2, 2, 2))])
def test_numpy_walls_equal_the_mirrored_periodic_box(dim, N, nc):
    """Walls at both x ends of n cells == the periodic run on 2 n cells holding the data and its mirror image, restricted to the first half."""
    ops = operators(N)
    u = euler_dg_state(tuple(nc) + (N,) * dim, seed=7)
    dx = [0.5] * dim
    dt = cfl_dt(u, dx, dim, N, cfl=0.6)
    s = np.ones(5)
    s[1] = -1.0
    got = _run(u, dt, dx, ops, {(0, 0): ("wall", s), (0, 1): ("wall", s)}, steps=2)
    big = np.concatenate([u, B.mirror_x(u)], axis=0)
    want = big
    for _ in range(2):
        want = A.step(want, dt, dx, ops, A.Euler())
    assert np.max(np.abs(got - want[:nc[0]])) <= 1e-12 * np.max(np.abs(want))


def test_numpy_periodic_bcs_reduce_to_the_oracle():
    """No condition == the periodic oracle step; Dirichlet with the periodic neighbour's traces == periodic too."""
    dim, N, nc = 3, 3, (3, 2, 2)
    ops = operators(N)
    u = euler_dg_state(tuple(nc) + (N,) * dim, seed=3)
    dx = [0.3] * dim
    dt = cfl_dt(u, dx, dim, N, cfl=0.6)
    want = A.step(u, dt, dx, ops, A.Euler())
    assert np.max(np.abs(B.step(u, dt, dx, ops, A.Euler(), {}) - want)) <= 1e-14 * np.max(np.abs(want))
    st = B.step(u, dt, dx, ops, A.Euler(), {}, stages=True)
    qL, qR, FL, FR = st["traces"][1]
    bcs = {(1, 0): ("dirichlet", (np.take(qR, nc[1] - 1, axis=1), np.take(FR, nc[1] - 1, axis=1))),
           (1, 1): ("dirichlet", (np.take(qL, 0, axis=1), np.take(FL, 0, axis=1)))}
    assert np.max(np.abs(B.step(u, dt, dx, ops, A.Euler(), bcs) - want)) <= 1e-14 * np.max(np.abs(want))
    assert np.array_equal(B.step(u, dt, dx, ops, A.Euler(), {}), want)                      # (the same operations in the same order)
    # the form with x, t and an ncp: no condition == step_xt, bit for bit
    pytest.importorskip("sympy")
    from tests.dg_boundary_cases import ORIGIN, T0, coupled_system
    o = coupled_system(3)[1]
    v = 1.0 + 0.3 * np.random.default_rng(3).random(tuple(nc) + (N,) * dim + (3,))
    want = A.step_xt(v, dt, dx, ops, o, t=T0, origin=ORIGIN)
    assert np.array_equal(B.step_xt(v, dt, dx, ops, o, {}, t=T0, origin=ORIGIN), want)
    assert np.array_equal(B.step_xt(v, dt, dx, ops, o, {}, t=T0, origin=ORIGIN, n_it=N - 1), A.step_xt(v, dt, dx, ops, o, t=T0, origin=ORIGIN, n_it=N - 1))


def test_numpy_outflow_of_a_uniform_state_is_steady():
    dim, N, nc = 2, 3, (3, 2)
    ops = operators(N)
    q0 = np.array([1.2, 0.3, -0.1, 0.0, 3.0])
    u = np.broadcast_to(q0, tuple(nc) + (N,) * dim + (5,)).copy()
    bcs = {(a, s): ("outflow",) for a in range(dim) for s in range(2)}
    got = B.step(u, 0.01, [0.5, 0.5], ops, A.Euler(), bcs)
    assert np.max(np.abs(got - u)) < 1e-13

"""The ADER-DG oracles against a long-double reference, and the sensitivity of every ADER-DG GPU case table.

1. oracle/aderdg_numpy.py run end to end in np.longdouble on the operators of oracle.dg_operators.operators_hp (built in mpmath from closed
   forms) is the reference; the fp64 C oracle (stage A, stage B, two steps) and the fp64 numpy step_xt (source + ncp, what
   tests/test_user_pde.py compares with) must match it to 1e-13 of the per-variable increment (tests/util.py dg_err) at the CFL-0.9 step.
2. Every case table of the GPU parity tests (tests/dg_cases.py), with the oracle as `got`: each n_it > 0 case must see its last Picard
   iteration (the mutant with n_it - 1 iterations >= 100 * DG_TOL).  A step shrunk until the case goes blind fails here.
3. The sharded tables (tests/test_gpu_distributed.py) on every rank's cells of the global result: the same, and a block stepped alone (no ghosts),
   a shard evaluated without its offset and a rank that keeps its own CFL maximum are all seen.  (The limited ones: tests/test_limiter.py.)
"""
import numpy as np
import pytest

import oracle
from oracle import aderdg_numpy as A
from oracle.dg_operators import operators, operators_hp
from tests import dg_cases as C
from tests.util import ADV_A, DG_TOL, cfl_dt, dg_err, dg_max_eigenvalue, euler_dg_state

HP_TOL = 1e-13


def test_operators_hp_are_exact():
    for N in range(2, 9):
        h, o = operators_hp(N), operators(N)
        assert all(h[k].dtype == np.longdouble for k in ("xi", "w", "D", "Kxi", "phiL", "phiR", "iK1", "F0"))
        eps = float(np.finfo(np.longdouble).eps)
        assert abs(float(h["w"].sum() - 1)) < 8 * eps
        for k in range(2 * N):                                               # Gauss: exact for degree <= 2N - 1
            assert abs(float(h["w"] @ h["xi"] ** k - np.longdouble(1) / (k + 1))) < 16 * eps
        for k in range(N):                                                   # D exact on degree <= N - 1
            want = k * h["xi"] ** (k - 1) if k else 0 * h["xi"]
            assert float(np.max(np.abs(h["D"] @ h["xi"] ** k - want))) < 1e4 * eps
        assert float(np.max(np.abs(h["iK1"] @ h["K1"] - np.eye(N)))) < 1e3 * eps
        for key in ("xi", "w", "D", "Kxi", "phiL", "phiR", "iK1"):          # and the fp64 operators are their rounding
            assert np.max(np.abs(o[key] - h[key].astype(np.float64))) < 1e-13 * max(1.0, float(np.max(np.abs(h[key])))), (N, key)


def _c_to_numpy_traces(st, dim, m, ncells):
    """numpy traces (per direction qL, qR, FL, FR) in the C oracle's layout [dim, 2 (L, R), cell, 2 (q, F), m, Nf]."""
    out = []
    for a in range(dim):
        qL, qR, FL, FR = st["traces"][a]
        sides = []
        for qq, FF in ((qL, FL), (qR, FR)):
            sides.append(np.stack([np.moveaxis(qq, -1, dim).reshape(ncells, m, -1), np.moveaxis(FF, -1, dim).reshape(ncells, m, -1)], axis=1))
        out.append(np.stack(sides))
    return np.stack(out)


HP_CASES = [(dim, N, nc) for dim, ncs in ((2, [(3, 1), (1, 2)]), (3, [(2, 1, 1), (1, 1, 1)])) for N in range(2, 9) for nc in ncs[N % 2:N % 2 + 1]]


@pytest.mark.parametrize("pde", ["euler", "advection"])
@pytest.mark.parametrize("dim,N,nc", HP_CASES)
def test_c_oracle_vs_long_double_reference(dim, N, nc, pde):
    m = 5 if pde == "euler" else 3
    pid = C.PDE_EULER if pde == "euler" else C.PDE_ADVECTION
    npde = A.Euler() if pde == "euler" else A.Advection(ADV_A, m)
    shape = tuple(nc) + (N,) * dim
    if pde == "euler":
        u = euler_dg_state(shape, seed=7 * N + dim)
    else:
        u = 1.0 + 0.3 * np.random.default_rng(N).random(shape + (m,))
    dx = [(1.0, 0.8, 1.3)[a] / nc[a] for a in range(dim)]
    dt = cfl_dt(u, dx, dim, N, pde=pid, m=m)
    ops, hp = operators(N), operators_hp(N)
    ul = u.astype(np.longdouble)
    st = A.step(ul, dt, dx, hp, npde, stages=True)
    assert st["unew"].dtype == np.longdouble and st["ustar"].dtype == np.longdouble
    ncells = int(np.prod(nc))
    us, tr = oracle.aderdg_stage_a(u.reshape(-1), dt, dx, ops, dim, N, m, pid, N)
    us0, tr0 = oracle.aderdg_stage_a(u.reshape(-1), dt, dx, ops, dim, N, m, pid, 0)
    e = [dg_err(us.reshape(u.shape), st["ustar"], ul),
         dg_err(tr, _c_to_numpy_traces(st, dim, m, ncells), tr0, var_axis=4)]
    un = oracle.aderdg_stage_b(us, tr, dt, dx, ops, dim, N, m, pid, nc)
    e.append(dg_err(un.reshape(u.shape), st["unew"], ul))
    u2 = oracle.aderdg_step(oracle.aderdg_step(u.reshape(-1), dt, dx, ops, dim, N, m, pid, N, nc), dt, dx, ops, dim, N, m, pid, N, nc)
    ref2 = A.step(A.step(ul, dt, dx, hp, npde), dt, dx, hp, npde)
    e.append(dg_err(u2.reshape(u.shape), ref2, ul))
    assert max(e) <= HP_TOL, e


def _coupled_system(dim):
    pytest.importorskip("sympy")
    from tests.test_user_pde import OracleXtPDE, coupled_xt_ncp_system
    return OracleXtPDE(coupled_xt_ncp_system(max_dim=dim, with_ncp=True, with_xt=True))


@pytest.mark.parametrize("dim,N,nc", [(2, 4, (2, 3)), (3, 3, (2, 2, 2)), (2, 8, (2, 2)), (3, 6, (1, 1, 2)), (3, 8, (1, 2, 1))])
def test_numpy_step_xt_vs_long_double_reference(dim, N, nc):
    """step_xt with a position/time-dependent flux, source and ncp (tests/test_user_pde.py's coupled system) in fp64 == in long double."""
    o = _coupled_system(dim)
    u = 1.0 + 0.3 * np.random.default_rng(100 * dim + N).random(tuple(nc) + (N,) * dim + (3,))
    dx = [(0.9, 1.1, 0.7)[a] / nc[a] for a in range(dim)]
    origin = [0.25, -0.5, 1.0][:dim]
    x3 = A._coords(tuple(nc), N, operators(N), dx, origin)
    lam = max(float(np.max(o.maxeig(u, x3, 0.4, a) * np.ones(u.shape[:-1]))) for a in range(dim))
    dt = cfl_dt(u, dx, dim, N, lam=lam)
    ul = u.astype(np.longdouble)
    a64 = A.step_xt(u, dt, dx, operators(N), o, t=0.4, origin=origin, stages=True)
    ahp = A.step_xt(ul, dt, dx, operators_hp(N), o, t=0.4, origin=origin, stages=True)
    assert ahp["unew"].dtype == np.longdouble
    e = [dg_err(a64["ustar"], ahp["ustar"], ul), dg_err(a64["unew"], ahp["unew"], ul)]
    b64 = A.step_xt(a64["unew"], dt, dx, operators(N), o, t=0.4 + dt, origin=origin)
    bhp = A.step_xt(ahp["unew"], dt, dx, operators_hp(N), o, t=0.4 + dt, origin=origin)
    e.append(dg_err(b64, bhp, ul))
    assert max(e) <= HP_TOL, e


# ---- every GPU case table sees its last Picard iteration (the oracle against itself: err 0, mutant >= 100 * DG_TOL) ----------------------------
@pytest.mark.parametrize("dim,N,nc", C.DG_CASES)
@pytest.mark.parametrize("n_picard", [-1, 0])
def test_dg_cases_see_the_last_iteration(dim, N, nc, n_picard):
    u, dx, dt = C.parity_input(dim, N, nc)
    r = C.DgRef(u, dt, dx, dim, N, nc, C.n_it_of(N, n_picard))
    r.check_ustar(r.stage_a()[0])
    r.check_traces(r.stage_a()[1])
    r.check_stage_b(r.stage_b())
    dts = [C.steps_dt(dt, single_stage=n_picard == 0)] * 3
    r.check_steps(r.steps(3, dts=dts), 3, dts=dts)


@pytest.mark.parametrize("N,nc,box", C.TILE_ORDER_CASES)
def test_tile_order_cases_see_the_last_iteration(N, nc, box):
    u, dx, dt = C.tile_order_input(N, nc)
    r = C.DgRef(u, dt, dx, 3, N, nc, N)
    r.check_stage_b(r.stage_b())


@pytest.mark.parametrize("N,nc", C.MULTIPASS_CASES + [C.BOX_MULTIPASS_CASE])
def test_multipass_cases_see_the_last_iteration(N, nc):
    u, dx, dt = C.multipass_input(N, nc, seed=606 if (N, nc) == C.BOX_MULTIPASS_CASE else None)
    r = C.DgRef(u, dt, dx, 3, N, nc, N)
    r.check_ustar(r.stage_a()[0])
    r.check_traces(r.stage_a()[1])
    r.check_steps(r.steps(1), 1)
    dts = [C.steps_dt(dt)] * 2
    r.check_steps(r.steps(2, dts=dts), 2, dts=dts)


@pytest.mark.parametrize("nc,n_picard", C.VARIANT_N6_CASES)
def test_variant_n6_cases_see_the_last_iteration(nc, n_picard):
    u, dx, dt = C.variant_n6_input(nc, n_picard)
    r = C.DgRef(u, dt, dx, 3, 6, nc, C.n_it_of(6, n_picard))
    r.check_ustar(r.stage_a()[0])
    r.check_traces(r.stage_a()[1])
    dts = [C.steps_dt(dt)] * 2
    r.check_steps(r.steps(2, dts=dts), 2, dts=dts)


@pytest.mark.parametrize("nc,n_picard", C.VARIANT_N8_CASES)
def test_variant_n8_cases_see_the_last_iteration(nc, n_picard):
    u, dx, dt = C.variant_n8_input(nc, n_picard)
    r = C.DgRef(u, dt, dx, 3, 8, nc, C.n_it_of(8, n_picard))
    r.check_ustar(r.stage_a()[0])
    r.check_traces(r.stage_a()[1])


@pytest.mark.parametrize("nc,n_picard", C.ONE_KERNEL_CASES)
def test_one_kernel_cases_see_the_last_iteration(nc, n_picard):
    u, dx, dts = C.one_kernel_input(nc)
    r = C.DgRef(u, dts[0], dx, 3, 6, nc, C.n_it_of(6, n_picard))
    steps = len(dts) if np.prod(nc) < 100 else 3
    for k in ((2, steps) if steps > 2 else (steps,)):
        r.check_steps(r.steps(k, dts=dts), k, dts=dts)


# ---- the sharded cases (tests/test_gpu_distributed.py), on every rank's cells: last iteration seen, ghosts seen, shard offset seen ------------
@pytest.mark.parametrize("N,nc,pdims,one_kernel", C.SHARDED_CASES)
def test_sharded_cases_see_the_last_iteration_and_the_ghosts(N, nc, pdims, one_kernel):
    G, u, dx, dts = C.sharded_input(N, nc, pdims)
    u, want, mutant = C.steps_ref(u, dx, N, G, dts)
    C.check_rank_slices(u, want, mutant, C.rank_slices(nc, pdims), lambda r, sl: C.steps_ref(u[sl], dx, N, nc, dts)[1], what="sharded %s" % (G,))


@pytest.mark.parametrize("N,nc,limited", [c for c in C.SHARDED_SELF_CASES if not c[2]])
def test_sharded_self_cases_see_the_last_iteration(N, nc, limited):
    """(one rank that is its own neighbour: the block alone IS the grid, there is no second run to tell it from)"""
    G, u, dx, dts = C.sharded_self_input(N, nc, limited)
    u, want, mutant = C.steps_ref(u, dx, N, G, dts)
    C.check_rank_slices(u, want, mutant, C.rank_slices(nc, [1, 1, 1]), what="rccl to self %s" % (G,))


@pytest.mark.parametrize("N,nc", C.EIGHT_SHARD_CASES)
def test_eight_shard_cases_see_the_last_iteration_and_the_ghosts(N, nc):
    G, u, dx, dts = C.eight_shard_input(N, nc)
    u, want, mutant = C.steps_ref(u, dx, N, G, dts)
    C.check_rank_slices(u, want, mutant, C.rank_slices(nc, [2, 2, 2]), lambda r, sl: C.steps_ref(u[sl], dx, N, nc, dts)[1], what="eight shards %s" % (G,))


def test_sharded_xt_case_sees_the_last_iteration_the_ghosts_and_the_shard_offset():
    pytest.importorskip("sympy")
    dim, N, nc, pdims = C.SHARDED_XT_CASE
    p, o, G, u, dx, dt = C.sharded_xt_input()
    u, want, mutant = C.xt_ref(o, u, dx, dt, N)
    slices = C.rank_slices(nc, pdims)
    offset = lambda sl: [C.XT_ORIGIN[a] + sl[a].start * dx[a] for a in range(dim)]      # noqa: E731
    C.check_rank_slices(u, want, mutant, slices, lambda r, sl: C.xt_ref(o, u[sl], dx, dt, N, origin=offset(sl))[1], what="x/t + ncp")
    # a shard that evaluates its terms at the global origin (its offset left out): the whole grid shifted so that the shard's cells sit there
    sl = slices[1]
    assert offset(sl) != C.XT_ORIGIN
    shifted = C.xt_ref(o, u, dx, dt, N, origin=[2 * C.XT_ORIGIN[a] - offset(sl)[a] for a in range(dim)])[1]
    e = dg_err(shifted[sl], want[sl], u[sl])
    assert e >= 100 * DG_TOL, e


@pytest.mark.parametrize("N,nc,pdims", C.SHARDED_RUN_CASES)
def test_sharded_run_cases_see_the_reduction(N, nc, pdims):
    """run() on two shards: three steps; the largest eigenvalue is rank 1's and 1.5 times rank 0's, so a rank 0 that skips the all_reduce takes
    another step count or ends elsewhere."""
    G, u, dx, t_end = C.sharded_run_input(N, nc, pdims)
    slices = C.rank_slices(nc, pdims)
    lam = [dg_max_eigenvalue(u[sl], 3) for sl in slices]
    assert lam[1] == dg_max_eigenvalue(u, 3) and lam[1] >= 1.5 * lam[0], lam
    steps, t, want = C.run_replay(u, dx, N, G, t_end)
    assert steps == 3 and abs(t - t_end) <= 1e-14 * t_end
    m_steps, _, mutant = C.run_replay(u, dx, N, G, t_end, n_it=N - 1)
    assert m_steps == 3
    C.check_rank_slices(u, want, mutant, slices, lambda r, sl: C.run_replay(u[sl], dx, N, nc, t_end)[2], what="run %s" % (G,))
    l_steps, _, local = C.run_replay(u, dx, N, G, t_end, lam_of=lambda state: dg_max_eigenvalue(state[slices[0]], 3))
    assert l_steps != steps or dg_err(local[slices[0]], want[slices[0]], u[slices[0]]) >= 100 * DG_TOL, l_steps

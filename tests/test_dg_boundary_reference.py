"""The ADER-DG domain-boundary restatement (tests/dg_boundary_numpy.py) without a GPU: what tests/test_gpu_dg_boundary.py compares the kernels with.

1. Anchor: the fp64 restatement against its own run in np.longdouble on operators_hp, for every row and kind set of tests/dg_boundary_cases.py:
   u* and the new state after one step (CFL 0.9) and after two, to HP_TOL of the per-variable increment.
2. Reduction: with no face named it is the periodic oracle step (aderdg_numpy.step / step_xt), bit for bit.
3. Sensitivity: with the restatement as `got`, every case sees every mutant that applies to it (dg_boundary_cases.MUTANTS_OF) at 100 * DG_TOL, and
   every mutant is seen by at least two rows.  The run() replay and the sharded case: the same for theirs."""
import numpy as np
import pytest

from oracle import aderdg_numpy as A
from oracle.dg_operators import operators
from tests import dg_boundary_cases as BC
from tests import dg_boundary_numpy as B
from tests.dg_cases import rank_slices
from tests.test_dg_reference_hp import HP_TOL
from tests.util import DG_TOL, dg_err

pytest.importorskip("sympy")          # (the x / t rows: tests/test_user_pde.py's term set)
ALL_CASES = [("euler",) + c for c in BC.EULER_CASES] + [("xt",) + c for c in BC.XT_CASES]
IDS = [t + "-" + BC.case_id((r, k)) for t, r, k in ALL_CASES]


@pytest.mark.parametrize("table,row,kind", ALL_CASES, ids=IDS)
def test_restatement_vs_long_double(table, row, kind):
    c = BC.get_case(table, row, kind)
    ul = c.u.astype(np.longdouble)
    e = []
    for dts in (None, c.dts):
        got, want = c.run(dts=dts), c.run(hp=True, dts=dts)
        assert want[-1]["unew"].dtype == np.longdouble and want[-1]["ustar"].dtype == np.longdouble
        e += [dg_err(got[-1]["ustar"], want[-1]["ustar"], want[-2]["unew"] if len(want) > 1 else ul), dg_err(got[-1]["unew"], want[-1]["unew"], ul)]
    print("anchor %s %s: u* %.2e, u %.2e; two steps: u* %.2e, u %.2e" % ((table, BC.case_id((row, kind))) + tuple(e)))
    assert max(e) <= HP_TOL, e


@pytest.mark.parametrize("table,row", [("euler", r) for r in BC.EULER_ROWS] + [("xt", r) for r in BC.XT_ROWS])
def test_no_face_named_is_the_periodic_oracle_bit_for_bit(table, row):
    c = BC.get_case(table, row, "all_faces")
    ops = operators(c.N)
    if table == "euler":
        want = A.step_single_stage(c.u, c.dt, c.dx, ops, c.pde) if c.n_it == 0 else A.step(c.u, c.dt, c.dx, ops, c.pde)
        got = B.step(c.u, c.dt, c.dx, ops, c.pde, {}, n_it=c.n_it)
    else:
        want = A.step_xt(c.u, c.dt, c.dx, ops, c.pde, t=c.t0, origin=c.origin)
        got = B.step_xt(c.u, c.dt, c.dx, ops, c.pde, {}, t=c.t0, origin=c.origin)
    assert np.array_equal(got, want)
    assert not np.array_equal(c.state(), want)


@pytest.mark.parametrize("table,row,kind", ALL_CASES, ids=IDS)
def test_every_case_sees_its_mutants(table, row, kind):
    c = BC.get_case(table, row, kind)
    assert set(c.mutants()) <= set(BC.ALL_MUTANTS)
    for dts in (None, c.dts):                      # what the GPU tests run: one step (Euler rows), two steps (x / t rows)
        if (dts is None) != (table == "euler"):
            continue
        want = c.state(dts=dts)
        assert np.isfinite(want).all()
        for m in c.mutants():
            e = dg_err(c.state(m, dts=dts), want, c.u)
            print("mutant %s %s %s: %.2e" % (table, BC.case_id((row, kind)), m, e))
            assert e >= 100 * DG_TOL, (m, e)


def test_every_mutant_is_seen_by_two_rows():
    rows = {m: set() for m in BC.ALL_MUTANTS}
    for table, row, kind in ALL_CASES:
        for m in BC.get_case(table, row, kind).mutants():
            rows[m].add((table, row))
    assert all(len(r) >= 2 for r in rows.values()), {m: len(r) for m, r in rows.items()}


@pytest.mark.parametrize("table,row,kind", BC.RUN_CASES)
def test_run_replay_sees_the_last_iteration_and_the_dirichlet_eigenvalue(table, row, kind):
    c = BC.get_case(table, row, kind)
    t_end = c.t_end()
    steps, t, want = c.replay(t_end)
    assert steps == 3 and abs(t - t_end) <= 1e-14 * t_end and np.isfinite(want).all()
    m_steps, _, mutant = c.replay(t_end, mutant="picard")
    assert m_steps == 3 and dg_err(mutant, want, c.u) >= 100 * DG_TOL
    if table == "xt":
        # the constant state's eigenvalue at the face nodes sets the step: taken without position and time the loop ends elsewhere
        assert c.dirichlet_eigenvalue(c.t0, kinds=("const",)) > max(c.state_eigenvalue(c.u, c.t0), c.dirichlet_eigenvalue(c.t0), c.const_eigenvalue_without_xt())
        x_steps, _, x0 = c.replay(t_end, mutant="const_lambda_x0")
        assert x_steps != steps or dg_err(x0, want, c.u) >= 100 * DG_TOL


def test_sharded_case_sees_its_mutants_and_the_shard_offset():
    c = BC.sharded_xt_bc_case()
    dim, N, nc, pdims = BC.SHARDED_XT_BC_CASE
    want, ul = c.state(dts=c.dts), c.u.astype(np.longdouble)
    assert dg_err(want, c.state(hp=True, dts=c.dts), ul) <= HP_TOL
    slices = rank_slices(nc, pdims)
    for m in c.mutants():
        e = [dg_err(c.state(m, dts=c.dts)[sl], want[sl], c.u[sl]) for sl in slices]
        print("sharded mutant %s: %s" % (m, e))
        assert max(e) >= 100 * DG_TOL, (m, e)
    e = dg_err(BC.rank_without_its_offset(c, slices[1], c.dts)[slices[1]], want[slices[1]], c.u[slices[1]])
    print("sharded, rank 1 without its offset: %.2e" % e)
    assert e >= 100 * DG_TOL, e

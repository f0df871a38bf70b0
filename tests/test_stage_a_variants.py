"""GPU parity of the two stage-A kernels built for 3-D, N = 6 (include/exahype_hip.h EXA_STAGE_A_LDS / EXA_STAGE_A_REG):
each against the CPU oracle on the same seeded inputs at the CFL-0.9 step (tests/util.py assert_dg_parity: DG_TOL of the per-variable
increment, relative 1e-10, and a case that sees the last Picard iteration; ADER-DG is "parity unpinned" against the reference, which holds
no ADER-DG -- see tests/test_gpu_parity.py), and against each other.

The register-resident kernel (exa_dg_reg.hpp) runs a persistent grid of two workgroups per CU that walk over the cells, so
the cases cover: fewer cells than workgroups, more cells than resident workgroups (several cells per workgroup, not a
multiple), sub-boxes of a block (shell / interior launches of the sharded step), anisotropic cells, 1..N Picard iterations.
"""
import numpy as np
import pytest

from tests import dg_cases as C
from tests.dg_cases import DgRef
from tests.util import euler_dg_state, rel_err

pytestmark = pytest.mark.gpu
N = 6


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from exahype_amd import solvers
    return solvers


@pytest.fixture(scope="module")
def orc():
    import oracle
    oracle.lib()
    return oracle


@pytest.mark.parametrize("variant", ["reg", "lds"])
@pytest.mark.parametrize("nc,n_it", C.VARIANT_N6_CASES)
def test_stage_a_variant_vs_oracle(exa, orc, variant, nc, n_it):
    u, dx, dt = C.variant_n6_input(nc, n_it)                         # anisotropic cells: the per-direction scale is a lane property in the reg kernel
    r = DgRef(u, dt, dx, 3, N, nc, C.n_it_of(N, n_it))
    s = exa.AderDgSolver(3, N, nc, n_picard=n_it, dx=dx, stage_a=variant)
    s.upload(u)
    s.predictor_volume(dt)
    r.check_ustar(s.download())
    r.check_traces(s.trace.cpu().numpy())
    # two full steps (stage B reads what stage A left)
    s.upload(u)
    dts = [C.steps_dt(dt)] * 2
    for d in dts:
        s.step(d)
    r.check_steps(s.download(), 2, dts=dts)


@pytest.mark.parametrize("variant", ["reg", "lds"])
@pytest.mark.parametrize("nc,n_it", C.VARIANT_N8_CASES)
def test_stage_a_variant_n8_vs_oracle(exa, orc, variant, nc, n_it):
    """cfg 4's order (N = 8): "reg" = the matrix-pipe kernel with the iterate in registers (exa_dg_m8.hpp), "lds" = the level-streamed
    kernel with the slab (exa_dg_stream.hpp); 294 cells > 256 resident workgroups in the last case."""
    N8 = 8
    u, dx, dt = C.variant_n8_input(nc, n_it)
    r = DgRef(u, dt, dx, 3, N8, nc, C.n_it_of(N8, n_it))
    s = exa.AderDgSolver(3, N8, nc, n_picard=n_it, dx=dx, stage_a=variant)
    assert ("m8" in s.stage_a_kernel_name()) == (variant == "reg")
    s.upload(u)
    s.predictor_volume(dt)
    r.check_ustar(s.download())
    r.check_traces(s.trace.cpu().numpy())


def test_stage_a_variants_agree_on_boxes(exa):
    """shell / interior box launches of the 2x2x2 partition: both kernels, box by box, give the same block (to rounding)."""
    nc = (9, 8, 7)
    u = euler_dg_state(tuple(nc) + (N,) * 3, seed=4242)
    dt = 1e-3
    out = {}
    for variant in ("reg", "lds"):
        s = exa.AderDgSolver(3, N, nc, stage_a=variant)
        s.upload(u)
        shell, interior = exa.CartesianPartition(8, 0, 3).shell_and_interior(nc)
        for lo, hi in shell + [interior]:
            s.predictor_volume(dt, lo, hi)
        out[variant] = (s.download().copy(), s.trace.cpu().numpy().copy())
    assert rel_err(out["reg"][0], out["lds"][0]) < 1e-12
    assert rel_err(out["reg"][1], out["lds"][1]) < 1e-12
    assert not np.array_equal(out["reg"][0], u)


RESERVE_CASES = [(6, (3, 2, 2), "reg"), (6, (3, 2, 2), "lds"), (8, (2, 2, 1), "reg")]
_reserve_ref = {}


def _reserve_case(order, nc):
    """input and oracle of a reserve case, computed once per (order, cells) and left unchanged"""
    if (order, nc) not in _reserve_ref:
        u, dx, dt = (C.variant_n6_input if order == 6 else C.variant_n8_input)(nc, -1)
        _reserve_ref[order, nc] = (u, dx, dt, DgRef(u, dt, dx, 3, order, nc, order))
    return _reserve_ref[order, nc]


@pytest.mark.parametrize("order,nc,variant", RESERVE_CASES)
def test_stage_a_reserve_clamps_the_persistent_grid(exa, orc, order, nc, variant):
    """exa_dg_plan_set_stage_a_reserve keeps the persistent grids that many workgroups below what the chip holds, at least one: with a
    reserve beyond any chip ONE workgroup walks all cells.  The arithmetic of a cell does not depend on which workgroup takes it, so u* and
    the traces are those of the unreserved launch bit for bit, and both are within the oracle's bound."""
    u, dx, dt, r = _reserve_case(order, nc)
    s = exa.AderDgSolver(3, order, nc, dx=dx, stage_a=variant)
    out = []
    for reserve in (0, 10 ** 6):
        s.set_reserve_cus(reserve)
        s.trace.zero_()
        s.upload(u)
        s.predictor_volume(dt)
        out.append((s.download().copy(), s.trace.cpu().numpy().copy()))
        r.check_ustar(out[-1][0], what="u* (reserve %d)" % reserve)
        r.check_traces(out[-1][1], what="traces (reserve %d)" % reserve)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_stage_a_variant_rejects_unknown(exa):
    from exahype_amd._lib import ExaHypeHipError
    s = exa.AderDgSolver(3, 4, (1, 1, 1))
    with pytest.raises(ExaHypeHipError):
        exa._lib.check(s.lib.exa_dg_plan_set_stage_a(s._plan, 7))

"""The step as ONE kernel (include/exahype_hip.h exa_dg_corrector_predictor; 3-D, N = 6): Riemann solve + corrector of the previous step in
front of the predictor, against the two-kernel step and against the CPU oracle at steps around the CFL-0.9 step (tests/util.py assert_dg_parity: DG_TOL of the
per-variable increment and relative 1e-10, with a case that sees the last Picard iteration; ADER-DG is "parity unpinned" against the reference,
which holds no ADER-DG -- see tests/test_gpu_parity.py)."""
import numpy as np
import pytest

from tests import dg_cases as C
from tests.dg_cases import DgRef
from tests.util import rel_err

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


@pytest.mark.parametrize("nc,n_it", C.ONE_KERNEL_CASES)
def test_one_kernel_steps_vs_oracle_and_two_kernel_steps(exa, orc, nc, n_it):
    u, dx, dts = C.one_kernel_input(nc)                                # a different dt every step: the corrector uses the previous one
    r = DgRef(u, dts[0], dx, 3, N, nc, C.n_it_of(N, n_it))
    one = exa.AderDgSolver(3, N, nc, n_picard=n_it, dx=dx, one_kernel_step=True)
    two = exa.AderDgSolver(3, N, nc, n_picard=n_it, dx=dx, one_kernel_step=False)
    assert one._one_kernel and not two._one_kernel
    one.upload(u)
    two.upload(u)
    steps = len(dts) if np.prod(nc) < 100 else 3
    for k in range(steps):
        one.step(dts[k])
        two.step(dts[k])
        assert one._pending_dt == dts[k]
        if k == 1:                                                     # reading u in the middle of a run applies the pending corrector
            r.check_steps(one.download(), 2, dts=dts)
            assert one._pending_dt is None
    a, b = one.download(), two.download()
    r.check_steps(a, steps, dts=dts)
    assert rel_err(a, b) < 1e-12
    assert rel_err(one.trace.cpu().numpy(), two.trace.cpu().numpy()) < 1e-12


def test_one_kernel_step_is_refused_where_it_is_not_built(exa):
    with pytest.raises(ValueError):
        exa.AderDgSolver(3, 4, (2, 2, 2), one_kernel_step=True)
    with pytest.raises(ValueError):
        exa.AderDgSolver(3, N, (2, 2, 2), stage_a="lds", one_kernel_step=True)
    s = exa.AderDgSolver(3, N, (2, 2, 2))                              # off unless asked for
    assert not s._one_kernel

"""SubcellLimiter(fv_mode=FV_MUSCL_HANCOCK, stream_planes=FV_STREAM_IF_NEEDED) at the 3-D orders whose patches only the plane-streaming
kernel serves -- N = 6, 7, 8, patches of 11, 13 and 15 volumes per axis with halo 2 -- and the limiter's glue kernels at those orders
(limiter_project_halo2_kernel, limiter_reconstruct_halo_kernel<.., 2>), which tests/limiter_muscl_cases.py never launched: its orders stop at 5.

  * the halo-2 projection on the grids (2, 3, 4) and (1, 3, 2), element by element over the whole patch against tests/limiter_muscl_ref.py
    reference_patch2 within projection_bound2 (the checker of tests/test_limiter_muscl.py), and with the wall / outflow / state faces at N = 6;
  * the reconstruction from patches with halo 2 bit-equal to the one from patches with halo 1 at N = 6 and 8;
  * one limited step at N = 6 on (2, 3, 4) and at N = 8 on (1, 2, 2) against the restatement around the solver's own DG candidate: relative
    error below 1e-10 (the figure of tests/test_limiter_muscl.py), untroubled cells bit-equal to the plain step;
  * the default stream_planes still refuses these orders and names plane streaming.
"""
import numpy as np
import pytest

from tests import limiter_cases as K
from tests import limiter_muscl_cases as KM
from tests import limiter_muscl_ref as M2
from tests.test_limiter_muscl import _bits, _cfl_dt, _check_patches2, _check_step, _mask, _operators, _project2, _ptr, _solver
from tests.util import euler_dg_state

pytestmark = pytest.mark.gpu
GRIDS = [(2, 3, 4), (1, 3, 2)]


@pytest.mark.parametrize("N", [6, 7, 8])
def test_projection_halo2_whole_patch_at_the_streamed_orders(N):
    worst = 0.0
    for g, nc in enumerate(GRIDS):
        u = K.state(3, N, nc, 5, g)
        s = _solver(3, N, nc)
        P, _ = _operators(s)
        cells = K.cell_list(int(np.prod(nc)), seed=100 * N + g)
        worst = max(worst, _check_patches2(_project2(s, u, cells), u, cells, P))
    print("projection halo 2, 3-D N %d: err / bound %.3f" % (N, worst))
    assert worst > 0.0


def test_projection_halo2_faces_with_conditions_at_N6():
    N, nc = 6, KM.BC_GRID[3]
    cond = KM.conditions(3, "wall_outflow_state")
    u = K.state(3, N, nc, 5, 7)
    s = _solver(3, N, nc)
    P, _ = _operators(s)
    cells = K.cell_list(int(np.prod(nc)), seed=300 * N)
    worst = _check_patches2(_project2(s, u, cells, cond), u, cells, P, cond)
    print("projection halo 2 with conditions, 3-D N %d: err / bound %.3f" % (N, worst))
    assert worst > 0.0


@pytest.mark.parametrize("N", [6, 8])
def test_reconstruction_halo2_equals_halo1_at_the_streamed_orders(N):
    import torch
    from exahype_amd import solvers as exa
    dim, nc = 3, (2, 3, 4)
    ncell = int(np.prod(nc))
    s = _solver(dim, N, nc)
    u0 = K.state(dim, N, nc, 5, 0)
    cells = K.cell_list(ncell, seed=7 * N + dim, subset=True)
    p1 = K.random_patches(dim, N, 5, len(cells), seed=11 * N + dim)
    p2 = KM.repad(p1, dim)
    cd = torch.as_tensor(cells).cuda()
    res = []
    for patches, halo in ((p1, 1), (p2, 2)):
        s.upload(u0)
        pd = torch.as_tensor(np.ascontiguousarray(patches)).cuda()
        exa.check(s.lib.exa_lim_reconstruct_patches_halo(s._plan, _ptr(pd), _ptr(cd), len(cells), _ptr(s.u), halo, None))
        torch.cuda.synchronize()
        res.append(s.download())
    assert np.all(np.abs(res[0]) < 1e20)                           # (no halo entry leaked)
    assert not np.array_equal(res[0], np.asarray(u0).reshape(res[0].shape))
    assert np.array_equal(_bits(res[1]), _bits(res[0]))


@pytest.mark.parametrize("N,nc", [(6, (2, 3, 4)), (8, (1, 2, 2))])
def test_one_limited_step_at_the_streamed_orders(N, nc):
    from exahype_amd import solvers as exa
    dim, dx = 3, 0.25
    u0 = euler_dg_state(nc + (N,) * dim, seed=40 + N)
    dt = _cfl_dt(u0, dim, N, dx)
    mask = _mask(nc, N)
    kw = dict(dx=[dx] * dim)
    plain = exa.AderDgSolver(dim, N, nc, **kw)
    plain.upload(u0)
    plain.step(dt)
    cand = plain.download().reshape(u0.shape)
    s = exa.AderDgSolver(dim, N, nc, **kw)
    lim = exa.SubcellLimiter(s, capacity=int(np.prod(nc)), fv_mode=exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_IF_NEEDED)
    assert lim._fv.streamed and lim.fv_halo == 2
    s.upload(u0)
    count = lim.step(dt, mask)
    assert int(count) == int(mask.sum())
    got = lim.download().reshape(u0.shape)
    ops = dict(s.operators(), N=N)
    want = M2.replace_troubled2(u0, cand, mask, dt, [dx] * dim, ops, M2.fv_update2(dim))
    _check_step(cand, got, want, mask)


def test_default_still_names_plane_streaming():
    from exahype_amd import solvers as exa
    for N in (6, 8):
        with pytest.raises(ValueError, match="plane streaming"):
            exa.SubcellLimiter(exa.AderDgSolver(3, N, (2, 1, 1)), capacity=1, fv_mode=exa.FV_MUSCL_HANCOCK)
    # the streamed limiter at an order with a resident plan keeps the resident kernel
    lim = exa.SubcellLimiter(exa.AderDgSolver(3, 4, (2, 1, 1)), capacity=1, fv_mode=exa.FV_MUSCL_HANCOCK, stream_planes=exa.FV_STREAM_IF_NEEDED)
    assert not lim._fv.streamed
    with pytest.raises(ValueError, match="fv_mode=FV_MUSCL_HANCOCK"):
        exa.SubcellLimiter(exa.AderDgSolver(3, 4, (2, 1, 1)), capacity=1, stream_planes=exa.FV_STREAM_IF_NEEDED)

"""The corrected FV Rusanov kernels (exahype_amd/csrc/fv_rusanov.hip, mode FV_RUSANOV) against the long-double reference
(oracle/fv_reference.py), for every row of tests/fv_cases.py -- one per branch of `fv_dispatch` and entry point -- times every state family.

The measure.  Every evolved variable of every interior volume lies within 2^-53 E of the reference, E being the operation count of the formula
applied term by term (oracle/fv_reference.py's docstring: each fp64 operation adds one unit of 2^-53 of its result to the bound its operands
carry; flat form E <= C M with C_ieee = 44 over the magnitude M).  The device bound E_dev is that same count with the documented accuracy of the
device primitives in place of the IEEE ones: `fast_rcp` <= 11 ulp = 22 units where 1 / rho enters (flux coefficient, kinetic energy in p, u_n, the
radicand of c), `fast_sqrt` <= 1 ulp = 2 units on c (exa_pde.hpp; scripts/rcp_accuracy.hip); contraction into fma, the mass flux kept as m_n and
|u_n| + c for the maximum remove roundings and add none.  E_dev applies where the kernel uses those primitives -- the plane-streaming kernel with
cached scalars (`Euler::fv_aux`); every other branch, and the advection, evaluates IEEE division and square root and is held to E_ieee.  Neither
is taken from what the kernels give; tests/test_fv_reference.py shows on the CPU that the C oracle stays inside E_ieee on these very inputs and that
every mutant of the reference (wrong spacing, no max, 1/4, wrong axis, wrong side, no pressure, a reciprocal 2^-40 off, the next patch's halo)
leaves E_dev 100-fold.  Halo and auxiliary values are bit-equal to the input, in the layout the entry defines.

Grid step: three steps, so the array swap is exercised; step k is compared with ONE reference step (the global-array form) from the device's own
state after step k - 1, so the bound stays a one-step bound.  The fused CFL scalar lies within the eigenvalue's own rounding bound (the same count:
2^-53 e_lambda, e_lambda from max_eigenvalue(..., prim)) of the long-double maximum over the new states and the boundary states.

EXA_FV_ERR_LOG=<file>: one JSON line per comparison (tests/util.py log_fv_measurement); the figures of the MI355X run are
profiles/fv_kernels_hp.txt.
"""
import numpy as np
import pytest

from oracle import fv_reference as R
from tests import fv_cases as K
from tests.util import euler_ref2d_patches, log_fv_measurement

pytestmark = pytest.mark.gpu
LD = np.longdouble
PATCH_ROWS = [r for r in K.ROWS if not r[8].startswith("grid")]
GRID_ROWS = [r for r in K.ROWS if r[8].startswith("grid")]


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from exahype_amd import solvers
    return solvers


def _pde(exa, pde):
    return exa.PDE_EULER if pde == R.PDE_EULER else exa.PDE_ADVECTION


def _run_entry(exa, row, Q, dt, h):
    """the row's entry on the device -> (result as numpy, layout, masked patches or None)"""
    import torch
    _, dim, P, H, n_real, n_aux, n, pde, entry = row
    k = exa.FVRusanovKernel(dim, P, H, n_real, n_aux, n, _pde(exa, pde), exa.FV_RUSANOV)
    qd = torch.as_tensor(Q).cuda()
    if entry == "inplace":
        k.time_step(qd, dt, h)
        torch.cuda.synchronize()
        return qd.cpu().numpy(), "halo", None
    if entry == "slot":
        slot = K.slot_of(n)
        k.time_step(qd, dt, h, slot=torch.as_tensor(slot).cuda())
        torch.cuda.synchronize()
        return qd.cpu().numpy(), "halo", slot < 0
    assert entry == "oop"
    out = k.time_step_oop(qd, dt, h)
    torch.cuda.synchronize()
    assert np.array_equal(qd.cpu().numpy(), Q), "time_step_oop wrote its input"
    return out.cpu().numpy(), "dense", None


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("row", PATCH_ROWS, ids=K.row_id)
def test_patch_update_within_bound(exa, row, family):
    _, dim, P, H, n_real, n_aux, n, pde, entry = row
    Q = K.row_state(row, family)
    dt, h = K.cfl_step(Q, dim, pde)
    got, layout, masked = _run_entry(exa, row, Q, dt, h)
    K.assert_within_bound(got, Q, dt, h, dim, P, H, n_real, n_aux, pde, K.primitives(row), "%s %s" % (K.row_id(row), family),
                          layout=layout, masked=masked, row=K.row_id(row), family=family, entry=entry)


def _lam_reference(U, bnd, dim, pde, prim):
    """long-double maximum of the eigenvalue over the states (and the boundary states) and the rounding bound that holds for an fp64 maximum:
    the device's maximum is attained at a state whose fp64 eigenvalue can reach the largest one -- lam_j + 2^-53 e_j >= max - 2^-53 e_argmax -- so
    the bound is the largest e among THOSE states, not among all (a volume with a small eigenvalue and a strong cancellation in its pressure
    does not widen it)."""
    states = U.reshape(-1, U.shape[-1])
    if bnd is not None:
        states = np.concatenate([states, np.stack(list(bnd.values()))])
    lam, e = [np.concatenate(x) for x in zip(*[R.max_eigenvalue(states, d, pde, prim) for d in range(dim)])]
    top = int(np.argmax(lam))
    can_win = lam + R.U53 * e >= lam[top] - R.U53 * e[top]
    return lam[top], np.max(e[can_win])


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("row", GRID_ROWS, ids=K.row_id)
def test_grid_step_within_bound(exa, row, family):
    _, dim, P, H, n_real, n_aux, n, pde, entry = row
    grid, dirichlet = K.grid_of(row)
    V = n_real + n_aux
    U = K.row_state(row, family).reshape(grid + (P,) * dim + (V,))
    bnd = K.boundary_states(row, family) if dirichlet else None
    dt, _ = K.cfl_step(U, dim, pde, extra=None if bnd is None else np.stack(list(bnd.values())))
    g = exa.FVPatchGrid(dim, grid, P, H, n_real, n_aux, _pde(exa, pde), exa.FV_RUSANOV, length=K.H_VOLUME * grid[0] * P, boundary=bnd, fused=True)
    assert abs(g.h - K.H_VOLUME) < 1e-15
    g.set_interior(U)
    prim = K.primitives(row)
    for step in range(3):
        before = g.interior()
        g.step(dt)
        after = g.interior()
        ref = R.grid_update(before, dt, g.h, dim, n_real, pde, boundary=bnd, prim=prim)
        worst = R.ratio(after, ref)
        lam_dev = g.max_eigenvalue()
        want, eb = _lam_reference(after, bnd, dim, pde, prim)
        if eb > 0:
            lam_ratio = float(abs(LD(lam_dev) - want) / (R.U53 * eb))
        else:                                                   # a constant eigenvalue (advection) has no rounding at all: the scalar is that constant
            assert lam_dev == float(want), (lam_dev, float(want))
            lam_ratio = 0.0
        what = "%s %s step %d" % (K.row_id(row), family, step)
        print("%s: err / bound %.3f, CFL scalar %.3f of its bound (%.2f x 2^-53 relative)" % (what, worst, lam_ratio, float(eb / want)))
        log_fv_measurement(what=what, row=K.row_id(row), family=family, entry=entry, ratio=worst, cfl_ratio=lam_ratio,
                           primitives="device" if prim is R.DEVICE else "ieee")
        assert worst <= 1.0, (what, worst)
        assert np.array_equal(after[..., n_real:], before[..., n_real:]), what + ": auxiliary variables changed"
        assert lam_ratio <= 1.0, (what, lam_dev, float(want), lam_ratio)


def test_eigenvalue_vs_device_pde_eval(exa):
    """the long-double eigenvalue agrees with the device's point-wise evaluation within 4 * 2^-53 relative.  It is here and not in the CPU module
    because exa.pde_eval has no host path: it launches pde_eval_kernel (the C oracle's orc_pde_maxeig is compared in tests/test_fv_reference.py)."""
    for family in K.FAMILIES:
        q = K.state(family, 1, 2, 20, 0, 5, 31).reshape(-1, 5)
        for d in range(3):
            want = R.max_eigenvalue(q, d, R.PDE_EULER)
            got = exa.pde_eval(exa.PDE_EULER, d, q)[1]
            rel = float(np.max(np.abs(got.astype(LD) - want) / want) / R.U53)
            print("pde_eval %s d%d: %.3f x 2^-53" % (family, d, rel))
            assert rel <= 4.0, (family, d, rel)


def test_faithful_persistent_kernel_on_distinct_patches(exa):
    """the headline FV row's bit-exact claim on patches that differ: 16 * 2048 + 37 patches (the persistent form; ragged last block, odd tail)"""
    import oracle
    import torch
    n = K.PERSISTENT_PATCHES
    Q = euler_ref2d_patches(n, 6, 10, seed=41)
    want = oracle.fv_faithful(Q, 0.2, 2, 4, 1, 5, 5, n, oracle.PDE_EULER_REF2D)
    k = exa.FVRusanovKernel(2, 4, 1, 5, 5, n, exa.PDE_EULER_REF2D, exa.FV_FAITHFUL)
    qd = torch.as_tensor(Q).cuda()
    k.time_step(qd, 0.2)
    torch.cuda.synchronize()
    assert np.array_equal(qd.cpu().numpy(), want)


@pytest.mark.parametrize("row", [next(r for r in PATCH_ROWS if r[8] == "inplace" and r[0] == b) for b in ("ref", "slab-cache", "cpt4")], ids=K.row_id)
def test_negative_control_h_off_by_2m30(exa, row):
    """the measure sees a 1e-9 error on the real kernels: the row's kernel run with h (1 + 2^-30) leaves the bound"""
    _, dim, P, H, n_real, n_aux, n, pde, entry = row
    Q = K.row_state(row, "supersonic")
    dt, h = K.cfl_step(Q, dim, pde)
    got, _, _ = _run_entry(exa, row, Q, dt, h * (1 + 2.0 ** -30))
    ref = R.update(Q, dt, h, dim, P, H, n_real, n_aux, pde, prim=K.primitives(row))
    worst = R.ratio(got, ref, R.interior(dim, P, H))
    print("negative control %s: err / bound %.3g" % (K.row_id(row), worst))
    log_fv_measurement(what="negative control " + K.row_id(row), ratio=worst)
    assert worst > 1.0, worst

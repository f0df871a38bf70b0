"""The FV Rusanov kernels as they are instantiated for GENERATED term sets (the side library of a SympyPDE: `fv_dispatch<DIM, exa::UserPDE, ..>` of
exahype_amd/csrc/fv_rusanov.hip) against the long-double reference (oracle/fv_reference.py: user_update / user_grid_update), for every row of
tests/fv_user_cases.py -- one per dispatch branch and entry point a generated term set reaches -- times every state family.  The sibling of
tests/test_fv_kernels_hp.py.

The measure.  Every evolved variable of every interior volume lies within 2^-53 E of the reference; E is the operation count of the update applied
term by term, with the term set's own expressions walked node by node (oracle/fv_reference.py's docstring: the count of the source, of the ncp at
the face's mean state and mid point, of the volume centres and of the shifted coordinates).  The FV unit of a side library is compiled without
contraction and its flux_rt / flux_xt, maxeig, source and ncp members use IEEE division and square root, so the bound is E_ieee throughout.
Nothing in it is taken from what the kernels give: tests/test_fv_user_reference.py shows on the CPU that fp64 evaluations of the same statement, with
the terms in the forms the generator may emit, stay inside it on these very inputs, and that every mutant (a face mid point at x_c +- h, an ncp at
q_c, the next patch's centre, a coordinate without the halo offset, ...) leaves it 100-fold.  Halo values, auxiliary variables and masked patches
are bit-equal to the input; time_step_oop leaves its input untouched.

Grid step: three steps; step k is compared with ONE reference step from the device's own state after step k - 1 at the grid's running time.  The
fused CFL scalar lies within the eigenvalue's own rounding bound of the long-double maximum over the new states at (x_c, t + dt) and the boundary
states (which FVPatchGrid evaluates at the origin and t = 0); after invalidate() the scan pass agrees within the same bound; g.time advances by
exactly fl(t + dt).

Negative controls: the kernels run with t, the centres or h off by 2^-30 relative leave the bound.

EXA_FV_ERR_LOG=<file>: one JSON line per comparison (tests/util.py log_fv_measurement); the figures of the MI355X run are
profiles/fv_user_kernels_hp.txt.
"""
import numpy as np
import pytest

from oracle import fv_reference as R
from tests import fv_user_cases as U
from tests.util import log_fv_measurement

pytestmark = pytest.mark.gpu
LD = np.longdouble
PATCH_ROWS = [r for r in U.ROWS if not U.is_grid(r)]
GRID_ROWS = [r for r in U.ROWS if U.is_grid(r)]
# the persistent row (32 805 patches) runs once, in the benign family
PATCH_CASES = [(r, f) for r in PATCH_ROWS for f in U.FAMILIES if r[0] != "ref-persistent" or f == "benign"]
OFF = 1 + 2.0 ** -30


@pytest.fixture(scope="module")
def exa():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from exahype_amd import solvers
    return solvers


def _run_entry(exa, row, Q, dt, h, centres, t):
    """the row's entry on the device -> (result as numpy, layout, masked patches or None)"""
    import torch
    _, name, dim, P, H, n_aux, n, entry = row
    k = exa.FVRusanovKernel(dim, P, H, U.n_real(row), n_aux, n, U.term_set(name).register(), exa.FV_RUSANOV)
    qd = torch.as_tensor(Q).cuda()
    cen = None if centres is None else torch.as_tensor(np.ascontiguousarray(centres)).cuda()
    if entry in ("inplace", "inplace-origin"):
        k.time_step(qd, dt, h, t=t, centres=cen)
        torch.cuda.synchronize()
        return qd.cpu().numpy(), "halo", None
    if entry == "slot":
        slot = U.slot_of(n)
        k.time_step(qd, dt, h, slot=torch.as_tensor(slot).cuda(), t=t, centres=cen)
        torch.cuda.synchronize()
        return qd.cpu().numpy(), "halo", slot < 0
    assert entry == "oop"
    out = k.time_step_oop(qd, dt, h, t=t, centres=cen)
    torch.cuda.synchronize()
    assert np.array_equal(qd.cpu().numpy(), Q), "time_step_oop wrote its input"
    return out.cpu().numpy(), "dense", None


@pytest.mark.parametrize("row,family", PATCH_CASES, ids=lambda x: U.row_id(x) if isinstance(x, tuple) else x)
def test_patch_update_within_bound(exa, row, family):
    Q = U.row_state(row, family)
    centres, t = U.coordinates(row)
    dt, h = U.cfl_step(row, Q, centres, t)
    got, layout, masked = _run_entry(exa, row, Q, dt, h, centres, t)
    U.assert_within_bound(got, Q, dt, h, row, centres, t, "%s %s" % (U.row_id(row), family), layout=layout, masked=masked,
                          row_id=U.row_id(row), branch=row[0], family=family, entry=row[7])


def _lam_reference(tm, states, X, t, t_bound, bnd, dim):
    """long-double maximum of the eigenvalue over the states at (X, t) and the boundary states (origin, t = 0), and the rounding bound that
    holds for an fp64 maximum: the largest bound among the states whose fp64 eigenvalue can reach the largest one"""
    lam, e = [], []
    for d in range(dim):
        v, b = R.user_max_eigenvalue(tm, states, d, X, t, t_bound, prim=R.IEEE)
        lam.append(v.ravel())
        e.append(b.ravel())
        if bnd is not None:
            v, b = R.user_max_eigenvalue(tm, np.stack(list(bnd.values())), d, prim=R.IEEE)
            lam.append(v.ravel())
            e.append(b.ravel())
    lam, e = np.concatenate(lam), np.concatenate(e)
    top = int(np.argmax(lam))
    can_win = lam + R.U53 * e >= lam[top] - R.U53 * e[top]
    return lam[top], np.max(e[can_win])


def _grid(exa, row, family, t_factor=1.0):
    _, name, dim, P, H, n_aux, n, entry = row
    grid, dirichlet = U.grid_of(row)
    m = U.n_real(row)
    Uh = U.row_state(row, family).reshape(grid + (P,) * dim + (m + n_aux,))
    bnd = U.boundary_states(row, family) if dirichlet else None
    centres, t0 = U.coordinates(row)
    xt = centres is not None
    g = exa.FVPatchGrid(dim, grid, P, H, m, n_aux, U.term_set(name).register(), exa.FV_RUSANOV, length=U.H_VOLUME * grid[0] * P, boundary=bnd,
                        origin=U.ORIGIN[:dim] if xt else None, time=t0 * t_factor, fused=True)
    assert abs(g.h - U.H_VOLUME) < 1e-15
    if xt:                                                      # the reference takes the fp64 centres the kernel gets
        assert np.allclose(g.centres.cpu().numpy(), centres, rtol=0, atol=1e-15)
        centres = g.centres.cpu().numpy()
    g.set_interior(Uh)
    dt, _ = U.cfl_step(row, Uh.reshape((n,) + Uh.shape[dim:]), centres, t0, None if bnd is None else np.stack(list(bnd.values())))
    return g, centres, t0, dt, bnd


@pytest.mark.parametrize("family", U.FAMILIES)
@pytest.mark.parametrize("row", GRID_ROWS, ids=U.row_id)
def test_grid_step_within_bound(exa, row, family):
    _, name, dim, P, H, n_aux, n, entry = row
    m, tm = U.n_real(row), U.terms(name)
    g, centres, t0, dt, bnd = _grid(exa, row, family)
    assert g.time == t0
    X = R.volume_centres(centres, n, dim, P, g.h)
    for step in range(3):
        before, t = g.interior(), g.time
        g.step(dt)
        after = g.interior()
        assert g.time == t + dt                                 # advances exactly: fl(t + dt), the time the kernel's scan evaluated at
        ref = R.user_grid_update(before, dt, g.h, dim, tm, centres, t, boundary=bnd)
        worst = R.ratio(after, ref)
        t_new = LD(t) + LD(dt)
        want, eb = _lam_reference(tm, after.reshape((n,) + after.shape[dim:]), X, t_new, abs(t_new) if tm.uses_t else 0.0, bnd, dim)
        assert eb > 0
        lam_ratio = float(abs(LD(g.max_eigenvalue()) - want) / (R.U53 * eb))
        g.invalidate()
        scan_ratio = float(abs(LD(g.max_eigenvalue()) - want) / (R.U53 * eb))
        what = "%s %s step %d" % (U.row_id(row), family, step)
        print("%s: err / bound %.3f, CFL scalar %.3f (scan pass %.3f) of its bound (%.2f x 2^-53 relative)" % (what, worst, lam_ratio, scan_ratio, float(eb / want)))
        log_fv_measurement(what=what, row_id=U.row_id(row), branch=row[0], family=family, entry=entry, ratio=worst, cfl_ratio=lam_ratio, scan_ratio=scan_ratio,
                           primitives="ieee")
        assert worst <= 1.0, (what, worst)
        assert np.array_equal(after[..., m:], before[..., m:]), what + ": auxiliary variables changed"
        assert lam_ratio <= 1.0 and scan_ratio <= 1.0, (what, lam_ratio, scan_ratio)


def _first(branch, name, entry):
    return next(r for r in U.ROWS if r[0] == branch and r[1] == name and r[7].startswith(entry))


NEGATIVE = [("t", _first("cpt4", U.CR, "inplace")), ("t", _first("nt1024-staged", U.CR, "inplace")), ("centres", _first("staged", U.CR, "inplace")),
            ("h", _first("slab", U.EG, "inplace"))]


@pytest.mark.parametrize("what,row", NEGATIVE, ids=lambda x: U.row_id(x) if isinstance(x, tuple) else x)
def test_negative_control_off_by_2m30(exa, what, row):
    """the measure sees a 1e-9 error on the real kernels: the row's kernel run with t, the centres or h times (1 + 2^-30) leaves the bound"""
    _, name, dim, P, H, n_aux, n, entry = row
    Q = U.row_state(row, "benign")
    centres, t = U.coordinates(row)
    dt, h = U.cfl_step(row, Q, centres, t)
    got, _, _ = _run_entry(exa, row, Q, dt, h * (OFF if what == "h" else 1), centres * OFF if what == "centres" else centres, t * (OFF if what == "t" else 1))
    ref = R.user_update(Q, dt, h, dim, P, H, U.terms(name), n_aux, centres, t)
    worst = R.ratio(got, ref, R.interior(dim, P, H))
    print("negative control %s of %s: err / bound %.3g" % (what, U.row_id(row), worst))
    log_fv_measurement(what="negative control %s %s" % (what, U.row_id(row)), ratio=worst)
    assert worst > 1.0, worst


def test_negative_control_grid_time_off_by_2m30(exa):
    row = _first("staged", U.CR, "grid:periodic")
    _, name, dim, P, H, n_aux, n, entry = row
    g, centres, t0, dt, bnd = _grid(exa, row, "benign", t_factor=OFF)
    before = g.interior()
    g.step(dt)
    ref = R.user_grid_update(before, dt, g.h, dim, U.terms(name), centres, t0, boundary=bnd)
    worst = R.ratio(g.interior(), ref)
    print("negative control t of %s: err / bound %.3g" % (U.row_id(row), worst))
    log_fv_measurement(what="negative control t " + U.row_id(row), ratio=worst)
    assert worst > 1.0, worst

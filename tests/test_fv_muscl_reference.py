"""CPU checks of the measure the MUSCL-Hancock kernels are held to (tests/fv_muscl_ref.py), of the mode's argument checks and of the generator's
keyword -- no GPU.

  * the plain fp64 numpy form of the five statements (fv_muscl_ref.fp64_update: rolls over the window, written apart from the long-double
    restatement) stays inside the bound 2^-53 E on every row x family of tests/fv_muscl_cases.py at CFL 0.5: the bound is satisfiable;
  * every mutant of the restatement leaves the bound at least 100-fold on at least one row: the bound is not slack (exemptions:
    fv_muscl_ref.mutant_exemption gives the reason);
  * the fp64 form reproduces the recorded runs (tests/golden/fv_muscl_runs.json): the orders 1.84 (advection of a sine) and 1.81 (Euler density
    wave) between 64^2 and 128^2 volumes and the Sod L1(rho) of 3.97e-3 at 256 volumes, each within 5 %;
  * include/exahype_hip.h declares EXA_FV_MUSCL_HANCOCK; exa_fv_plan_create takes mode 2 (without a GPU: EXA_ERR_NO_DEVICE, no longer
    "unknown FV mode 2"), refuses halo_size 1, EULER_REF2D, a term set generated without the keyword and a shape whose LDS plan does not fit;
  * SympyPDE(muscl_hancock=True) refuses a source, an ncp and (x, t) terms; a term set without the keyword hashes what it hashed before.
"""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from oracle import fv_reference as R
from tests import fv_muscl_cases as K
from tests import fv_muscl_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fv_muscl_runs.json")))
EXA_OK, EXA_ERR_INVALID, EXA_ERR_NO_DEVICE = 0, -1, -3


@pytest.mark.parametrize("row", K.ROWS, ids=K.row_id)
def test_fp64_form_is_inside_the_bound(row):
    dim, P, H, n_real, n_aux, n, pde, _ = row
    for family in K.families(row):
        Q = K.row_state(row, family)
        dt, h = K.cfl_step(Q, dim, pde)
        ref = M.update(Q, dt, h, dim, P, H, n_real, n_aux, pde)
        got = M.fp64_update(Q, dt, h, dim, P, H, n_real, pde)
        sel = M.interior(dim, P, H)
        worst = M.ratio(got, ref, sel)
        print("%s %s: fp64 form err / bound %.3f, E / M at most %.1f" % (K.row_id(row), family, worst, float(np.max(ref.E / ref.M))))
        assert 0.0 < worst <= 1.0, (K.row_id(row), family, worst)
        # what the restatement leaves alone
        keep = np.ones(Q.shape[1:], dtype=bool)
        keep[sel[1:] + (slice(0, n_real),)] = False
        assert np.array_equal(ref.new[:, keep].astype(np.float64), Q[:, keep])


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    worst, reasons = 0.0, set()
    for row in K.CPU_MUTANT_ROWS:
        dim, P, H, n_real, n_aux, n, pde, _ = row
        why = M.mutant_exemption(mutant, dim, pde, n_aux)
        if why is not None:
            reasons.add(why)
            continue
        for family in K.families(row)[:2]:
            Q = K.row_state(row, family)
            dt, h = K.cfl_step(Q, dim, pde)
            ref = M.update(Q, dt, h, dim, P, H, n_real, n_aux, pde)
            mut = M.update(Q, dt, h, dim, P, H, n_real, n_aux, pde, mutant=mutant, track=False)
            worst = max(worst, M.ratio(mut.new.astype(np.float64), ref, M.interior(dim, P, H)))
    print("mutant %s: err / bound %.3g%s" % (mutant, worst, "".join("\n  exempt: " + r for r in reasons)))
    if reasons and worst == 0.0:
        # exempt on every row: the reason must hold -- the mutant changes no evolved value of the restatement itself
        row = K.ROWS[2]
        dim, P, H, n_real, n_aux, n, pde, _ = row
        Q = K.row_state(row, "benign")
        dt, h = K.cfl_step(Q, dim, pde)
        a = M.update(Q, dt, h, dim, P, H, n_real, n_aux, pde, track=False).new
        b = M.update(Q, dt, h, dim, P, H, n_real, n_aux, pde, mutant=mutant, track=False).new
        assert n_aux > 0 and np.array_equal(a, b), "the exemption's reason does not hold"
        return
    assert worst >= 100.0, (mutant, worst)


def test_minmod_decides_by_the_signs():
    """products of tiny differences underflow: 1e-200 and 2e-200 have the same sign, their product is 0; a NaN difference gives slope 0"""
    V = lambda x: R._V(np.array(x, dtype=M.LD), np.zeros(len(x), dtype=M.LD))     # noqa: E731
    s = M._minmod(V([1e-200, -1e-200, 1e-200, np.nan, 0.0, 3.0]), V([2e-200, -3e-200, -1e-200, 1.0, 1.0, 2.0]))
    assert np.array_equal(s.v.astype(np.float64), np.array([1e-200, -1e-200, 0.0, 0.0, 0.0, 2.0]))
    # the fp64 form decides the same way.  Advection (a = 1 along axis 0, Rusanov = upwind), q_i = i^2 1e-200, r = 1/2: the slopes of volumes 1 and 2
    # are 1e-200 and 3e-200, w_i^+ = q_i + s_i/2 - (r/2) s_i = q_i + s_i/4, so q_2 <- 4 - (4.75 - 1.25)/2 = 2.25 (e-200); with slopes that
    # underflowed to zero it would be the first-order 4 - 3/2 = 2.5
    q = np.zeros((1, 5, 5, 1))
    q[0, :, :, 0] = (np.arange(5.0) ** 2)[:, None] * 1e-200
    got = M.fp64_block(q, 0.5, 1.0, 2, 1, R.PDE_ADVECTION)
    assert got.shape == (1, 1, 1, 1) and abs(got[0, 0, 0, 0] / 2.25e-200 - 1) < 1e-12


def test_outside_stencil_matches_the_statement():
    """the entries no interior update reads: (+-2, +-1), the 3-D corners and layers beyond the second -- and nothing else"""
    m = M.outside_stencil(2, 3, 3)
    assert m[0].all() and m[:, 0].all() and m[-1].all()            # the third layer
    assert not m[1, 3] and not m[2, 3] and not m[2, 2]             # second layer beside the interior, first layer, the edge entry (1, 1)
    assert m[1, 2] and m[2, 1] and m[1, 1]                         # (2, 1), (1, 2), (2, 2)
    m3 = M.outside_stencil(3, 2, 2)
    assert m3[1, 1, 1] and not m3[1, 1, 2] and m3[0, 1, 2] and not m3[0, 2, 2] and not m3[2, 2, 2]
    # the restatement itself never reads them: NaN there changes nothing
    row = (3, 2, 2, 5, 0, 2, K.E, "")
    Q = K.row_state(row, "benign")
    dt, h = K.cfl_step(Q, 3, K.E)
    Qn = Q.copy()
    Qn[:, m3] = np.nan
    a = M.fp64_update(Q, dt, h, 3, 2, 2, 5, K.E)[M.interior(3, 2, 2)]
    b = M.fp64_update(Qn, dt, h, 3, 2, 2, 5, K.E)[M.interior(3, 2, 2)]
    assert np.array_equal(a, b)
    # ... and every entry inside the stencil is read: a large change of its density, up or down, changes an interior value (one of the two signs
    # turns a minmod that was zero into a slope, or a slope into zero)
    for idx in np.argwhere(~m3):
        changed = False
        for delta in (0.4, -0.4):
            Qn = Q.copy()
            Qn[(0,) + tuple(idx) + (0,)] += delta
            changed = changed or not np.array_equal(M.fp64_update(Qn, dt, h, 3, 2, 2, 5, K.E)[M.interior(3, 2, 2)], a)
        assert changed, idx


def test_recorded_runs():
    """the issue's table: orders 1.84 / 1.81 and the Sod error 3.97e-3, within 5 %, and the golden file is what the fp64 form gives"""
    g = GOLDEN
    assert abs(g["advection"]["order_muscl"] / 1.84 - 1) < 0.05 and abs(g["density_wave"]["order_muscl"] / 1.81 - 1) < 0.05
    assert abs(g["sod"]["muscl"]["l1"] / 3.97e-3 - 1) < 0.05
    assert g["sod"]["muscl"]["min_rho"] >= 0.125 - 1e-12 and g["sod"]["muscl"]["min_p"] >= 0.1 - 1e-12
    l1 = {}
    for N in (64, 128):
        for name, (G, exact), t_end, m, pde in (("advection", M.sine_advection(N), 0.5, 1, R.PDE_ADVECTION),
                                                ("density_wave", M.density_wave(N), 0.25, 5, R.PDE_EULER)):
            Gn, steps = M.run_global(G, t_end, 1.0 / N, 2, m, pde, g["cfl"], "muscl")
            l1[name, N] = float(np.mean(np.abs(Gn[..., 0] - exact(t_end))))
            want = g[name]["muscl_%d" % N]
            assert steps == want["steps"] and abs(l1[name, N] / want["l1"] - 1) < 1e-9, (name, N, steps, l1[name, N], want)
    for name, order in (("advection", 1.84), ("density_wave", 1.81)):
        got = float(np.log2(l1[name, 64] / l1[name, 128]))
        print("%s: L1 %.3e / %.3e, order %.3f" % (name, l1[name, 64], l1[name, 128], got))
        assert abs(got / order - 1) < 0.05, (name, got)


def test_recorded_sod_run():
    from examples.sod_tube_fv_walls import initial_state, l1_density
    from exahype_amd.boundary import Wall, fv_faces
    nx, P = 64, 4
    cond = fv_faces({(0, 0): Wall(), (0, 1): Wall()}, 2, 5, 0, R.PDE_EULER)[2]
    Gn, steps = M.run_global(R.assemble(initial_state(nx, P), 2), 0.1, 1.0 / (nx * P), 2, 5, R.PDE_EULER, GOLDEN["cfl"], "muscl", conditions=cond)
    l1 = l1_density(R.cut_patches(Gn, 2, (nx, 1), P)[..., 0], 0.1)
    print("Sod, 256 volumes: L1(rho) %.4e in %d steps" % (l1, steps))
    assert steps == GOLDEN["sod"]["muscl"]["steps"] and abs(l1 / GOLDEN["sod"]["muscl"]["l1"] - 1) < 1e-9
    assert abs(l1 / 3.97e-3 - 1) < 0.05


# ---- the C-ABI's argument checks (they come before the device check) -------------------------------------------------------------------
def test_header_declares_the_mode():
    text = open(os.path.join(ROOT, "include", "exahype_hip.h")).read()
    assert re.search(r"^#define\s+EXA_FV_MUSCL_HANCOCK\s+2\b", text, flags=re.M)
    assert re.search(r"^#define\s+EXA_PDE_FLAG_MUSCL_HANCOCK\s+16\b", text, flags=re.M)
    from exahype_amd import _lib, solvers
    assert _lib.FV_MUSCL_HANCOCK == 2 and solvers.FV_MUSCL_HANCOCK == 2


def _create(lib, *args):
    h = C.c_void_p()
    rc = lib.exa_fv_plan_create(*args, C.byref(h))
    msg = lib.exa_last_error().decode()
    if rc == EXA_OK:
        lib.exa_fv_plan_destroy(h)
    return rc, msg


def test_plan_create_takes_mode_2():
    """exa_fv_plan_create(0, 2, 2, 4, 2, 5, 0, 1, EXA_PDE_EULER, &p): the arguments pass -- without a GPU the answer is EXA_ERR_NO_DEVICE (it was
    EXA_ERR_INVALID, "unknown FV mode 2"), with one EXA_OK"""
    from exahype_amd import _lib
    lib = _lib.load()
    rc, msg = _create(lib, 0, 2, 2, 4, 2, 5, 0, 1, _lib.PDE_EULER)
    assert rc == (EXA_OK if _lib.device_count() > 0 else EXA_ERR_NO_DEVICE), (rc, msg)


def test_plan_create_refusals():
    from exahype_amd import _lib
    lib = _lib.load()
    rc, msg = _create(lib, 0, 2, 2, 4, 1, 5, 0, 1, _lib.PDE_EULER)
    assert rc == EXA_ERR_INVALID and "MUSCL-Hancock reads two halo layers" in msg, (rc, msg)
    rc, msg = _create(lib, 0, 2, 2, 4, 2, 5, 0, 1, _lib.PDE_EULER_REF2D)
    assert rc == EXA_ERR_INVALID and "EULER_REF2D" in msg, (rc, msg)
    rc, msg = _create(lib, 0, 3, 2, 4, 2, 5, 0, 1, _lib.PDE_EULER)
    assert rc == EXA_ERR_INVALID and "unknown FV mode 3" in msg, (rc, msg)
    # 3-D P = 12: 8 (16^3 5 + 14^3 5) = 273 600 bytes against 163 840
    rc, msg = _create(lib, 0, 2, 3, 12, 2, 5, 0, 1, _lib.PDE_EULER)
    assert rc == EXA_ERR_INVALID and "273600" in msg and "163840" in msg, (rc, msg)
    assert K.lds_plan(3, 12, 5, 5) is None
    # the shapes the mode must serve all have a plan
    for dim, P, n_real, V in [(2, p, 5, 5) for p in range(1, 33)] + [(2, p, 5, 10) for p in range(1, 21)] + [(3, p, 5, 6) for p in range(1, 9)]:
        assert K.lds_plan(dim, P, n_real, V) is not None, (dim, P, V)
        rc, msg = _create(lib, 0, 2, dim, P, 2, n_real, V - n_real, 1, _lib.PDE_EULER)
        assert rc != EXA_ERR_INVALID, (dim, P, V, msg)
    # the other modes answer as they did
    rc, msg = _create(lib, 0, 1, 2, 4, 0, 5, 0, 1, _lib.PDE_EULER)
    assert rc == EXA_ERR_INVALID and "the Rusanov stencil reads one halo layer" in msg


# ---- the generator's keyword -----------------------------------------------------------------------------------------------------------
def _swe(**kw):
    import sympy
    from exahype_amd.pde_codegen import SympyPDE
    g = 9.81

    def flux(q, d):
        u = q[1 + d] / q[0]
        f = [q[1 + d], q[1] * u, q[2] * u]
        f[1 + d] = f[1 + d] + g * q[0] ** 2 / 2
        return f
    return SympyPDE(3, flux, lambda q, d: sympy.Abs(q[1 + d] / q[0]) + sympy.sqrt(g * q[0]), max_dim=2, name="swe", **kw)


def test_keyword_refuses_what_the_scheme_has_no_place_for():
    sympy = pytest.importorskip("sympy")
    from exahype_amd.pde_codegen import SympyPDE
    adv = lambda q, d: [q[0] * (1.0 + d)]                          # noqa: E731
    eig = lambda q, d: sympy.Float(1.0 + d)                        # noqa: E731
    SympyPDE(1, adv, eig, max_dim=2, muscl_hancock=True)
    with pytest.raises(ValueError, match="source"):
        SympyPDE(1, adv, eig, max_dim=2, source=lambda q: [-q[0]], muscl_hancock=True)
    with pytest.raises(ValueError, match="non-conservative"):
        SympyPDE(1, adv, eig, max_dim=2, ncp=lambda q, dq, d: [q[0] * dq[0]], muscl_hancock=True)
    with pytest.raises(ValueError, match="position / time"):
        SympyPDE(1, lambda q, x, t, d: [q[0] * (1.0 + x[0])], eig, max_dim=2, muscl_hancock=True)
    with pytest.raises(TypeError):
        SympyPDE(1, adv, eig, 2, "user", None, None, None, None, None, False, True)          # keyword only


def test_keyword_leaves_other_term_sets_alone():
    pytest.importorskip("sympy")
    plain, flagged = _swe(), _swe(muscl_hancock=True)
    assert "HAS_MUSCL_HANCOCK" not in plain.source() and "static constexpr bool HAS_MUSCL_HANCOCK = true;" in flagged.source()
    assert plain.source() == flagged.source().replace(
        "    // the second-order MUSCL-Hancock patch update is built for this term set (exa_fv_muscl.hpp)\n"
        "    static constexpr bool HAS_MUSCL_HANCOCK = true;\n", "")
    # the key of a term set without the keyword: the recipe it always had -- its source, the files its units are built from, build.py, the
    # flags -- and none of the new unit's files
    csrc = os.path.join(ROOT, "exahype_amd", "csrc")
    h = hashlib.sha256(plain.source().encode())
    for f in ("dg_inst.hip", "fv_rusanov.hip", "exa_dg_kernels.hpp", "exa_dg_stream.hpp", "exa_dg_reg.hpp", "exa_dg_fused.hpp",
              "exa_dg_common.hpp", "exa_launch.hpp", "exa_pde.hpp", "exa_dg_plain.hpp", "exa_dg_m8.hpp", "exa_dg_boundary.hpp"):
        h.update(open(os.path.join(csrc, f), "rb").read())
    h.update(open(os.path.join(ROOT, "exahype_amd", "build.py"), "rb").read())
    h.update(repr(None).encode())
    h.update(os.environ.get("EXA_EXTRA_FLAGS", "").encode())
    assert plain.key() == h.hexdigest()[:16]
    assert flagged.key() != plain.key()

"""Conservative DG / FV interface of the a-posteriori subcell limiter for GENERATED term sets: SympyPDE(conservative_interface=True), the
marker and EXA_PDE_FLAG_CONSERVATIVE, the side library's unit lim_conserve_user.hip (its filler exa_user_fill_lim_conserve, the slots
behind exa_lim_face_flux / exa_lim_interface_correct) and SubcellLimiter.step / step_a_posteriori / run with conservative=True.

CPU: keyword, marker and refusals; the unit compiles against the generated shallow-water header and against a 24-variable system (whose
3-D N = 8 face-flux kernel would not fit 64 KB of LDS: the guard); the numpy restatement (tests/limiter_conservative_user_ref.py) holds the
dam break's totals to the rounding bound where the default mode loses 1e-3; the committed values come from it; the flag is visible to C99.
GPU: grids and masks of tests/test_limiter_conservative.py, tolerance 1e-10 of the largest magnitude.  Shallow water: every element of
fvflux and one conservative step against the restatement, the totals of that step against the bound; an outflow / wall box; generated Euler
against the built-in set (1e-12); a system with a source; three rounds with the cumulative mask equal in every cell; the dam break through
run() and through the example; the refusals that stay.

The conservation bound is limiter_conservative_ref.bound: 16 steps 2^-53 in the normalisation of limiter_mood_ref.defects.  The totals of
the one-step tests are summed in long double, so that the measurement adds none of its own."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import sympy

from tests import limiter_admissible_ref as R
from tests import limiter_conservative_ref as K
from tests import limiter_conservative_user_ref as U
from tests import limiter_mood_ref as M
from tests.test_gpu_distributed import _run_ranks
from tests.test_limiter_admissible import EULER_SOURCE_SHA256, SWE_SOURCE_SHA256, _with_criterion, euler_criterion, swe_lim
from tests.test_limiter_conservative import MARGIN, _defects_ld, _mask_array, _masks, _totals_ld
from tests.test_limiter_conservative import _dt as _euler_dt
from tests.test_limiter_conservative import _state as _euler_state
from tests.test_user_pde import NumpyPDE, euler_sympy, reaction_advection, swe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "exahype_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "limiter_conservative_dam_break.json")
MARKER = "static constexpr bool HAS_CONSERVATIVE_INTERFACE = true;"
ORDERS = [2, 3, 4, 6, 8]
NAMES = ["single", "adjacent", "same_neighbour", "all"]
gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def swe_cons():
    return _with_criterion(swe(), admissible=lambda q: [q[0]], dmp=(0,), conservative_interface=True)


@functools.lru_cache(maxsize=None)
def euler_cons():
    return _with_criterion(euler_sympy(), admissible=euler_criterion, dmp=(0, 4), conservative_interface=True)


@functools.lru_cache(maxsize=None)
def reaction_cons():
    return _with_criterion(reaction_advection(max_dim=2), conservative_interface=True)


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_keyword_generates_the_marker_and_nothing_else():
    """(fails on a tree without the feature: the constructor does not know the keyword)"""
    from exahype_amd.pde_codegen import SympyPDE
    base = swe()
    flux = lambda q, d: [e.subs(dict(zip(base.q, q)), simultaneous=True) for e in base.flux_exprs[d]]
    eig = lambda q, d: base.eig_exprs[d].subs(dict(zip(base.q, q)), simultaneous=True)
    p = SympyPDE(3, flux, eig, max_dim=2, name="shallow_water", conservative_interface=True)
    src = p.source()
    assert MARKER in src and p.conservative_interface
    # ... one block in front of the struct's end, nothing else
    a = src.index("    // the a-posteriori subcell limiter's conservative DG / FV interface")
    b = src.index("};\n}  // namespace exa")
    assert src[:a] + src[b:] == base.source()
    with pytest.raises(TypeError):                                   # keyword only
        SympyPDE(3, flux, eig, 2, "shallow_water", None, None, None, None, None, True)
    # with a criterion: the marker follows the criterion's block; a source term is allowed
    with_both = swe_cons().source()
    assert with_both.index("HAS_ADMISSIBLE = true") < with_both.index(MARKER)
    assert MARKER in reaction_cons().source() and "HAS_SOURCE = true" in reaction_cons().source()


def test_term_sets_without_the_keyword_generate_the_source_and_key_they_did():
    import hashlib
    s = swe().source()
    assert "CONSERVATIVE" not in s and "CONSERVATIVE" not in swe_lim().source()
    assert hashlib.sha256(s.encode()).hexdigest() == SWE_SOURCE_SHA256
    assert hashlib.sha256(euler_sympy().source().encode()).hexdigest() == EULER_SOURCE_SHA256
    off = _with_criterion(swe(), admissible=lambda q: [q[0]], dmp=(0,), conservative_interface=False)
    assert off.source() == swe_lim().source() and off.key() == swe_lim().key()
    assert swe_cons().key() != swe_lim().key()
    # the new files enter the key of term sets with the keyword only
    from exahype_amd import pde_codegen
    opened = []
    real_open = open

    def spy(path, *a, **kw):
        opened.append(os.path.basename(str(path)))
        return real_open(path, *a, **kw)
    pde_codegen.open = spy
    try:
        swe_lim().key()
        assert "lim_conserve_user.hip" not in opened and "exa_lim_conserve.hpp" not in opened
        swe_cons().key()
        assert "lim_conserve_user.hip" in opened and "exa_lim_conserve.hpp" in opened
    finally:
        del pde_codegen.open


def test_keyword_refuses_position_time_and_non_conservative_terms():
    from exahype_amd.pde_codegen import SympyPDE
    flux = lambda q, d: [q[0], q[1]]
    one = lambda q, d: sympy.Float(1)
    with pytest.raises(ValueError, match="position / time"):
        SympyPDE(2, lambda q, x, t, d: [q[0] * (1 + x[0]), q[1]], one, max_dim=2, conservative_interface=True)
    with pytest.raises(ValueError, match="position / time"):
        SympyPDE(2, flux, one, max_dim=2, source=lambda q, x, t: [t * q[0], 0], conservative_interface=True)
    with pytest.raises(ValueError, match="non-conservative product"):
        SympyPDE(2, flux, one, max_dim=2, ncp=lambda q, dq, d: [q[1] * dq[0], 0], conservative_interface=True)
    SympyPDE(2, flux, one, max_dim=2, source=lambda q: [-q[0], q[0]], conservative_interface=True)       # a source of the state alone is fine


ADVECTION_24 = """#pragma once
#include <hip/hip_runtime.h>
#include "exa_pde.hpp"
namespace exa {
struct UserPDE {                                  // linear advection of 24 variables, three dimensions
    static constexpr int NV = 24;
    static constexpr int NFLUX = 24;
    static constexpr int NAUX = 1;
    static constexpr int MAXDIM = 3;
    __device__ static inline double vel(int d) { return d == 0 ? 1.0 : (d == 1 ? 0.5 : -0.75); }
    __device__ static inline void flux_rt(const double* q, int d, double* F) {
        for (int v = 0; v < NV; v++) F[v] = vel(d) * q[v];
    }
    __device__ static inline double maxeig(const double*, int d) { return fabs(vel(d)); }
    __device__ static inline double maxeig_fast(const double*, int d) { return fabs(vel(d)); }
    static constexpr bool HAS_CONSERVATIVE_INTERFACE = true;
};
}  // namespace exa
"""


@pytest.mark.parametrize("which", ["shallow_water", "advection_24"])
def test_the_unit_compiles(tmp_path, which):
    """this one unit only, not a side library.  24 variables: the 3-D N = 8 face-flux kernel needs 2760 * 24 + 960 = 67 200 bytes of static
    LDS, more than the 65 536 a workgroup may declare -- without the guard hipcc refuses the unit"""
    import shutil
    hdr = tmp_path / "user_pde.hpp"
    hdr.write_text(swe_cons().source() if which == "shallow_water" else ADVECTION_24)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-pass-failed", "-I", CSRC,
                        "-DEXA_PDE_ID=100", '-DEXA_USER_PDE_HEADER="%s"' % hdr, "-c", os.path.join(CSRC, "lim_conserve_user.hip"),
                        "-o", str(tmp_path / "limc.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 2760 * 24 + 960 > 65536 >= 2760 * 23 + 960


@functools.lru_cache(maxsize=None)
def _dam(N, nx, rounds=3):
    return U.run_dam_break(N, nx, rounds=rounds)


@pytest.mark.parametrize("N", [4, 6, 8])
def test_restatement_conserves_the_dam_break_to_rounding(N):
    r = _dam(N, 16)
    print(r, "bound %.3e" % K.bound(r["steps"]))
    assert "failed" not in r
    assert max(r["cons"]) <= K.bound(r["steps"]) and len(r["cons"]) == 3
    assert r["min_h"] > 0 and r["unresolved"] == 0


def test_default_mode_loses_mass_on_the_same_case():
    r = R.run_dam_break(4, 16)
    print(r)
    assert "failed" not in r and r["mass"] > 1e-3


def test_golden_values_come_from_the_restatement():
    g = _golden()
    assert {"dim2_N4_nx16", "dim2_N6_nx16", "dim2_N8_nx16"} <= set(g)
    r, want = _dam(4, 16), g["dim2_N4_nx16"]
    assert r["steps"] == want["steps"] == 118 and r["max_troubled"] == want["max_troubled"] == 8 and r["unresolved"] == want["unresolved"] == 0
    for k in ("min_h", "change"):
        assert abs(r[k] - want[k]) <= 1e-9 * abs(want[k]), k
    for name, v in g.items():
        assert "failed" not in v and v["min_h"] > 0 and v["unresolved"] == 0, name
        assert max(v["cons"]) <= K.bound(v["steps"]) and len(v["cons"]) == 3, name      # at rounding level in every committed case


def test_flag_is_declared_for_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "exahype_hip.h"\n'
                   'int probe(int pde) { return (exa_pde_flags(pde) & EXA_PDE_FLAG_CONSERVATIVE) == 8 && EXA_PDE_FLAG_CONSERVATIVE == 8; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_example_term_set_is_the_tests():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import importlib
        ex = importlib.import_module("dam_break_limited")
    finally:
        sys.path.pop(0)
    assert ex.shallow_water().source() == swe_lim().source()         # the default is what it was
    assert ex.shallow_water(conservative_interface=True).source() == swe_cons().source()     # one side library serves the example and the tests


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _phase(nc, N, xi):
    dim = len(nc)
    ph = 0.0
    for a in range(dim):
        cs, ns = [1] * (2 * dim), [1] * (2 * dim)
        cs[a], ns[dim + a] = nc[a], N
        ph = ph + (a + 1) * (np.arange(nc[a]).reshape(cs) + xi.reshape(ns)) / nc[a]
    return ph


def _swe_state(N, nc, seed):
    """A smooth positive shallow-water state with node-wise noise and one jump, as test_limiter_conservative._state makes for Euler:
    h = 1 + 0.2 sin + noise, 0.4 times that in the layer c_0 = 0, velocities of 0.3"""
    rng = np.random.default_rng(seed)
    ops = M.operators(N)
    shape = tuple(nc) + (N, N)
    ph = _phase(nc, N, np.asarray(ops["xi"]))
    h = 1.0 + 0.2 * np.sin(2 * np.pi * ph) + 0.02 * rng.random(shape)
    h[0] *= 0.4
    u = np.zeros(shape + (3,))
    u[..., 0] = h
    for a in range(2):
        u[..., 1 + a] = h * (0.3 * np.cos(2 * np.pi * ph + a) + 0.02 * rng.random(shape))
    return u, ops


def _reaction_state(N, nc, seed):
    rng = np.random.default_rng(seed)
    ops = M.operators(N)
    shape = tuple(nc) + (N, N)
    ph = _phase(nc, N, np.asarray(ops["xi"]))
    u = np.stack([1.0 + 0.2 * np.sin(2 * np.pi * ph) + 0.02 * rng.random(shape), 0.5 + 0.1 * np.cos(2 * np.pi * ph) + 0.02 * rng.random(shape)], axis=-1)
    u[0] *= 0.4
    return u, ops


def _dt(u, dx, N, pde):
    lam = max(np.max(pde.maxeig(u, d)) for d in range(2))
    return 0.4 * dx[0] / ((2 * N - 1) * 2 * lam)


SWE_SIGN = {0: np.array([1.0, -1, 1]), 1: np.array([1.0, 1, -1])}
BOX = {(0, 0): "outflow", (0, 1): "wall", (1, 0): "wall", (1, 1): "outflow"}


def _bcs(box):
    """(the solver's boundary dict, the restatement's)"""
    from exahype_amd.boundary import Outflow, Wall
    if not box:
        return None, None
    return ({k: Outflow() if v == "outflow" else Wall(sign=SWE_SIGN[k[0]]) for k, v in BOX.items()},
            {k: ("outflow",) if v == "outflow" else ("wall", SWE_SIGN[k[0]]) for k, v in BOX.items()})


@functools.lru_cache(maxsize=None)
def _reference(N, name, box=False, conservative=True):
    """(u, mask, dt, dx, u_new, F~ per (cell, axis, side)) of one shallow-water step with the given mask, computed once and shared"""
    grid, cells = _masks(2)[name]
    u, ops = _swe_state(N, grid, 200 + N)
    dx = [1.0 / grid[0]] * 2
    pde = R.ShallowWater()
    dt = _dt(u, dx, N, pde)
    mask = _mask_array(grid, cells)
    fluxes = {}
    new = U.step_with_mask(u, mask, dt, dx, ops, pde, _bcs(box)[1], conservative=conservative, fluxes=fluxes)
    for a in (u, mask, new):
        a.setflags(write=False)
    return u, mask, dt, dx, new, fluxes


def _limiter(spde, dim, N, grid, dx, boundary=None, extra=2, builtin=False):
    from exahype_amd import solvers as exa
    kw = {} if builtin else dict(pde=spde.register(), n_vars=spde.n_vars)
    s = exa.AderDgSolver(dim, N, grid, dx=dx, boundary=boundary, **kw)
    return s, exa.SubcellLimiter(s, capacity=int(np.prod(grid)) + extra)


def _face_fluxes_of(s, lim, u, mask):
    """the device's fvflux [capacity, 2 dim, nv, face nodes] for the given state and mask; empty slots keep the sentinel -7.25"""
    import torch
    s.upload(u)
    lim._conservative_setup("step")
    m = torch.as_tensor(np.array(mask.reshape(-1))).to(s.dev)
    lim._compact(m)
    lim._project(m, s.u, s.time)
    lim._fvflux.fill_(-7.25)
    lim._face_flux()
    torch.cuda.synchronize()
    return lim._fvflux.cpu().numpy().reshape(lim.capacity, 2 * s.dim, s.nv, s.N ** (s.dim - 1))


@gpu
def test_flag_and_entries_of_the_side_library():
    from exahype_amd import _lib
    lib = _lib.load()
    pid = swe_cons().register()
    assert lib.exa_pde_flags(pid) == 4 | 8
    assert lib.exa_pde_flags(reaction_cons().register()) == 8
    assert lib.exa_pde_flags(swe_lim().register()) == 4
    so = C.CDLL(swe_cons().build())
    assert hasattr(so, "exa_user_fill_lim_conserve")
    assert not hasattr(C.CDLL(swe_lim().build()), "exa_user_fill_lim_conserve")


@gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("N", ORDERS)
def test_shallow_water_face_flux_equals_the_restatement(N, name):
    """every element of fvflux[slot][d*2+side][var][node] of the listed slots; the -1 slots behind them keep the sentinel"""
    u, mask, dt, dx, _, fluxes = _reference(N, name)
    s, lim = _limiter(swe_cons(), 2, N, mask.shape, dx)
    got = _face_fluxes_of(s, lim, u, mask)
    cells = list(zip(*np.nonzero(mask)))                           # the compacted list is in the order of the flat cell index
    scale = max(np.max(np.abs(f)) for f in fluxes.values())
    worst = 0.0
    for slot, idx in enumerate(cells):
        for a in range(2):
            for side in range(2):
                want = np.moveaxis(fluxes[(idx, a, side)].reshape(-1, 3), -1, 0)
                worst = max(worst, float(np.max(np.abs(got[slot, a * 2 + side] - want))))
    print("N %d %s: %d slots, max |g| %.3e, worst error %.3e" % (N, name, len(cells), scale, worst))
    assert worst <= 1e-10 * scale
    assert np.all(got[len(cells):] == -7.25)                       # empty slots: nothing written
    assert lim.capacity > len(cells) or name == "all"              # (every other mask leaves -1 slots)


@gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("N", ORDERS)
def test_shallow_water_step_equals_the_restatement_and_keeps_the_totals(N, name):
    """One step(dt, mask, conservative=True): every cell against the restatement, the totals of (h, hu, hv) within the bound of one step.
    The same step with conservative=False loses more than 100 times the bound in its worst variable -- wherever the mask has a DG / FV
    face at all: with every cell troubled there is none, both modes are the same FV update and both keep the totals."""
    u, mask, dt, dx, want, _ = _reference(N, name)
    w = M.operators(N)["w"]
    s, lim = _limiter(swe_cons(), 2, N, mask.shape, dx)
    s.upload(u)
    n = lim.step(dt, mask, conservative=True)
    got = lim.download()
    assert int(n) == int(mask.sum())
    tol = 1e-10 * np.max(np.abs(want))
    err = np.max(np.abs(got - want), axis=(2, 3, 4))
    d = _defects_ld(_totals_ld(u, w), _totals_ld(got, w))
    print("N %d %s: worst cell error %.3e of max |u| %.3e; defects %s, bound %.3e" % (N, name, err.max(), np.max(np.abs(want)), ["%.2e" % x for x in d], K.bound(1)))
    assert np.all(err <= tol), np.argwhere(err > tol)
    assert max(d) <= K.bound(1), d
    s.upload(u)
    s.time = 0.0
    lim.step(dt, mask, conservative=False)
    plain = lim.download()
    d0 = _defects_ld(_totals_ld(u, w), _totals_ld(plain, w))
    print("   without the correction: %s" % ["%.2e" % x for x in d0])
    if name == "all":
        assert max(d0) <= K.bound(1), d0
    else:
        assert max(d0) > 100 * K.bound(1), d0
        # the correction is what was compared: without it the same step differs from the restatement by far more than the tolerance
        assert np.max(np.abs(plain - want)) > 1e-6 * np.max(np.abs(want))


@gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("N", [3, 4])
def test_shallow_water_outflow_wall_box(N, name):
    u, mask, dt, dx, want, _ = _reference(N, name, True)
    s, lim = _limiter(swe_cons(), 2, N, mask.shape, dx, boundary=_bcs(True)[0])
    s.upload(u)
    lim.step(dt, mask, conservative=True)
    got = lim.download()
    tol = 1e-10 * np.max(np.abs(want))
    err = np.max(np.abs(got - want), axis=(2, 3, 4))
    print("N %d %s box: worst cell error %.3e of max |u| %.3e" % (N, name, err.max(), np.max(np.abs(want))))
    assert np.all(err <= tol), np.argwhere(err > tol)


@gpu
@pytest.mark.parametrize("N", [3, 6, 8])
def test_generated_euler_equals_the_builtin_set(N):
    """3-D, mask `adjacent`: fvflux and one conservative step of the generated Euler set against the built-in one, 1e-12 relative (the
    tolerance tests/test_user_pde.py holds the two sets to; the two round their eigenvalues differently).  N = 8: a face fills the
    wavefront and the LDS need is largest."""
    grid, cells = _masks(3)["adjacent"]
    u, _ = _euler_state(3, N, grid, 300 + N)
    dx = [1.0 / grid[0]] * 3
    dt = _euler_dt(u, dx, 3, N)
    mask = _mask_array(grid, cells)
    out = []
    for builtin in (True, False):
        s, lim = _limiter(euler_cons(), 3, N, grid, dx, builtin=builtin)
        flux = _face_fluxes_of(s, lim, u, mask)
        s.upload(u)
        s.time = 0.0
        lim.step(dt, mask, conservative=True)
        out.append((flux, lim.download()))
    (f0, u0), (f1, u1) = out
    nslots = len(cells)
    ef = np.max(np.abs(f0[:nslots] - f1[:nslots])) / np.max(np.abs(f0[:nslots]))
    eu = np.max(np.abs(u0 - u1)) / np.max(np.abs(u0))
    print("N %d: fvflux rel %.3e, step rel %.3e" % (N, ef, eu))
    assert np.all(f1[nslots:] == -7.25)
    assert ef <= 1e-12 and eu <= 1e-12
    # ... and the correction took place: the same step without it is far away
    s.upload(u)
    s.time = 0.0
    lim.step(dt, mask)
    assert np.max(np.abs(lim.download() - u1)) > 1e-6 * np.max(np.abs(u1))


@gpu
@pytest.mark.parametrize("name", ["single", "adjacent"])
def test_system_with_a_source_equals_the_restatement(name):
    """reaction_advection (two variables: the per-variable limiter kernels; S(q) in the DG step and as + dt S in the FV update).  The
    totals are not checked: the source changes them."""
    N = 3
    grid, cells = _masks(2)[name]
    u, ops = _reaction_state(N, grid, 17)
    dx = [1.0 / grid[0]] * 2
    pde = NumpyPDE(reaction_cons())
    assert hasattr(pde, "source")
    dt = _dt(u, dx, N, pde)
    mask = _mask_array(grid, cells)
    want = U.step_with_mask(u, mask, dt, dx, ops, pde)
    s, lim = _limiter(reaction_cons(), 2, N, grid, dx)
    s.upload(u)
    lim.step(dt, mask, conservative=True)
    got = lim.download()
    tol = 1e-10 * np.max(np.abs(want))
    err = np.max(np.abs(got - want), axis=(2, 3, 4))
    print("%s: worst cell error %.3e of max |u| %.3e" % (name, err.max(), np.max(np.abs(want))))
    assert np.all(err <= tol), np.argwhere(err > tol)
    plain = U.step_with_mask(u, mask, dt, dx, ops, pde, conservative=False)
    assert np.max(np.abs(plain - want)) > 1e-6 * np.max(np.abs(want))


def _rough_dam(N, nc):
    """the dam break's two levels along x with a cell-internal oscillation of the depth, so that the DG candidate of the first step already
    leaves the bounds next to the jumps"""
    ops = M.operators(N)
    u = R.dam_initial(N, nc[0])
    u = np.broadcast_to(u, tuple(nc) + u.shape[2:]).copy()
    xi = np.asarray(ops["xi"])
    osc = (1 + 0.03 * np.sin(2 * np.pi * xi)).reshape(1, 1, N, 1) * (1 + 0.03 * np.sin(2 * np.pi * (xi + 0.1))).reshape(1, 1, 1, N)
    cellph = np.cos(1.7 * np.arange(int(np.prod(nc)))).reshape(tuple(nc) + (1, 1))
    u[..., 0] *= 1 + (osc - 1) * cellph
    return u, ops


@gpu
def test_rounds_equal_the_restatement():
    """two dam-break steps of three rounds each: the cumulative mask equal in every cell, u to 1e-10"""
    N, nc = 4, (8, 2)
    u, ops = _rough_dam(N, nc)
    dx = [1.0 / nc[0]] * 2
    pde = R.ShallowWater()
    dt = _dt(u, dx, N, pde)
    s, lim = _limiter(swe_cons(), 2, N, nc, dx, extra=0)
    s.upload(u)
    for k in range(2):
        info = {}
        u, cum, _ = U.step(u, dt, dx, ops, pde, R.swe_admissible, (0,), rounds=3, info=info)
        print("step %d: new cells per round %s, smallest margins %s" % (k, info["new"], ["%.2e" % x for x in info["margin"]]))
        assert min(info["margin"]) >= MARGIN                       # no cell may be excused
        assert 0 < cum.sum() < cum.size
        n = lim.step_a_posteriori(dt, conservative=True, rounds=3)
        got_mask = lim._mask_cum.cpu().numpy()
        assert np.array_equal(got_mask, cum), np.argwhere(got_mask != cum)
        assert int(n) == int(cum.sum())
        err = np.max(np.abs(lim.download() - u)) / np.max(np.abs(u))
        print("   rel err %.3e" % err)
        assert err < 1e-10


@gpu
@pytest.mark.parametrize("N", [4, 6])
def test_dam_break_conserves_through_run(N):
    import torch
    nx = 16
    want = _golden()["dim2_N%d_nx%d" % (N, nx)]
    s, lim = _limiter(swe_cons(), 2, N, (nx, 1), [1.0 / nx] * 2, extra=0)
    assert lim.capacity == 16
    ops = s.operators()
    u0 = R.dam_initial(N, nx)
    s.upload(u0)
    worst = []
    steps = lim.run(want["t_end"], cfl=want["cfl"], track=True, conservative=True, rounds=3,
                    monitor=lambda l, k, c: worst.append(l.s.u[..., 0].min()))
    torch.cuda.synchronize()
    st = lim.stats
    assert set(st) == {"min_admissible", "max_troubled", "finite", "unresolved"} and st["min_admissible"].shape == (1,)
    u = lim.download()
    change = R.depth_change(u, u0, ops["w"])
    cons = M.defects(M.totals(u0, ops["w"]), M.totals(u, ops["w"]))
    print("N %d: steps %d (restatement %d) change %.8f (%.8f) min h %.6f (%.6f) troubled <= %d (%d) unresolved %d"
          % (N, steps, want["steps"], change, want["change"], st["min_admissible"][0].item(), want["min_h"], st["max_troubled"].item(),
             want["max_troubled"], st["unresolved"].item()))
    print("   cons %s (restatement %s), bound %.3e" % (cons, want["cons"], K.bound(steps)))
    assert bool(st["finite"]) and np.isfinite(u).all()
    assert abs(s.time - want["t_end"]) < 1e-12
    assert abs(steps - want["steps"]) <= 0.01 * want["steps"]
    assert abs(change - want["change"]) <= 0.01 * want["change"]
    assert st["max_troubled"].item() == want["max_troubled"]
    assert st["unresolved"].item() == 0
    assert st["min_admissible"][0].item() > 0 and torch.stack(worst).min().item() > 0 and len(worst) == steps      # over every step
    assert max(cons) <= K.bound(steps) and len(cons) == 3, cons


@gpu
def test_example_runs_conservative():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dam_break_limited.py"), "16", "4", "0.05", "conservative"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = r.stdout.strip().splitlines()[-1]
    vals = dict(kv.split("=") for kv in line.split())
    want = _golden()["dim2_N4_nx16"]
    steps = int(vals["steps"])
    assert abs(steps - want["steps"]) <= 0.01 * want["steps"] and float(vals["min_h"]) > 0 and int(vals["max_troubled"]) == want["max_troubled"]
    assert float(vals["mass_defect"]) <= K.bound(steps) and vals["unresolved"] == "0"


@gpu
def test_still_refuses_a_registered_set_without_the_keyword():
    from exahype_amd import solvers as exa
    s = exa.AderDgSolver(2, 4, (3, 2), pde=swe_lim().register(), n_vars=3, dx=[0.5, 0.5], fused_single_stage=False)
    lim = exa.SubcellLimiter(s, capacity=4)
    with pytest.raises(ValueError, match="built-in Euler") as e:
        lim.step_a_posteriori(1e-4, conservative=True)
    assert "conservative_interface=True" in str(e.value)
    buf = (C.c_double * 8)()
    cells = (C.c_long * 1)(-1)
    assert s.lib.exa_lim_face_flux(s._plan, C.cast(buf, C.c_void_p), C.cast(cells, C.c_void_p), 1, C.cast(buf, C.c_void_p), None) == -1
    msg = s.lib.exa_last_error()
    assert b"built-in Euler" in msg and b"conservative_interface" in msg


PARTITION_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from exahype_amd import solvers as exa
from tests.test_limiter_conservative_user import swe_cons
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
part = exa.CartesianPartition(world, rank, 2, [2, 1])
s = exa.AderDgSolver(2, 4, (4, 2), dx=[1.0 / 8] * 2, pde=swe_cons().register(), n_vars=3, part=part, backend_is_gloo=True)
lim = exa.SubcellLimiter(s, capacity=8)
for call in (lambda: lim.step_a_posteriori(1e-3, conservative=True), lambda: lim.run(1e-3, conservative=True),
             lambda: lim.step(1e-3, np.zeros((4, 2), dtype=bool), conservative=True)):
    try:
        call()
    except ValueError as e:
        assert "partitioned" in str(e) and "out of scope" in str(e), e
    else:
        raise AssertionError("a partitioned grid was accepted")
print("rank", rank, "refused")
dist.barrier(); dist.destroy_process_group()
'''


@gpu
def test_still_refuses_a_partitioned_axis(tmp_path):
    swe_cons().build()                                               # once, before the ranks start
    _run_ranks(tmp_path, PARTITION_WORKER % dict(root=ROOT), 2)

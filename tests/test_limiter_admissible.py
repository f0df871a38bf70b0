"""A-posteriori subcell limiting with the term set's own criterion: SympyPDE(admissible=..., dmp=...), the generated detection kernels
(the side library's unit lim_user.hip behind exa_lim_snapshot / exa_lim_detect), exa_lim_bounds_count and SubcellLimiter.

CPU: code generation and its refusals, the unchanged source of term sets without the keywords, the C-ABI entry, the numpy restatement
(tests/limiter_admissible_ref.py) against limiter_mood_ref with the Euler criterion, and why the feature exists: a smooth shallow-water
state with hv < 0 is troubled in the Euler layout and clean with the criterion [h].
GPU: masks equal to the restatement's in EVERY cell (the inputs keep every decision quantity 1e-9 away from its threshold; asserted on the
numpy side before the launch), bounds bit for bit, generated Euler against the built-in detector, K_DMP = 0 and one variable, two ranks,
and the double dam break through run() against the committed restatement values."""
import ctypes as C
import functools
import hashlib
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import sympy

from tests import limiter_admissible_ref as R
from tests import limiter_mood_ref as M
from tests.test_limiter_a_posteriori import MARGIN
from tests.test_user_pde import euler_sympy, reaction_advection, swe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "limiter_dam_break.json")
gpu = pytest.mark.gpu

# generated source of swe() / euler_sympy() (no keywords) at the commit before the keywords existed
SWE_SOURCE_SHA256 = "ebeae88b17de2a63df7d09f5f18263fbc213ae3de279f2e4ff0018d1e9eb8cd7"
EULER_SOURCE_SHA256 = "560a5f8d325b9774300032475e97db7983824612e6ba1295fc72bef47a00a1e6"


def _with_criterion(base, **kw):
    """the term set `base` (a SympyPDE built without the keywords) again, with admissible= / dmp="""
    from exahype_amd.pde_codegen import SympyPDE
    sub = lambda e, q: e.subs(dict(zip(base.q, q)), simultaneous=True)
    return SympyPDE(base.n_vars, flux=lambda q, d: [sub(e, q) for e in base.flux_exprs[d]], max_eigenvalue=lambda q, d: sub(base.eig_exprs[d], q),
                    source=(lambda q: [sub(e, q) for e in base.source_exprs]) if base.source_exprs is not None else None,
                    max_dim=base.max_dim, name=base.name, **kw)


def euler_criterion(q):
    return [q[0], sympy.Float(0.4) * (q[4] - (q[1] ** 2 + q[2] ** 2 + q[3] ** 2) / (2 * q[0]))]


@functools.lru_cache(maxsize=None)
def swe_lim():
    return _with_criterion(swe(), admissible=lambda q: [q[0]], dmp=(0,))


@functools.lru_cache(maxsize=None)
def euler_lim():
    return _with_criterion(euler_sympy(), admissible=euler_criterion, dmp=(0, 4))


@functools.lru_cache(maxsize=None)
def reaction_lim():
    return _with_criterion(reaction_advection(max_dim=2), admissible=lambda q: [q[0]], dmp=())


@functools.lru_cache(maxsize=None)
def advection_one():
    from exahype_amd.pde_codegen import SympyPDE
    a = (1.0, 0.5)
    return SympyPDE(1, flux=lambda q, d: [a[d] * q[0]], max_eigenvalue=lambda q, d: sympy.Float(abs(a[d])), max_dim=2, name="advection_one",
                    dmp=(0,))


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_codegen_marker_members_flag_and_refusals():
    from exahype_amd import _lib
    from exahype_amd.pde_codegen import SympyPDE
    base = swe()
    flux = lambda q, d: [e.subs(dict(zip(base.q, q)), simultaneous=True) for e in base.flux_exprs[d]]
    eig = lambda q, d: base.eig_exprs[d].subs(dict(zip(base.q, q)), simultaneous=True)
    p = SympyPDE(3, flux, eig, max_dim=2, name="shallow_water", admissible=lambda q: [q[0]], dmp=(0,))
    src = p.source()
    for piece in ("HAS_ADMISSIBLE = true", "K_ADM = 1;", "K_DMP = 1;", "DMP_VAR[1] = {0};",
                  "__device__ static inline void admissible(const double* q, double* g)", "g[0] = q[0];"):
        assert piece in src, piece
    assert "fast_rcp" not in src[src.index("HAS_ADMISSIBLE"):]        # IEEE division in the criterion
    two = SympyPDE(5, lambda q, d: list(q), lambda q, d: sympy.Float(1), admissible=euler_criterion, dmp=(4, 0)).source()
    tail = two[two.index("HAS_ADMISSIBLE"):]
    assert "K_ADM = 2;" in tail and "DMP_VAR[2] = {4, 0};" in tail and "/q[0]" in tail and "fast_rcp" not in tail
    only_dmp = SympyPDE(1, lambda q, d: [q[0]], lambda q, d: sympy.Float(1), dmp=(0,)).source()
    assert "K_ADM = 0;" in only_dmp and "K_DMP = 1;" in only_dmp
    nothing_watched = SympyPDE(2, lambda q, d: list(q), lambda q, d: sympy.Float(1), admissible=lambda q: [q[0]], dmp=()).source()
    assert "K_DMP = 0;" in nothing_watched
    mk = lambda **kw: SympyPDE(3, flux, eig, max_dim=2, **kw)
    for bad in (dict(admissible=lambda q: [q[0] + p.x[0]]), dict(admissible=lambda q: [q[0] * p.t]),          # x / t
                dict(admissible=lambda q: [q[0]] * 5), dict(admissible=lambda q: []),                          # more than four, none
                dict(dmp=(3,)), dict(dmp=(-1,)), dict(admissible=lambda q: [q[0]], dmp=(0, 0)),                # out of range, duplicates
                dict(dmp=(0, 1, 2, 0, 1))):
        with pytest.raises(ValueError):
            mk(**bad)
    pid = p.register()                                               # builds the side library with its detector unit
    lib = _lib.load()
    assert lib.exa_pde_flags(pid) & 4 and not lib.exa_pde_flags(pid) & 3
    assert lib.exa_pde_flags(swe().register()) == 0


def test_term_sets_without_the_keywords_generate_the_source_they_did():
    s = swe().source()
    assert "HAS_ADMISSIBLE" not in s and "K_DMP" not in s
    assert hashlib.sha256(s.encode()).hexdigest() == SWE_SOURCE_SHA256
    assert hashlib.sha256(euler_sympy().source().encode()).hexdigest() == EULER_SOURCE_SHA256
    # ... and the keywords add one block in front of the struct's end, nothing else
    with_kw = swe_lim().source()
    a = with_kw.index("    // what the a-posteriori subcell limiter checks")
    b = with_kw.index("};\n}  // namespace exa")
    assert with_kw[:a] + with_kw[b:] == s
    assert swe().key() != swe_lim().key()


def test_bounds_count_is_exported_declared_and_zero_for_null(tmp_path):
    from exahype_amd import _lib
    lib = _lib.load()
    assert lib.exa_lim_bounds_count(None) == 0
    plan = C.create_string_buffer(4096)                              # stands in for a plan of a built-in term set (pde 0)
    assert lib.exa_lim_bounds_count(C.cast(plan, C.c_void_p)) == 4
    src = tmp_path / "use.c"
    src.write_text('#include "exahype_hip.h"\n'
                   'long probe(const exa_dg_plan* p) { return exa_lim_bounds_count(p) + EXA_PDE_FLAG_ADMISSIBLE; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                        "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _euler_cases():
    """(name, old, cand, kwargs of detect) in the case families of tests/test_limiter_a_posteriori.py, 2-D and 3-D"""
    from tests.test_limiter_a_posteriori import _level_state, _perturbed
    out = []
    for dim, N, nc in ((2, 3, (5, 3)), (2, 4, (1, 4)), (3, 3, (3, 2, 4)), (3, 4, (2, 3, 2))):
        flat = _level_state(dim, N, (1,) * dim, 7, noise=0.0)
        flat = np.broadcast_to(flat, tuple(nc) + flat.shape[dim:]).copy()
        x = np.linspace(0, 1, flat[..., 0].size, endpoint=False).reshape(flat.shape[:-1])
        smooth = flat.copy()
        smooth[..., 0] *= 1 + 0.05 * np.sin(2 * np.pi * x)
        out.append(("clean", smooth, smooth * (1 + 1e-6 * np.cos(2 * np.pi * x))[..., None], {}))
        old = _level_state(dim, N, nc, 11 * N + dim)
        out.append(("random", old, _perturbed(old, dim, 5 * N + dim), {}))
        c, last, mid = (0,) * dim, (N - 1,) * dim, (N // 2,) * dim
        for name in ("overshoot", "undershoot E", "negative pressure", "NaN", "inf"):
            cand = flat.copy()
            if name == "overshoot":
                cand[c + last + (0,)] += 0.01
            elif name == "undershoot E":
                cand[c + mid + (4,)] -= 0.01
            elif name == "negative pressure":
                cand[c + (0,) * dim + (1,)] = 3.0 * np.sqrt(cand[c + (0,) * dim + (0,)] * cand[c + (0,) * dim + (4,)])
            elif name == "NaN":
                cand[c + last + (2,)] = np.nan
            else:
                cand[c + mid + (3,)] = -np.inf
            out.append((name, flat, cand, {}))
        # a jump at the periodic wrap, and the same with no neighbour across the faces of that axis
        axis = dim - 1
        jump = flat.copy()
        low = [slice(None)] * dim
        low[axis] = slice(0, nc[axis] - 1)
        jump[tuple(low)] *= 0.25
        cand = jump.copy()
        cand[tuple(low) + (0,) * dim + (0,)] = 0.6 * float(flat[(0,) * (2 * dim) + (0,)])
        out.append(("wrap", jump, cand, {}))
        out.append(("no neighbour", jump, cand, dict(no_neighbour={(axis, 0), (axis, 1)})))
        # ghost bounds across the faces of axis 0: the neighbour block's layers hold other levels
        rng = np.random.default_rng(3 * N + dim)
        other = _level_state(dim, N, nc, 19 * N + dim)
        gb = M.cell_bounds(other)
        ghost = {(0, 0): gb[-1], (0, 1): gb[0]}
        cand = _perturbed(old, dim, 29 + dim)
        cand[..., 0] += 0.05 * rng.random(cand.shape[:-1])
        out.append(("ghost", old, cand, dict(ghost=ghost)))
    return out


def test_restatement_with_the_euler_criterion_is_limiter_mood_ref():
    crit = R.criterion(euler_lim())
    decided = 0
    for name, old, cand, kw in _euler_cases():
        want, wm = M.detect(cand, M.cell_bounds(old), **kw)
        assert np.array_equal(R.cell_bounds(old, (0, 4)), M.cell_bounds(old))
        got, gm = R.detect(cand, R.cell_bounds(old, (0, 4)), crit, (0, 4), **kw)
        assert np.array_equal(got, want), (name, np.argwhere(got != want))
        assert min(wm.min(), gm.min()) >= MARGIN, name               # (the two evaluations of the pressure round differently)
        decided += int(want.sum())
        if name in ("overshoot", "undershoot E", "negative pressure", "NaN", "inf"):
            assert want.sum() == 1 and want.flat[0]
        if name == "clean":
            assert not want.any()
    assert decided > 20


def _swe_smooth(N, nc, hv=-0.3):
    """smooth positive shallow-water state: h = 1 + 0.05 sin over all nodes, u = 0.2, v = hv (< 0: hv is negative everywhere)"""
    shape = tuple(nc) + (N, N)
    x = np.linspace(0, 1, int(np.prod(shape)), endpoint=False).reshape(shape)
    q = np.zeros(shape + (3,))
    q[..., 0] = 1 + 0.05 * np.sin(2 * np.pi * x)
    q[..., 1] = 0.2 * q[..., 0]
    q[..., 2] = hv * q[..., 0]
    return q, x


def test_why_the_feature_exists_shallow_water_in_the_euler_layout():
    """h, hu, hv with hv < 0: the Euler layout reads hv as an energy and hu as the only momentum, p = 0.4 (hv - hu^2 / (2 h)) < 0 -- every cell
    is troubled and the grid would run first-order FV; with the criterion [h] and the DMP on h the same smooth state is clean"""
    old, x = _swe_smooth(4, (3, 3))
    cand = old * (1 + 1e-6 * np.cos(2 * np.pi * x))[..., None]
    euler_layout, _ = M.detect(cand, M.cell_bounds(old))
    assert euler_layout.all()
    own, margin = R.detect(cand, R.cell_bounds(old, (0,)), R.swe_admissible, (0,))
    assert not own.any() and margin.min() >= MARGIN
    # hv < 0 on part of the grid only: the cells there, and none with the criterion
    part = old.copy()
    part[:2, :, :, :, 2] *= -1.0
    euler_layout, _ = M.detect(part, M.cell_bounds(part))
    assert euler_layout[2].all()
    assert not R.detect(part, R.cell_bounds(part, (0,)), R.swe_admissible, (0,))[0].any()


def test_golden_values_come_from_the_restatement():
    g = _golden()
    assert sorted(g) == ["dim2_N4_nx16", "dim2_N6_nx16"]
    for name, want in g.items():
        r = R.run_dam_break(want["N"], want["nx"], 2, t_end=want["t_end"], cfl=want["cfl"])
        print(r)
        assert "failed" not in r and r["min_h"] > 0                  # the restatement itself keeps h > 0 at both orders, CFL 0.4
        assert want["cfl"] == 0.4 and want["t_end"] == 0.05
        assert r["steps"] == want["steps"] and r["max_troubled"] == want["max_troubled"] and 0 < want["max_troubled"] < 16
        for k in ("change", "min_h"):
            assert abs(r[k] - want[k]) <= 1e-9 * abs(want[k]), k


def test_example_and_scripts_import_without_gpu():
    for rel in ("examples/dam_break_limited.py", "scripts/quick_bench_limiter_admissible.py", "scripts/make_limiter_admissible_golden.py"):
        src = open(os.path.join(ROOT, rel)).read()
        compile(src, rel, "exec")
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import importlib
        ex = importlib.import_module("dam_break_limited")
    finally:
        sys.path.pop(0)
    p = ex.shallow_water()
    assert p.adm_exprs == [p.q[0]] and p.dmp_vars == [0]
    assert p.source() == swe_lim().source()                          # one side library serves the example and the tests


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
class _Detector:
    """one solver + limiter per (term set, shape, boundary); detect(old, cand) -> (mask, bounds) as numpy"""

    def __init__(self, spde, dim, N, nc, boundary=None):
        from exahype_amd import solvers as exa
        kw = dict(pde=spde.register(), n_vars=spde.n_vars) if spde is not None else {}
        self.s = exa.AderDgSolver(dim, N, nc, dx=[1.0 / nc[0]] * dim, boundary=boundary, **kw)
        self.lim = exa.SubcellLimiter(self.s, capacity=4)
        self.nc = tuple(nc)

    def __call__(self, old, cand):
        self.s.upload(cand)
        m = self.lim.detect_candidate(old).cpu().numpy()
        assert m.dtype == np.bool_ and m.shape == self.nc
        nb = self.s.lib.exa_lim_bounds_count(self.s._plan)
        assert self.lim._bounds.shape == (int(np.prod(self.nc)), nb)
        return m, self.lim._bounds.cpu().numpy().reshape(self.nc + (nb,))


def _check(det, old, cand, admissible, dmp, expect=None, no_neighbour=(), label=""):
    R.reset_margin()
    want, margin = R.detect(cand, R.cell_bounds(old, dmp), admissible, dmp, no_neighbour=no_neighbour)
    print("%s N %d nc %s: %d of %d troubled, smallest margin %.3e" % (label, det.s.N, det.nc, want.sum(), want.size, R.smallest_margin()))
    assert R.smallest_margin() >= MARGIN and margin.min() >= MARGIN  # no cell may be excused
    if expect is not None:
        assert np.array_equal(want, expect), "the case '%s' does not decide what it was built to decide" % label
    got, bounds = det(old, cand)
    assert np.array_equal(got, want), (label, np.argwhere(got != want))
    assert np.array_equal(bounds, R.cell_bounds(old, dmp)), label    # min / max are exact
    return want


def _only(nc, *cells):
    e = np.zeros(nc, dtype=bool)
    for c in cells:
        e[c] = True
    return e


@gpu
@pytest.mark.parametrize("nc", [(3, 3), (1, 4), (2, 3)])
@pytest.mark.parametrize("N", [2, 3, 4, 6, 8])
def test_shallow_water_detector_equals_the_restatement(N, nc):
    from exahype_amd.boundary import Outflow, Wall
    det = _Detector(swe_lim(), 2, N, nc)
    assert det.s.lib.exa_lim_bounds_count(det.s._plan) == 2
    old, x = _swe_smooth(N, nc)
    clean = old * (1 + 1e-6 * np.cos(2 * np.pi * x))[..., None]
    adm, dmp = R.swe_admissible, (0,)
    none = np.zeros(nc, dtype=bool)
    _check(det, old, clean, adm, dmp, none, label="clean")
    lo, hi = R.neighbourhood(R.cell_bounds(old, dmp))
    delta = np.maximum(R.D0, R.EPS * (hi - lo))
    cells = [tuple(int(i) for i in np.unravel_index(k, nc)) for k in np.linspace(0, np.prod(nc) - 1, 4).astype(int)]
    first, last = (0, 0), (N - 1, N - 1)
    c = cells[0]
    cand = clean.copy()
    cand[c + last + (0,)] = 0.0                                      # h <= floor at one node (the DMP sees it too)
    _check(det, old, cand, adm, dmp, _only(nc, c), label="h <= floor")
    cand = clean.copy()
    cand[c + last + (0,)] = 5e-13                                    # 0 < h <= floor
    _check(det, old, cand, adm, dmp, _only(nc, c), label="0 < h <= floor")
    c = cells[1]
    cand = clean.copy()
    cand[c + last + (1,)] = np.nan                                   # in a momentum: only the finiteness check sees it
    _check(det, old, cand, adm, dmp, _only(nc, c), label="NaN")
    c = cells[2]
    cand = clean.copy()
    cand[c + first + (2,)] = np.inf
    _check(det, old, cand, adm, dmp, _only(nc, c), label="+inf")
    c = cells[3]
    for factor, expect, label in ((2.0, _only(nc, c), "beyond delta"), (0.5, none, "inside delta")):
        for which in ("over", "under", "both"):
            cand = clean.copy()
            if which in ("over", "both"):
                cand[c + last + (0,)] = hi[c][0] + factor * delta[c][0]
            if which in ("under", "both"):
                cand[c + first + (0,)] = lo[c][0] - factor * delta[c][0]
            _check(det, old, cand, adm, dmp, expect, label="%s %s" % (which, label))
    # outflow / wall faces: no neighbour across them.  The first layer of the axis holds three times the depth; a node of every cell of the
    # last layer raised to twice its level is within the bounds only through the periodic wrap
    for axis in range(2):
        if nc[axis] < 2:
            continue
        jump = old.copy()
        fl, ll = [slice(None)] * 2, [slice(None)] * 2
        fl[axis], ll[axis] = 0, nc[axis] - 1
        jump[tuple(fl)] *= 3.0
        cand = jump.copy()
        cand[tuple(ll) + last + (0,)] = 2.0
        sign = [1.0, 1.0, 1.0]
        sign[1 + axis] = -1.0
        faces = {(axis, 0), (axis, 1)}
        per = _check(det, jump, cand, adm, dmp, label="jump, periodic axis %d" % axis)
        bdet = _Detector(swe_lim(), 2, N, nc, boundary={(axis, 0): Outflow(), (axis, 1): Wall(sign=sign)})
        bc = _check(bdet, jump, cand, adm, dmp, no_neighbour=faces, label="jump, outflow / wall axis %d" % axis)
        assert not per[tuple(ll)].any()
        if nc[axis] >= 3:                                            # (two cells: the first layer is the inner neighbour as well)
            assert bc[tuple(ll)].all()


def _euler_defects(old):
    """candidate with an overshoot, an energy undershoot, a negative pressure, a NaN and an inf in five cells, tiny noise elsewhere"""
    dim = M._dim(old)
    nc, N = old.shape[:dim], old.shape[dim]
    rng = np.random.default_rng(5)
    cand = old * (1 + 1e-6 * rng.uniform(-1, 1, old.shape[:-1]))[..., None]
    cells = [tuple(int(i) for i in np.unravel_index(k, nc)) for k in np.linspace(0, np.prod(nc) - 1, 5).astype(int)]
    last, mid, zero = (N - 1,) * dim, (N // 2,) * dim, (0,) * dim
    cand[cells[0] + last + (0,)] += 2.0
    cand[cells[1] + mid + (4,)] -= 1.0
    cand[cells[2] + zero + (1,)] = 3.0 * np.sqrt(cand[cells[2] + zero + (0,)] * cand[cells[2] + zero + (4,)])
    cand[cells[3] + last + (2,)] = np.nan
    cand[cells[4] + mid + (3,)] = -np.inf
    return cand, cells


@gpu
@pytest.mark.parametrize("N", [6, 8])
def test_generated_euler_criterion_equals_the_builtin_detector(N):
    """3-D, N^3 > 64: four waves per cell, the cross-wave reduction through LDS"""
    from tests.test_limiter_conservative import _state
    nc = (2, 2, 3)
    old, _ = _state(3, N, nc, 40 + N)
    cand, cells = _euler_defects(old)
    R.reset_margin()
    want, _ = R.detect(cand, R.cell_bounds(old, (0, 4)), R.criterion(euler_lim()), (0, 4))
    ref, margin = M.detect(cand, M.cell_bounds(old))
    print("N %d: %d of %d troubled, smallest margins %.3e %.3e" % (N, want.sum(), want.size, R.smallest_margin(), margin.min()))
    assert R.smallest_margin() >= MARGIN and margin.min() >= MARGIN
    assert np.array_equal(want, ref) and all(want[c] for c in cells) and not want.all()
    builtin = _Detector(None, 3, N, nc)
    generated = _Detector(euler_lim(), 3, N, nc)
    assert builtin.s.lib.exa_lim_bounds_count(builtin.s._plan) == 4 and generated.s.lib.exa_lim_bounds_count(generated.s._plan) == 4
    mb, bb = builtin(old, cand)
    mg, bg = generated(old, cand)
    assert mb.tobytes() == mg.tobytes() and np.array_equal(mg, want)
    assert bb.tobytes() == bg.tobytes() and np.array_equal(bg, M.cell_bounds(old))


@gpu
def test_nothing_watched_and_one_variable():
    N, nc = 3, (3, 2)
    shape = nc + (N, N)
    rng = np.random.default_rng(8)
    # two species, admissible = [q0], dmp = (): positivity of q0 and finiteness only
    det = _Detector(reaction_lim(), 2, N, nc)
    assert det.s.lib.exa_lim_bounds_count(det.s._plan) == 0
    old = np.stack([1.0 + 0.1 * rng.random(shape), -0.5 + 0.1 * rng.random(shape)], axis=-1)       # q1 < 0 is nobody's business
    cand = old.copy()
    cand[(0, 0) + (1, 1) + (0,)] = -1e-3                              # q0 <= floor
    cand[(1, 1) + (2, 0) + (1,)] = np.nan
    cand[(2, 0) + (0, 2) + (0,)] = 50.0                               # far beyond any maximum principle: nothing is watched
    cand[(2, 1) + (0, 0) + (1,)] = -70.0
    _check(det, old, cand, lambda q: [q[..., 0]], (), _only(nc, (0, 0), (1, 1)), label="dmp = ()")
    # one variable, dmp = (0,), no expression: finiteness and the maximum principle only -- a sign means nothing
    det = _Detector(advection_one(), 2, N, nc)
    assert det.s.lib.exa_lim_bounds_count(det.s._plan) == 2
    old = (np.sin(2 * np.pi * np.linspace(0, 1, int(np.prod(shape)), endpoint=False)).reshape(shape) + 0.01 * rng.random(shape))[..., None]
    cand = old + 1e-6
    b = R.cell_bounds(old, (0,))
    lo, hi = R.neighbourhood(b)
    cand[(0, 1) + (1, 2) + (0,)] = hi[0, 1, 0] + 0.01
    cand[(2, 0) + (2, 2) + (0,)] = lo[2, 0, 0] - 0.01
    cand[(1, 0) + (0, 0) + (0,)] = np.inf
    want = _check(det, old, cand, None, (0,), _only(nc, (0, 1), (2, 0), (1, 0)), label="one variable")
    assert (old < 0).any() and not want.all()


def _free_port():
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        return so.getsockname()[1]


def _run_ranks(tmp_path, text, world, timeout=600):
    script = tmp_path / "worker.py"
    script.write_text(text)
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:                                   # exactly the processes started here
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, o[-3000:])


DETECT_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch, torch.distributed as dist
from exahype_amd import solvers as exa
from tests import limiter_admissible_ref as R
from tests.test_limiter_admissible import swe_lim, MARGIN
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
dim, N, nc, pdims = 2, %(N)d, %(nc)r, %(pdims)r
part = exa.CartesianPartition(world, rank, dim, pdims)
Gr = tuple(nc[a] * part.pdims[a] for a in range(dim))
rng = np.random.default_rng(31)
shape = Gr + (N, N)
old = np.zeros(shape + (3,))
old[..., 0] = rng.uniform(0.5, 2.0, Gr + (1, 1)) + 0.01 * rng.random(shape)      # a level per cell: the neighbours' bounds matter
lo_x, hi_x = nc[0] - 1, nc[0]                                                     # the layers either side of the block face
old[lo_x, ..., 0] = 0.2 + 0.01 * rng.random(shape[1:])
old[hi_x, ..., 0] = 3.0 + 0.01 * rng.random(shape[1:])
old[..., 1] = 0.2 * old[..., 0]
old[..., 2] = -0.3 * old[..., 0]
cand = old.copy()
cand[..., 0] += rng.choice([0.0, 1e-5, 0.02], size=Gr).reshape(Gr + (1, 1)) * rng.uniform(-1, 1, shape)
cand[lo_x], cand[hi_x] = old[lo_x], old[hi_x]
# at the block face: values only the OTHER block's bounds allow (2.5 next to the layer of 3, 0.3 next to the layer of 0.2) ...
cand[lo_x, :, 0, 0, 0] = 2.5
cand[hi_x, :, N - 1, N - 1, 0] = 0.3
# ... and a defect on either side of it that nothing allows
cand[lo_x, 0, 1, 1, 0] = 10.0
cand[hi_x, 1, 1, 1, 0] = 0.01
R.reset_margin()
want, margin = R.detect(cand, R.cell_bounds(old, (0,)), R.swe_admissible, (0,))
assert R.smallest_margin() >= MARGIN, R.smallest_margin()
expect = np.zeros(Gr[1], dtype=bool)
expect[0] = True
assert np.array_equal(want[lo_x], expect) and np.array_equal(want[hi_x], np.roll(expect, 1)) and not want.all()
s = exa.AderDgSolver(dim, N, nc, pde=swe_lim().register(), n_vars=3, dx=[1.0 / Gr[0]] * dim, part=part, backend_is_gloo=True)
lim = exa.SubcellLimiter(s, capacity=4)
sl = tuple(slice(part.coords[a] * nc[a], (part.coords[a] + 1) * nc[a]) for a in range(dim))
s.upload(cand[sl])
got = lim.detect_candidate(old[sl]).cpu().numpy()
assert lim.hx_bounds is not None and lim._bounds.shape[1] == 2
assert np.array_equal(got, want[sl]), (rank, np.argwhere(got != want[sl]))
# the block alone, periodic in itself, decides differently: the exchange is what the comparison saw
alone, _ = R.detect(cand[sl], R.cell_bounds(old[sl], (0,)), R.swe_admissible, (0,))
differs = int((alone != want[sl]).sum())
print("rank", rank, "troubled", int(got.sum()), "of", got.size, "differs from the block alone in", differs, "cells")
assert differs >= 2, (rank, differs)
dist.barrier(); dist.destroy_process_group()
'''


@gpu
def test_shallow_water_detector_on_two_ranks(tmp_path):
    swe_lim().build()                                                # once, before the ranks start
    _run_ranks(tmp_path, DETECT_WORKER % dict(root=ROOT, N=4, nc=(2, 3), pdims=[2, 1]), 2)


@gpu
@pytest.mark.parametrize("N", [4, 6])
def test_double_dam_break_through_run(N):
    """Periodic double dam break (h = 1 | 0.1 | 1, g = 9.81) on 16 x 1 cells to t = 0.05, CFL 0.4, against the restatement's committed values"""
    import torch
    from exahype_amd import solvers as exa
    nx = 16
    want = _golden()["dim2_N%d_nx%d" % (N, nx)]
    s = exa.AderDgSolver(2, N, (nx, 1), pde=swe_lim().register(), n_vars=3, dx=[1.0 / nx] * 2)
    lim = exa.SubcellLimiter(s, capacity=16)                         # an overflow fails the run
    ops = s.operators()
    u0 = R.dam_initial(N, nx)
    s.upload(u0)
    worst = []
    steps = lim.run(want["t_end"], cfl=want["cfl"], track=True,
                    monitor=lambda l, k, c: worst.append(torch.minimum(l.s.u[..., 0].min(), l.stats["min_admissible"][0])))
    torch.cuda.synchronize()
    st = lim.stats
    assert set(st) == {"min_admissible", "max_troubled", "finite"} and st["min_admissible"].shape == (1,)
    u = lim.download()
    change = R.depth_change(u, u0, ops["w"])
    print("N %d: steps %d (restatement %d) change %.8f (%.8f) min h %.6f (%.6f) troubled <= %d (%d)"
          % (N, steps, want["steps"], change, want["change"], st["min_admissible"][0].item(), want["min_h"], st["max_troubled"].item(),
             want["max_troubled"]))
    assert bool(st["finite"]) and np.isfinite(u).all()
    assert st["min_admissible"][0].item() > 0                         # the running minimum: every step, every node
    assert torch.stack(worst).min().item() > 0 and len(worst) == steps
    assert abs(s.time - want["t_end"]) < 1e-12
    assert abs(steps - want["steps"]) <= 0.01 * want["steps"]
    assert abs(change - want["change"]) <= 0.01 * want["change"]
    assert st["max_troubled"].item() == want["max_troubled"] and st["max_troubled"].item() < 16


@gpu
def test_defaults_unchanged_builtin_plan_and_registered_set_without_the_keywords():
    import torch
    from exahype_amd import solvers as exa
    s = exa.AderDgSolver(2, 4, (3, 2))
    assert s.lib.exa_lim_bounds_count(s._plan) == 4
    lim = exa.SubcellLimiter(s, capacity=4)
    lim._mood_setup()
    assert lim._bounds.shape == (6, 4)
    # a registered term set without the keywords keeps the Euler layout: four bounds, and one variable is still refused
    s3 = exa.AderDgSolver(2, 4, (3, 2), pde=swe().register(), n_vars=3)
    assert s3.lib.exa_lim_bounds_count(s3._plan) == 4
    from exahype_amd.pde_codegen import SympyPDE
    one = SympyPDE(1, flux=lambda q, d: [(1.0, 0.5)[d] * q[0]], max_eigenvalue=lambda q, d: sympy.Float(1.0), max_dim=2, name="advection_plain")
    s1 = exa.AderDgSolver(2, 3, (3, 2), pde=one.register(), n_vars=1)
    l1 = exa.SubcellLimiter(s1, capacity=4)
    with pytest.raises(Exception, match="n_vars >= 2"):
        l1.detect_candidate(np.ones((3, 2, 3, 3, 1)))
    # the conservative mode keeps refusing registered sets, with or without their own criterion
    sc = exa.AderDgSolver(2, 4, (3, 2), pde=swe_lim().register(), n_vars=3, dx=[0.5, 0.5], fused_single_stage=False)
    with pytest.raises(ValueError, match="built-in Euler"):
        exa.SubcellLimiter(sc, capacity=4).step_a_posteriori(1e-4, conservative=True)
    torch.cuda.synchronize()


@gpu
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dam_break_limited.py"), "16", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = r.stdout.strip().splitlines()[-1]
    vals = dict(kv.split("=") for kv in line.split())
    want = _golden()["dim2_N4_nx16"]
    assert abs(int(vals["steps"]) - want["steps"]) <= 0.01 * want["steps"] and float(vals["min_h"]) > 0 and int(vals["max_troubled"]) == want["max_troubled"]

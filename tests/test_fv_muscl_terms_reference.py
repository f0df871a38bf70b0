"""CPU checks of the MUSCL-Hancock update with a source and a non-conservative product (no GPU):

  * the separately written fp64 form (tests/fv_muscl_terms_ref.fp64_block) is inside the restatement's rounding bound on every row and family of
    tests/fv_muscl_terms_cases.py -- the bound is not too tight for the arithmetic the kernels use;
  * every mutant (one change of a new term each) leaves that bound at least 100-fold on a row that carries the term it touches; a mutant that
    cannot apply to a set has a stated exemption;
  * for a set with neither term the restatement gives the values of tests/fv_muscl_ref.update_block bit for bit;
  * for a constant B = a the flux form and the ncp form agree within the sum of their bounds;
  * tests/golden/fv_muscl_terms_runs.json is what the fp64 form gives, the order of the advection-reaction wave is 1.84 within 5 %, and its
    flux form and ncp form agree to 1e-12 in L1;
  * SympyPDE(muscl_terms=True): what it takes, what it refuses, what it generates; the header's flag.
"""
import functools
import json
import os
import re

import numpy as np
import pytest

from oracle import fv_reference as R
from tests import fv_muscl_ref as M
from tests import fv_muscl_terms_cases as K
from tests import fv_muscl_terms_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fv_muscl_terms_runs.json")))


def _patch_case(row, family):
    name, dim, P, H, n_aux, n, _ = row
    Q = K.patch_state(row, family)
    dt, h = K.cfl_step(name, dim, Q.reshape(-1, Q.shape[-1]))
    return Q, dt, h


@pytest.mark.parametrize("row", K.PATCH_ROWS, ids=K.patch_id)
def test_fp64_form_is_inside_the_bound(row):
    name, dim, P, H, n_aux, n, _ = row
    m, tm = K.n_real(name), K.terms(name)
    for family in K.FAMILIES:
        Q, dt, h = _patch_case(row, family)
        ref = T.update(Q, dt, h, dim, P, H, m, n_aux, terms=tm)
        got = T.fp64_update(Q, dt, h, dim, P, H, m, n_aux, tm)
        sel = T.interior(dim, P, H)
        worst = T.ratio(got, ref, sel)
        print("%s %s: fp64 form err / bound %.3f, E / M at most %.1f" % (K.patch_id(row), family, worst, float(np.max(ref.E / ref.M))))
        assert 0.0 < worst <= 1.0, (K.patch_id(row), family, worst)
        keep = np.ones(Q.shape[1:], dtype=bool)                   # what the restatement leaves alone
        keep[sel[1:] + (slice(0, m),)] = False
        assert np.array_equal(ref.new[:, keep].astype(np.float64), Q[:, keep])


@pytest.mark.parametrize("row", K.GRID_ROWS, ids=K.grid_id)
def test_fp64_form_is_inside_the_bound_on_the_grid_rows(row):
    name, dim = row[0], row[1]
    m, tm = K.n_real(name), K.terms(name)
    for family in K.FAMILIES:
        s = K.grid_setup(row, family)
        ref = T.grid_update(s.U, s.dt, s.h, dim, m, terms=tm, conditions=s.conditions)
        got = T.fp64_grid_update(s.U, s.dt, s.h, dim, m, tm, s.conditions)
        worst = T.ratio(got, ref)
        print("%s %s: fp64 form err / bound %.3f" % (K.grid_id(row), family, worst))
        assert 0.0 < worst <= 1.0, (K.grid_id(row), family, worst)
        assert np.array_equal(ref.new[..., m:].astype(np.float64), s.U[..., m:])


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    worst, reasons, applied = {}, {}, 0
    for row in K.PATCH_ROWS:
        name, dim, P, H, n_aux, n, _ = row
        m, tm = K.n_real(name), K.terms(name)
        why = T.mutant_exemption(mutant, tm)
        if why is not None:
            reasons[name] = why
            continue
        applied += 1
        for family in K.FAMILIES:
            Q, dt, h = _patch_case(row, family)
            ref = T.update(Q, dt, h, dim, P, H, m, n_aux, terms=tm)
            mut = T.update(Q, dt, h, dim, P, H, m, n_aux, terms=tm, mutant=mutant, track=False)
            worst[name] = max(worst.get(name, 0.0), T.ratio(mut.new.astype(np.float64), ref, T.interior(dim, P, H)))
    print("mutant %s: err / bound %s%s" % (mutant, {k: "%.3g" % v for k, v in worst.items()},
                                           "".join("\n  exempt on %s: %s" % kv for kv in sorted(reasons.items()))))
    assert applied > 0 and max(worst.values()) >= 100.0, (mutant, worst)
    # the exemptions hold: on such a set the mutant changes no value of the restatement
    for name in reasons:
        row = next(r for r in K.PATCH_ROWS if r[0] == name)
        _, dim, P, H, n_aux, n, _ = row
        Q, dt, h = _patch_case(row, "benign")
        a = T.update(Q, dt, h, dim, P, H, K.n_real(name), n_aux, terms=K.terms(name), track=False).new
        b = T.update(Q, dt, h, dim, P, H, K.n_real(name), n_aux, terms=K.terms(name), mutant=mutant, track=False).new
        assert np.array_equal(a, b), (mutant, name, "the exemption's reason does not hold")


def test_every_set_carries_what_the_table_says():
    t = {name: K.terms(name) for name in K.SETS}
    assert (t[K.EG].has_source, t[K.EG].has_ncp) == (True, False)
    assert (t[K.TL].has_source, t[K.TL].has_ncp) == (False, True) and t[K.TL].ncp_sees_state(3)
    assert (t[K.CS].has_source, t[K.CS].has_ncp) == (True, True) and t[K.CS].ncp_sees_state(3)
    assert not any(x.uses_xt for x in t.values())
    # every mutant applies to at least one set
    assert all(any(T.mutant_exemption(mu, x) is None for x in t.values()) for mu in T.MUTANTS)


def test_without_the_terms_it_is_the_restatement_of_the_conservative_scheme():
    """a set with neither term: the same long-double values as tests/fv_muscl_ref.update_block, bit for bit"""
    from tests import fv_cases as K1
    from tests import fv_muscl_grid_cases as G
    from tests import fv_user_cases as KU
    rng_rows = [(2, 4, 5, R.PDE_EULER, None, K1.state("riemann", 3, 2, 4, 2, 6, 5)),
                (3, 2, 5, R.PDE_EULER, None, K1.state("benign", 2, 3, 2, 2, 5, 6)),
                (2, 5, 3, R.PDE_EULER, R.UserTerms(G.flagged("swe")), KU.state(KU.SW, "riemann", 3, 2, 5, 2, 4, 7))]
    for dim, P, m, pde, tm, Q in rng_rows:
        A = Q.astype(T.LD)
        a = M.update_block(A, 1e-2, 0.1, dim, m, pde, tm)
        b = T.update_block(A, 1e-2, 0.1, dim, m, pde, tm)
        assert a[0].dtype == np.longdouble and np.array_equal(a[0], b[0]) and not np.array_equal(a[0], A[(slice(None),) + (slice(2, -2),) * dim + (slice(0, m),)])
        assert np.all(b[2] > 0)


def test_constant_matrix_is_the_flux_form():
    """B_d = a_d and f_d = a_d q are the same scheme in exact arithmetic: on data linear along one axis the two long-double results differ by
    less than the sum of the two fp64 bounds (and far less: the references' own error)"""
    from examples import advection_reaction_fv_second_order as X
    tf, tn = R.UserTerms(X.term_set("flux")), R.UserTerms(X.term_set("ncp"))
    for axis in range(2):
        i = np.indices((9, 8))[axis].astype(np.float64)
        A = (0.3 + 0.1 * i)[None, ..., None].astype(T.LD)
        a = T.update_block(A, 0.02, 0.1, 2, 1, terms=tf)
        b = T.update_block(A, 0.02, 0.1, 2, 1, terms=tn)
        diff = np.abs(a[0] - b[0])
        assert np.all(diff <= R.U53 * (a[2] + b[2])), float(np.max(diff / (R.U53 * (a[2] + b[2]))))
        print("axis %d: the forms differ by %.3g of the summed bounds" % (axis, float(np.max(diff / (R.U53 * (a[2] + b[2]))))))
        assert not np.array_equal(a[0], A[:, 2:-2, 2:-2, :1])       # (the update did something: the wave decays)


@functools.lru_cache(maxsize=None)
def _runs():
    from examples import advection_reaction_fv_second_order as X
    out = {}
    for form in X.FORMS:
        tm = R.UserTerms(X.term_set(form))
        for N in (64, 128):
            G, exact = X.wave(N)
            Gn, steps = T.run_global(G, X.T_END, 1.0 / N, 2, tm, GOLDEN["cfl"], "muscl")
            out[form, N] = (float(np.mean(np.abs(Gn[..., 0] - exact(X.T_END)))), steps)
    return out


def test_recorded_runs():
    """the golden file is what the fp64 form gives; the order is the 1.84 of the scheme without a source, within 5 %; flux form = ncp form"""
    from examples import advection_reaction_fv_second_order as X
    g = GOLDEN
    assert (g["cfl"], g["t_end"], g["k"], tuple(g["velocity"])) == (X.CFL, X.T_END, X.K, X.A)
    runs = _runs()
    for form in X.FORMS:
        for N in (64, 128):
            l1, steps = runs[form, N]
            want = g[form]["muscl_%d" % N]
            print("%s form, %d^2: L1 %.6e in %d steps (recorded %.6e in %d)" % (form, N, l1, steps, want["l1"], want["steps"]))
            assert steps == want["steps"] and abs(l1 / want["l1"] - 1) < 1e-9, (form, N, steps, l1, want)
        order = float(np.log2(runs[form, 64][0] / runs[form, 128][0]))
        print("%s form: order %.3f (recorded %.3f; first order, recorded: %.3f)" % (form, order, g[form]["order_muscl"], g[form]["order_rusanov"]))
        assert abs(order / 1.84 - 1) < 0.05 and abs(g[form]["order_muscl"] / 1.84 - 1) < 0.05, (form, order)
        assert set(g[form]) >= {"rusanov_64", "rusanov_128", "order_rusanov"}
    for N in (64, 128):
        assert abs(runs["flux", N][0] / runs["ncp", N][0] - 1) < 1e-12, (N, runs["flux", N], runs["ncp", N])
        assert abs(g["flux"]["muscl_%d" % N]["l1"] / g["ncp"]["muscl_%d" % N]["l1"] - 1) < 1e-12


# ---- the generator's keyword -----------------------------------------------------------------------------------------------------------
def _adv(**kw):
    import sympy
    from exahype_amd.pde_codegen import SympyPDE
    return SympyPDE(1, lambda q, d: [q[0] * (1.0 + d)], lambda q, d: sympy.Float(1.0 + d), max_dim=2, **kw)


SRC = lambda q: [-q[0]]                                            # noqa: E731
NCP = lambda q, dq, d: [q[0] * dq[0]]                              # noqa: E731


def test_keyword_takes_a_source_and_an_ncp():
    pytest.importorskip("sympy")
    for kw in ({"source": SRC}, {"ncp": NCP}, {"source": SRC, "ncp": NCP}, {}):
        s = _adv(muscl_hancock=True, muscl_terms=True, **kw)
        text = s.source()
        assert "static constexpr bool HAS_MUSCL_TERMS = true;" in text and "static constexpr bool HAS_MUSCL_HANCOCK = true;" in text
        assert ("HAS_SOURCE" in text) == ("source" in kw) and ("HAS_NCP" in text) == ("ncp" in kw)
        assert s.muscl_terms and s.muscl_hancock


def test_keyword_refusals():
    sympy = pytest.importorskip("sympy")
    from exahype_amd.pde_codegen import SympyPDE
    eig = lambda q, d: sympy.Float(1.0 + d)                        # noqa: E731
    adv = lambda q, d: [q[0] * (1.0 + d)]                          # noqa: E731
    with pytest.raises(ValueError, match="position / time"):       # (x, t) stays out of the second-order update
        _adv(muscl_hancock=True, muscl_terms=True, source=lambda q, x, t: [-q[0] * x[0]])
    with pytest.raises(ValueError, match="position / time"):
        _adv(muscl_hancock=True, muscl_terms=True, ncp=lambda q, dq, x, t, d: [(1 + t) * dq[0]])
    with pytest.raises(ValueError, match="position / time"):
        SympyPDE(1, lambda q, x, t, d: [q[0] * (1.0 + x[0])], eig, max_dim=2, muscl_hancock=True, muscl_terms=True)
    with pytest.raises(ValueError, match="muscl_hancock=True"):
        _adv(muscl_terms=True, source=SRC)
    with pytest.raises(ValueError, match="muscl_hancock=True"):
        _adv(muscl_terms=True)
    with pytest.raises(TypeError):
        SympyPDE(1, adv, eig, 2, "user", None, None, None, None, None, False, True, True)          # keyword only
    # the two old refusals stay and name the way out
    with pytest.raises(ValueError, match="source") as e:
        _adv(muscl_hancock=True, source=SRC)
    assert "muscl_terms=True" in str(e.value)
    with pytest.raises(ValueError, match="non-conservative") as e:
        _adv(muscl_hancock=True, ncp=NCP)
    assert "muscl_terms=True" in str(e.value)


def test_keyword_leaves_other_term_sets_alone():
    """without the keyword: the text the generator always wrote (the flagged text minus the two markers) and a key of its own"""
    pytest.importorskip("sympy")
    hancock = ("    // the second-order MUSCL-Hancock patch update is built for this term set (exa_fv_muscl.hpp)\n"
               "    static constexpr bool HAS_MUSCL_HANCOCK = true;\n")
    for kw in ({"source": SRC}, {"ncp": NCP}, {"source": SRC, "ncp": NCP}):
        plain, flagged = _adv(**kw), _adv(muscl_hancock=True, muscl_terms=True, **kw)
        text = flagged.source()
        assert "MUSCL" not in plain.source()
        lines = text.split("\n")
        k = next(i for i, ln in enumerate(lines) if "HAS_MUSCL_TERMS" in ln)
        assert lines[k].strip() == "static constexpr bool HAS_MUSCL_TERMS = true;" and lines[k - 1].lstrip().startswith("//")
        stripped = "\n".join(lines[:k - 1] + lines[k + 1:]).replace(hancock, "")
        assert plain.source() == stripped
        assert plain.key() != flagged.key()
    # a conservative set with muscl_hancock=True alone is what it was, too
    a, b = _adv(muscl_hancock=True), _adv(muscl_hancock=True, muscl_terms=True)
    assert "HAS_MUSCL_TERMS" not in a.source() and a.source() == b.source().replace(
        "    // ... and that update takes the source / ncp above (midpoint rule in time, jump term of the predicted face states)\n"
        "    static constexpr bool HAS_MUSCL_TERMS = true;\n", "")


def test_header_declares_the_flag():
    text = open(os.path.join(ROOT, "include", "exahype_hip.h")).read()
    assert re.search(r"^#define\s+EXA_PDE_FLAG_MUSCL_TERMS\s+32\b", text, flags=re.M)
    from exahype_amd import _lib
    assert _lib.PDE_FLAG_MUSCL_TERMS == 32 and _lib.PDE_FLAG_MUSCL_HANCOCK == 16

"""CPU checks behind tests/test_dg_wide_sets.py (term sets of 4, 6, 7 and 8 variables, tests/wide_term_sets.py).

(a) oracle/aderdg_numpy.py on the lambdified ring sets in fp64 == the same in np.longdouble on operators_hp, to 1e-13 of the per-variable
    increment, for every set at a 3-D and a 2-D shape.
(b) Every row of the GPU case tables, with the oracle as `got`, sees its last Picard iteration (mutant >= 100 * DG_TOL): one step at CFL 0.9 and,
    for the rows that keep it, three steps at CFL 0.6.
(c) Which stage-A kernel the selector (dg_inst.hip stage_a_kind) gives the four sets: tests/host/stage_a_selection.cpp on their side libraries
    against tests/golden/stage_a_selection_wide.txt, and the facts the GPU tests rely on stated here one by one -- among them that the
    combinations whose streamed kernel would need more than 160 KiB of LDS have no name and no slab.  tests/test_dg_wide_sets.py launches nothing
    this test has not cleared.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import aderdg_numpy as A
from oracle.dg_operators import operators, operators_hp
from tests import wide_term_sets as W
from tests.dg_cases import n_it_of
from tests.util import DG_TOL, assert_dg_parity, dg_err

HP_TOL = 1e-13
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "stage_a_selection.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "stage_a_selection_wide.txt")


def test_ring_sets_are_what_the_tables_assume():
    for name, (nv, over_q0, with_source) in W.SETS.items():
        p = W.ring(name)
        src = p.source()
        assert p.n_vars == nv and "NV = %d" % nv in src and ("HAS_SOURCE = true" in src) == with_source and not p.uses_xt
        if over_q0:                                                        # the generator caches 1 / q_0: the streamed kernel's AXO block is in use
            naux = int(re.search(r"NAUX = (\d+)", src).group(1))
            assert naux >= 1 and naux == p.n_aux()
    # a swapped variable or direction index moves the flux
    q = 1.0 + 0.3 * np.random.default_rng(0).random((5, 8))
    f = [W.numpy_pde("ring8").flux(q, d) for d in range(3)]
    assert min(np.min(np.abs(f[a] - f[b])) for a in range(3) for b in range(a)) > 1e-3
    assert all(np.min(np.abs(f[d][:, v] - f[d][:, w])) > 1e-4 for d in range(3) for v in range(8) for w in range(v))
    assert np.array_equal(W.numpy_pde("ring8", (1, 2)).flux(q, 1)[:, [0, 2, 1]], f[1][:, :3])
    # the eigenvalue bound is one: the spectral radius of dF_d / dq stays below it at the states the tables use (1 + 0.3 * random)
    import sympy
    for name, (nv, _, _) in W.SETS.items():
        p = W.ring(name)
        qs = 1.0 + 0.3 * np.random.default_rng(nv).random((8, nv))
        for d in range(3):
            jac = sympy.lambdify(p.q, sympy.Matrix(p.flux_exprs[d]).jacobian(p.q), "numpy")
            for s in qs:
                rho = np.max(np.abs(np.linalg.eigvals(np.array(jac(*s), dtype=float))))
                assert rho <= float(W.numpy_pde(name).maxeig(s[None, :], d)[0]), (name, d, rho)


@pytest.mark.parametrize("name", sorted(W.SETS))
@pytest.mark.parametrize("dim,N,nc", [(3, 3, (2, 1, 1)), (3, 5, (1, 1, 2)), (2, 7, (1, 2))])
def test_numpy_oracle_vs_long_double_reference(name, dim, N, nc):
    u, dx, dt = W.wide_input(name, dim, N, nc)
    pde, ul = W.numpy_pde(name), u.astype(np.longdouble)
    a64 = A.step(u, dt, dx, operators(N), pde, stages=True)
    ahp = A.step(ul, dt, dx, operators_hp(N), pde, stages=True)
    assert ahp["unew"].dtype == np.longdouble and ahp["ustar"].dtype == np.longdouble
    e = [dg_err(a64["ustar"], ahp["ustar"], ul), dg_err(a64["unew"], ahp["unew"], ul)]
    e.append(dg_err(A.step(a64["unew"], dt, dx, operators(N), pde), A.step(ahp["unew"], dt, dx, operators_hp(N), pde), ul))
    e.append(dg_err(A.step_single_stage(u, dt, dx, operators(N), pde), A.step_single_stage(ul, dt, dx, operators_hp(N), pde), ul))
    print("%s dim %d N %d: fp64 against long double %s" % (name, dim, N, ["%.2e" % x for x in e]))
    assert max(e) <= HP_TOL, e


@pytest.mark.parametrize("dim,name,N,nc,n_picards,family,three", W.all_rows())
def test_wide_rows_see_the_last_iteration(dim, name, N, nc, n_picards, family, three):
    u = W.wide_input(name, dim, N, nc)[0]
    for n_picard in n_picards:
        if n_it_of(N, n_picard) == 0:
            continue
        for steps in (1, 3) if three else (1,):
            want, mut = W.want_and_mutant(name, dim, N, nc, n_picard, steps)
            if (name, dim, N, n_picard) in W.NO_MUTANT:                    # the documented exception: really under the bound, and carried by n_picard = 6
                em = dg_err(W.reference(name, dim, N, nc, N - 1, steps), want, u)
                assert mut is None and em < 100 * DG_TOL and 6 in n_picards, (name, N, em)
            else:
                e, em = assert_dg_parity(want, want, u, mut, tol=DG_TOL, what="%s %d-D N %d n_picard %d, %d step(s)" % (name, dim, N, n_picard, steps))
            print("%s %d-D N %d %s n_picard %d steps %d: mutant %.2e" % (name, dim, N, nc, n_picard, steps, em))


def test_fused_rows_move():
    """(single stage: no mutant; the rows' increments are far above rounding)"""
    for name, N, nc in W.FUSED_ROWS:
        u = W.wide_input(name, 2, N, nc)[0]
        assert np.max(np.abs(W.reference(name, 2, N, nc, 0, 3, single_stage=True) - u)) > 1e-3


def test_swapped_flux_rows_are_far_from_the_oracle():
    for name, N, nc in W.SWAP_ROWS:
        assert np.max(np.abs(W.reference(name, 3, N, nc, N, 1, swap=(1, 2)) - W.reference(name, 3, N, nc, N, 1))) > 1e-5


# ---- (c) the selector ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def selection(tmp_path_factory):
    """{(set, dim, N, n_it, variant): (name, scratch_bytes)} and the program's lines for the four sets"""
    from exahype_amd import build
    lib = os.path.dirname(build.build())
    sets = [(name, W.ring(name).build()) for name in sorted(W.SETS)]
    exe = str(tmp_path_factory.mktemp("sel") / "stage_a_selection")
    r = subprocess.run([build._hipcc(), "-x", "hip", "--offload-arch=" + build.ARCH, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", build.CSRC, SRC, "-o", exe,
                        "-L", lib, "-lexahype_hip", "-ldl", "-Wl,-rpath," + lib], capture_output=True, text=True, env=build.compiler_env())
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe] + ["%s=%s" % s for s in sets], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("ring")]
    table = {}
    for l in lines:
        m = re.match(r"(\w+) dim=(\d) N=(\d) n_it=(\d) variant=(\d) name=(.*) has_stage_ba=\d scratch_bytes=(\d+) ops_image=\d+$", l)
        if m:
            table[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)))] = (m.group(6), int(m.group(7)))
    return table, lines


def test_wide_selection_matches_the_pinned_table(selection):
    got, want = selection[1], open(GOLDEN).read().splitlines()
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not bad, "%d lines, golden %d; first differences:\n%s" % (len(got), len(want), "\n".join("got  %s\nwant %s" % b for b in bad[:5]))


def test_wide_selection_facts(selection):
    t = selection[0]
    assert len(t) == 4 * 2 * 7 * 3 * 3

    def kinds(name, dim, N, n_its=(0, 1, 3), variants=(0, 1, 2)):
        return {t[(name, dim, N, n, v)][0] for n in n_its for v in variants}

    def all_are(name, dim, N, family, **kw):
        ks = kinds(name, dim, N, **kw)
        assert all(k.startswith(family) for k in ks), (name, dim, N, ks)

    def refused(name, dim, N):
        assert kinds(name, dim, N) == {""} and all(t[(name, dim, N, n, v)][1] == 0 for n in (0, 1, 3) for v in (0, 1, 2)), (name, dim, N)

    def picard(name, dim, N, family):                                 # a Picard loop: the family; the single-stage scheme: its own kernel or the streamed one
        all_are(name, dim, N, family, n_its=(1, 3), variants=(0, 2))
        all_are(name, dim, N, W.family_of(name, dim, N, 0, family), n_its=(0,))
    # ring8, 3-D: the LDS kernel (16 cells per workgroup) at N = 2 only, the streamed kernel -- for the single-stage scheme as well -- up to N = 7, nothing at N = 8
    assert kinds("ring8", 3, 2, n_its=(1, 3)) == {"dg_stage_a_kernel<3, 2, exa::UserPDE, 16>"}
    for N in range(3, 8):
        assert kinds("ring8", 3, N) == {"dg_stage_a_stream_kernel<%d, exa::UserPDE, 1, 1>" % N} and t[("ring8", 3, N, 1, 0)][1] > 0
    refused("ring8", 3, 8)
    # ring6r, 3-D: LDS up to N = 4, streamed at N = 5, 6, 7 (no longer the register-resident kernel at N = 6: its cell image does not fit twice)
    for N in (2, 3, 4):
        picard("ring6r", 3, N, W.LDS)
    for N in (5, 6, 7):
        assert kinds("ring6r", 3, N) == {"dg_stage_a_stream_kernel<%d, exa::UserPDE, 1, 1>" % N}
    refused("ring6r", 3, 8)
    # 2-D: both are refused at N = 8 and served by the LDS kernel below
    for name in ("ring6r", "ring8"):
        refused(name, 2, 8)
        for N in range(2, 8):
            picard(name, 2, N, W.LDS)
    # ring4: the register-resident kernel at 3-D N = 6 with a Picard loop (default and variant 2), the LDS kernel as variant 1
    all_are("ring4", 3, 6, W.REG, n_its=(1, 3), variants=(0, 2))
    all_are("ring4", 3, 6, W.LDS, n_its=(1, 3), variants=(1,))
    all_are("ring4", 3, 6, W.SINGLE, n_its=(0,))
    # ... and the rows read from the program: ring4 at N = 5 the LDS kernel, at N = 7 the streamed one, at N = 8 the matrix-pipe kernel for a Picard
    # loop (streamed as variant 1 and for the single-stage scheme); ring7s the LDS kernel up to N = 3, streamed at N = 4 to 7, nothing at N = 8
    picard("ring4", 3, 5, W.LDS)
    assert kinds("ring4", 3, 7) == {"dg_stage_a_stream_kernel<7, exa::UserPDE, 1, 1>"}
    all_are("ring4", 3, 8, W.M8, n_its=(1, 3), variants=(0, 2))
    all_are("ring4", 3, 8, W.STREAM, n_its=(1, 3), variants=(1,))
    all_are("ring4", 3, 8, W.STREAM, n_its=(0,))
    for (name, N), family in W.WIDE_FAMILY.items():
        if name == "ring7s":
            picard(name, 3, N, family)
    picard("ring7s", 3, 2, W.LDS)
    for N in (4, 7):
        assert kinds("ring7s", 3, N) == {"dg_stage_a_stream_kernel<%d, exa::UserPDE, 1, 1>" % N}
    for N in range(2, 8):
        picard("ring7s", 2, N, W.LDS)
    refused("ring7s", 3, 8)
    refused("ring7s", 2, 8)
    for N in range(2, 9):
        picard("ring4", 2, N, W.LDS)
    # every row of the GPU tables names a kernel of the family it asserts, and every refusal of the tables is one here
    for dim, name, N, nc, n_picards, family, three in W.all_rows():
        for n_picard in n_picards:
            n_it = n_it_of(N, n_picard)                                  # (the selector asks only whether there is a Picard loop)
            assert t[(name, dim, N, 1 if n_it > 0 else 0, 0)][0].startswith(W.family_of(name, dim, N, n_picard, family)), (name, dim, N, n_picard)
    for name, dim, N in W.REFUSED:
        refused(name, dim, N)

"""CPU check of the measure tests/test_fv_kernels_hp.py holds the corrected FV Rusanov kernels to (no GPU).  CASES is every row of
tests/fv_cases.py: patch rows that differ in the entry alone share their inputs and make one case; every grid row is a case of its own, its
halo-less states stitched across the patches with the halo layers filled from the neighbours / the boundary states (K.patches_with_halo).

* `oracle.fv_corrected` (C, fp64, IEEE division and square root) lies within 2^-53 E_ieee of the long-double reference
  (oracle/fv_reference.py), element by element, on every case and every state family.  E_ieee is the operation count of the formula applied
  term by term -- derived in oracle/fv_reference.py's docstring: one unit of 2^-53 times |result| per fp64 operation, carried through the
  formula; its flat form is E <= C_ieee M with C_ieee = 44 (the count is laid out line by line there).  E <= 44 M is asserted here too, so
  the per-term bound is never wider than the flat one.  Nothing in it is taken from what the code under test gives.
* every mutant of the reference leaves the DEVICE bound (2^-53 E_dev: the same count with fast_rcp <= 11 ulp, fast_sqrt <= 1 ulp; E_ieee for
  the cases whose kernel runs IEEE arithmetic) by a factor of 100 on every case it applies to, in EVERY state family.  A mutant that cannot
  apply is exempt by name with its reason; EXEMPT lists every exempt (mutant, case) and test_exemptions_are_the_listed_ones holds
  oracle/fv_reference.py's mutant_exemption to exactly that list, so no exemption can appear unnoticed.  The mutants act patch by patch, so a
  case with more than MUTANT_PATCHES patches shows them on its first MUTANT_PATCHES.
* the long-double eigenvalue agrees with orc_pde_maxeig within 4 * 2^-53 relative.  (`exa.pde_eval` has no host path -- it launches
  pde_eval_kernel -- so its comparison is in the GPU module: tests/test_fv_kernels_hp.py::test_eigenvalue_vs_device_pde_eval.)
"""
import numpy as np
import pytest

import oracle
from oracle import fv_reference as R
from tests import fv_cases as K

LD = np.longdouble
C_IEEE_FLAT = 44
MUTANT_PATCHES = 64
PATCH_ROWS = [r for r in K.ROWS if not r[8].startswith("grid")]
GRID_ROWS = [r for r in K.ROWS if r[8].startswith("grid")]
# patch rows that differ in the entry alone share their inputs: one case, held to the bound of the in-place call (the widest of its entries: a
# shape whose in-place call runs the fast primitives is updated out of place by an IEEE kernel)
CASES = [(K.branch(*s, "inplace"),) + s + ("inplace",) for s in sorted({r[1:8] for r in PATCH_ROWS})] + GRID_ROWS
assert {r[1:8] for r in K.ROWS} == {c[1:8] for c in CASES}

A3 = ("no_max: the advection's eigenvalue is the same constant in every volume", "no_pressure_energy: the advection has no pressure",
      "rcp_2m40: the advection has no reciprocal")
TWO_D, ONE_PATCH = "wrong_axis: a 2-D row has no third axis", "halo_next_patch: there is no next patch"
EXEMPT = {
    "ref-2d-P4-H1-5+5-n37-euler-inplace": (TWO_D,),
    "ref-persistent-2d-P4-H1-5+5-n32805-euler-inplace": (TWO_D,),
    "staged-2d-P8-H1-5+0-n9-euler-inplace": (TWO_D,),
    "staged-2d-P8-H1-5+1-n9-adv-inplace": (TWO_D,) + A3,
    "nt1024-staged-2d-P20-H1-5+0-n3-euler-inplace": (TWO_D,),
    "cpt4-2d-P40-H1-5+0-n2-euler-inplace": (TWO_D,),
    "ref-2d-P4-H1-5+5-n15-euler-grid_periodic_5x3": (TWO_D,),
    "ref-2d-P4-H1-5+5-n7-euler-grid_dirichlet_1x7": (TWO_D,),
    "nt1024-staged-2d-P24-H1-5+3-n4-euler-grid_periodic_2x2": (TWO_D,),
    "cpt4-2d-P40-H1-5+0-n4-euler-grid_periodic_2x2": (TWO_D,),
    "slab-fitnv-3d-P13-H1-8+0-n2-adv-inplace": A3,
    "slab-fitnv-3d-P13-H1-8+1-n2-adv-inplace": A3,
    "slab-generic-3d-P15-H1-5+0-n2-adv-inplace": A3,
    "slab-generic-3d-P15-H1-5+2-n2-adv-inplace": A3,
    "slab-generic-3d-P13-H1-5+0-n6-adv-grid_periodic_2x1x3": A3,
    "slab-cache-3d-P16-H1-5+0-n1-euler-inplace": (ONE_PATCH,),
    "cpt4-3d-P16-H1-5+2-n1-euler-inplace": (ONE_PATCH,),
    "slab-cache+lds-3d-P16-H2-5+0-n1-euler-inplace": (ONE_PATCH,),
}


def test_exemptions_are_the_listed_ones():
    """mutant_exemption exempts exactly the (mutant, case) pairs of EXEMPT -- the two kinds the table's design names (no third axis in 2-D, no next
    patch of a single patch) and the three mutants that have nothing to change in the advection -- and every other pair is run"""
    got = {}
    for case in CASES:
        for mutant in R.MUTANTS:
            if R.mutant_exemption(mutant, case[1], case[6], case[7]) is not None:
                got.setdefault(K.row_id(case), set()).add(mutant)
    assert got == {k: {x.split(":")[0] for x in v} for k, v in EXEMPT.items()}
    assert {c[7] for c in CASES if any(x in A3 for x in EXEMPT.get(K.row_id(c), ()))} == {R.PDE_ADVECTION}
    assert {c[1] for c in CASES if TWO_D in EXEMPT.get(K.row_id(c), ())} == {2} and {c[6] for c in CASES if ONE_PATCH in EXEMPT.get(K.row_id(c), ())} == {1}


@pytest.mark.parametrize("case", CASES, ids=K.row_id)
@pytest.mark.parametrize("family", K.FAMILIES)
def test_c_oracle_within_ieee_bound(case, family):
    _, dim, P, H, n_real, n_aux, n, pde, entry = case
    Q = K.patches_with_halo(case, family)
    dt, h = K.cfl_step(Q, dim, pde)
    ref = R.update(Q, dt, h, dim, P, H, n_real, n_aux, pde, prim=R.IEEE)
    got = oracle.fv_corrected(Q, dt, h, dim, P, H, n_real, n_aux, n, pde)
    sel = R.interior(dim, P, H)
    worst = R.ratio(got, ref, sel)
    flat = float(np.max(ref.E / ref.M))
    print("fv_corrected %s %s: err / bound %.3f, E / M %.2f" % (K.row_id(case), family, worst, flat))
    assert worst <= 1.0, worst
    assert flat <= C_IEEE_FLAT, flat
    # halo and auxiliary values: returned untouched by both
    keep = np.ones(Q.shape, dtype=bool)
    keep[sel + (slice(0, n_real),)] = False
    assert np.array_equal(got[keep], Q[keep]) and np.array_equal(ref.new[keep].astype(np.float64), Q[keep])


@pytest.mark.parametrize("row", GRID_ROWS, ids=K.row_id)
def test_grid_form_equals_patch_form(row):
    """the global-array form == halo fill + the patch form, to the last long-double bit (the same arithmetic on the same values)"""
    _, dim, P, H, n_real, n_aux, n, pde, entry = row
    grid, dirichlet = K.grid_of(row)
    for family in K.FAMILIES:
        U = K.row_state(row, family).reshape(grid + (P,) * dim + (n_real + n_aux,))
        bnd = K.boundary_states(row, family) if dirichlet else None
        dt, h = K.cfl_step(U, dim, pde)
        a = R.grid_update(U, dt, h, dim, n_real, pde, boundary=bnd)
        b = R.update(K.patches_with_halo(row, family), dt, h, dim, P, H, n_real, n_aux, pde)
        assert np.array_equal(a.new.reshape((n,) + (P,) * dim + (-1,)), b.new[R.interior(dim, P, H)])
        assert np.array_equal(a.E.reshape(b.E.shape), b.E) and np.array_equal(a.M.reshape(b.M.shape), b.M)


@pytest.mark.parametrize("case", CASES, ids=K.row_id)
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_leaves_device_bound(case, mutant):
    _, dim, P, H, n_real, n_aux, n, pde, entry = case
    why = R.mutant_exemption(mutant, dim, n, pde)
    if why is not None:
        assert mutant in {x.split(":")[0] for x in EXEMPT[K.row_id(case)]}, (mutant, why)      # exempt by name (test_exemptions_are_the_listed_ones)
        return
    prim = K.primitives(case)
    seen = {}
    for family in K.FAMILIES:
        Q = K.patches_with_halo(case, family, min(n, MUTANT_PATCHES))
        dt, h = K.cfl_step(Q, dim, pde)
        ref = R.update(Q, dt, h, dim, P, H, n_real, n_aux, pde, prim=prim)
        mut = R.update(Q, dt, h, dim, P, H, n_real, n_aux, pde, mutant=mutant, track=False)
        seen[family] = R.ratio(mut.new, ref, R.interior(dim, P, H))
    print("mutant %s on %s: x bound %s" % (mutant, K.row_id(case), {f: "%.3g" % v for f, v in seen.items()}))
    assert min(seen.values()) >= 100.0, (mutant, seen)


def test_max_eigenvalue_vs_c_oracle():
    L = oracle.lib()
    for family in K.FAMILIES:
        q = K.state(family, 1, 2, 20, 0, 5, 31).reshape(-1, 5)
        for d in range(3):
            want = R.max_eigenvalue(q, d, R.PDE_EULER)
            got = np.array([L.orc_pde_maxeig(oracle.PDE_EULER, np.ascontiguousarray(x), d) for x in q])
            rel = np.max(np.abs(got.astype(LD) - want) / want)
            print("maxeig %s d%d: %.3f x 2^-53" % (family, d, float(rel / R.U53)))
            assert rel <= 4 * R.U53, (family, d, float(rel / R.U53))
    for d in range(3):
        assert float(R.max_eigenvalue(np.ones((3, 5)), d, R.PDE_ADVECTION)[0]) == abs(float(R.ADV_A[d]))

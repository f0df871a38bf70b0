// MUSCL-Hancock patch update (exa_fv_muscl.hpp) for a generated term set: the unit a side library carries when the term set was built with
// pde_codegen.SympyPDE(..., muscl_hancock=True) (HAS_MUSCL_HANCOCK; exa_register_pde calls the filler).  With muscl_terms=True
// (HAS_MUSCL_TERMS) the term set may carry a source and / or a non-conservative product of the state alone.
#include EXA_USER_PDE_HEADER      // struct exa::UserPDE
#include "exa_fv_muscl.hpp"

static_assert(exa::pde_has_muscl_hancock<exa::UserPDE>::value, "fv_muscl_user.hip is built for term sets generated with muscl_hancock=True");
static_assert(!exa::pde_has_xt<exa::UserPDE>::value, "MUSCL-Hancock: terms of the state alone (no position / time dependence)");
static_assert(exa::pde_has_muscl_terms<exa::UserPDE>::value || (!exa::pde_has_ncp<exa::UserPDE>::value && !exa::pde_has_source<exa::UserPDE>::value),
              "MUSCL-Hancock: a source or a non-conservative product only with HAS_MUSCL_TERMS (SympyPDE(muscl_hancock=True, muscl_terms=True))");

extern "C" int exa_user_fill_fv_muscl(exa::PdeKernels* k) {
    if (k->abi != exa::PDE_KERNELS_ABI) return exa::PDE_KERNELS_ABI;
    k->fv_muscl = exa::fv_muscl_entry<exa::UserPDE>;
    return 0;
}

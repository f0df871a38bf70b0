// The conservative DG / FV interface of the subcell limiter for a generated term set that asks for it
// (pde_codegen.SympyPDE(conservative_interface=True); exa_pde.hpp pde_has_conservative_interface).  Built by SympyPDE.build() into the term
// set's side library for such term sets only; exa_register_pde calls the filler and exa_lim_face_flux / exa_lim_interface_correct go through
// the table's slots.  The kernels are those of exa_lim_conserve.hpp with the term set's flux_rt and maxeig.
#include <cstdio>
#include <cstdlib>
#include EXA_USER_PDE_HEADER      // struct exa::UserPDE
#include "exa_lim_conserve.hpp"

static_assert(exa::pde_has_conservative_interface<exa::UserPDE>::value, "the term set does not ask for the conservative interface");
static_assert(!exa::pde_has_xt<exa::UserPDE>::value && !exa::pde_has_ncp<exa::UserPDE>::value,
              "the conservative interface serves term sets of the state alone without a non-conservative product");

extern "C" int exa_user_fill_lim_conserve(exa::PdeKernels* k) {
    if (k->abi != exa::PDE_KERNELS_ABI) return exa::PDE_KERNELS_ABI;
    exa::lim_conserve_fill<exa::UserPDE>(k);
    return 0;
}

// The conservative DG / FV interface of the subcell limiter for a generated term set that asks for it
// (pde_codegen.SympyPDE(conservative_interface=True); exa_pde.hpp pde_has_conservative_interface).  Built by SympyPDE.build() into the term
// set's side library for such term sets only; capi.cpp resolves the entries in exa_register_pde and exa_lim_face_flux /
// exa_lim_interface_correct dispatch to them.  The kernels are those of exa_lim_conserve.hpp with the term set's flux_rt and maxeig.
#include <cstdio>
#include <cstdlib>
#include EXA_USER_PDE_HEADER      // struct exa::UserPDE
#include "exa_lim_conserve.hpp"

static_assert(exa::pde_has_conservative_interface<exa::UserPDE>::value, "the term set does not ask for the conservative interface");
static_assert(!exa::pde_has_xt<exa::UserPDE>::value && !exa::pde_has_ncp<exa::UserPDE>::value,
              "the conservative interface serves term sets of the state alone without a non-conservative product");

// fvflux[slot][d*2+side][var][face node]; R: the reconstruction matrix [N][2N-1] (device)
extern "C" int exa_user_lim_face_flux(int dim, int N, const double* patch, const long* cells, long n, double* fvflux, const double* R, void* stream) {
    return exa::lim_face_flux_all<exa::UserPDE>(dim, N, patch, cells, n, fvflux, R, (hipStream_t)stream);
}

// kinds[d*2+side]: include/exahype_hip.h EXA_LIM_FACE_* (null: periodic); w, phiL, phiR (host, N entries): the lift phiL_i / w_i, phiR_i / w_i.
// One launch per (axis, side).
extern "C" int exa_user_lim_interface_correct(int dim, int N, const long* nc, double* u, const double* trace, const long* cells, long n,
                                              const unsigned char* mask, const int* kinds, const double* fvflux, double dt, const double* dx,
                                              const double* w, const double* phiL, const double* phiR, void* stream) {
    return exa::lim_interface_correct_all<exa::UserPDE>(dim, N, nc, u, trace, cells, n, mask, kinds, fvflux, dt, dx, w, phiL, phiR,
                                                        (hipStream_t)stream);
}

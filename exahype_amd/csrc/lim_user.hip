// The a-posteriori detector of the subcell limiter for a generated term set that says itself what "admissible" means and which variables the
// discrete maximum principle watches (pde_codegen.SympyPDE(admissible=..., dmp=...); exa_pde.hpp pde_has_admissible).  Built by
// SympyPDE.build() into the term set's side library for such term sets only; capi.cpp resolves the entries in exa_register_pde and
// exa_lim_snapshot / exa_lim_detect dispatch to them.  The kernels are those of exa_lim_detect.hpp with every criterion constant folded.
#include <cstdio>
#include <cstdlib>
#include EXA_USER_PDE_HEADER      // struct exa::UserPDE
#include "exa_lim_detect.hpp"

using Crit = exa::LimPdeCrit<exa::UserPDE>;

extern "C" int exa_user_lim_k_dmp() { return exa::UserPDE::K_DMP; }
extern "C" int exa_user_lim_k_adm() { return exa::UserPDE::K_ADM; }

// bounds[cell][2 K_DMP] (not touched with K_DMP = 0)
extern "C" int exa_user_lim_snapshot(int dim, int N, long ncells, const double* u, double* u_old, double* bounds, void* stream) {
    return exa::lim_snapshot_launch<Crit>(dim, N, exa::UserPDE::NV, ncells, u, u_old, bounds, (hipStream_t)stream);
}

// ghosts[d*2+side]: the neighbour block's bounds [transverse cell][2 K_DMP] where kinds[d*2+side] == EXA_LIM_FACE_GHOST
extern "C" int exa_user_lim_detect(int dim, int N, const long* nc, const double* u, const double* bounds, const double* const* ghosts,
                                   const int* kinds, double d0, double eps, double floor, unsigned char* mask, void* stream) {
    exa::LimGhosts gb{};
    for (int f = 0; f < 2 * dim; f++) gb.layer[f] = ghosts ? ghosts[f] : nullptr;
    return exa::lim_detect_launch<Crit>(dim, N, exa::UserPDE::NV, nc, u, bounds, &gb, kinds, d0, eps, floor, mask, (hipStream_t)stream);
}

// The a-posteriori detector of the subcell limiter for a generated term set that says itself what "admissible" means and which variables the
// discrete maximum principle watches (pde_codegen.SympyPDE(admissible=..., dmp=...); exa_pde.hpp pde_has_admissible).  Built by
// SympyPDE.build() into the term set's side library for such term sets only; exa_register_pde calls the filler and exa_lim_snapshot /
// exa_lim_detect go through the table's slots.  The kernels are those of exa_lim_detect.hpp with every criterion constant folded.
#include <cstdio>
#include <cstdlib>
#include EXA_USER_PDE_HEADER      // struct exa::UserPDE
#include "exa_lim_detect.hpp"

using Crit = exa::LimPdeCrit<exa::UserPDE>;

// bounds[cell][2 K_DMP] (not touched with K_DMP = 0)
static int lim_snapshot(int dim, int N, long ncells, const double* u, double* u_old, double* bounds, hipStream_t s) {
    return exa::lim_snapshot_launch<Crit>(dim, N, exa::UserPDE::NV, ncells, u, u_old, bounds, s);
}

// ghosts->layer[d*2+side]: the neighbour block's bounds [transverse cell][2 K_DMP] where kinds[d*2+side] == EXA_LIM_FACE_GHOST
static int lim_detect(int dim, int N, const long* nc, const double* u, const double* bounds, const exa::LimGhosts* ghosts, const int* kinds, double d0,
                      double eps, double floor, unsigned char* mask, hipStream_t s) {
    return exa::lim_detect_launch<Crit>(dim, N, exa::UserPDE::NV, nc, u, bounds, ghosts, kinds, d0, eps, floor, mask, s);
}

extern "C" int exa_user_fill_lim(exa::PdeKernels* k) {
    if (k->abi != exa::PDE_KERNELS_ABI) return exa::PDE_KERNELS_ABI;
    k->k_dmp = exa::UserPDE::K_DMP;
    k->lim_snapshot = lim_snapshot;
    k->lim_detect = lim_detect;
    return 0;
}

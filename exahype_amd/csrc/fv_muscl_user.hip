// MUSCL-Hancock patch update (exa_fv_muscl.hpp) for a generated term set: the unit a side library carries when the term set was built with
// pde_codegen.SympyPDE(..., muscl_hancock=True) (HAS_MUSCL_HANCOCK; exa_register_pde resolves exa_user_fv_muscl_launch).  With muscl_terms=True
// (HAS_MUSCL_TERMS) the term set may carry a source and / or a non-conservative product of the state alone.
#include EXA_USER_PDE_HEADER      // struct exa::UserPDE
#include "exa_fv_muscl.hpp"

static_assert(exa::pde_has_muscl_hancock<exa::UserPDE>::value, "fv_muscl_user.hip is built for term sets generated with muscl_hancock=True");
static_assert(!exa::pde_has_xt<exa::UserPDE>::value, "MUSCL-Hancock: terms of the state alone (no position / time dependence)");
static_assert(exa::pde_has_muscl_terms<exa::UserPDE>::value || (!exa::pde_has_ncp<exa::UserPDE>::value && !exa::pde_has_source<exa::UserPDE>::value),
              "MUSCL-Hancock: a source or a non-conservative product only with HAS_MUSCL_TERMS (SympyPDE(muscl_hancock=True, muscl_terms=True))");

extern "C" int exa_user_fv_muscl_launch(int dim, int P, int H, int n_real, int n_aux, long n_patches, double* Q, double dt, double h, const long* slot,
                                        void* stream, double* out) {
    using namespace exa;
    const int V = n_real + n_aux;
    if (n_real > FVM_MAXV || n_real < UserPDE::NV) { set_error("user PDE evolves %d variables; n_real = %d", UserPDE::NV, n_real); return -1; }
    if (dim == 2) return fv_muscl_run<2, UserPDE>(P, H, n_real, V, n_patches, Q, dt, h, slot, (hipStream_t)stream, out);
    if constexpr (UserPDE::MAXDIM >= 3) {
        if (dim == 3) return fv_muscl_run<3, UserPDE>(P, H, n_real, V, n_patches, Q, dt, h, slot, (hipStream_t)stream, out);
    }
    set_error("user PDE: no MUSCL-Hancock kernel for dim %d", dim);
    return -1;
}

// the plane-streaming form of the 3-D update (a plan of exa_fv_plan_create_streamed that is_streamed).  A side library built before this entry
// existed lacks it: exa_register_pde still takes such a library, exa_fv_plan_create_streamed refuses a streamed plan of its term set until it is rebuilt
extern "C" int exa_user_fv_muscl_stream_launch(int P, int H, int n_real, int n_aux, long n_patches, double* Q, double dt, double h, const long* slot,
                                               void* stream, double* out) {
    using namespace exa;
    const int V = n_real + n_aux;
    if (n_real > FVM_MAXV || n_real < UserPDE::NV) { set_error("user PDE evolves %d variables; n_real = %d", UserPDE::NV, n_real); return -1; }
    if constexpr (UserPDE::MAXDIM >= 3) return fv_muscl_stream_run<UserPDE>(P, H, n_real, V, n_patches, Q, dt, h, slot, (hipStream_t)stream, out);
    set_error("user PDE: no streamed MUSCL-Hancock kernel (the term set is 2-D)");
    return -1;
}

// the grid step on halo-less arrays (exa_fv_grid_step_muscl_device); grid: exa::FvMusclGrid.  A side library built before this entry existed
// lacks it: exa_register_pde still takes such a library, the grid step refuses its term set until it is rebuilt
extern "C" int exa_user_fv_muscl_grid_launch(int dim, int P, int n_real, int n_aux, long n_patches, const double* Q, double* out, double dt, double h,
                                             const void* grid, void* stream) {
    using namespace exa;
    const int V = n_real + n_aux;
    if (!grid) { set_error("user PDE: MUSCL-Hancock grid step without a grid"); return -1; }
    if (n_real > FVM_MAXV || n_real < UserPDE::NV) { set_error("user PDE evolves %d variables; n_real = %d", UserPDE::NV, n_real); return -1; }
    const FvMusclGrid& ga = *static_cast<const FvMusclGrid*>(grid);
    if (dim == 2) return fv_muscl_grid_run<2, UserPDE>(P, n_real, V, n_patches, Q, out, dt, h, ga, (hipStream_t)stream);
    if constexpr (UserPDE::MAXDIM >= 3) {
        if (dim == 3) return fv_muscl_grid_run<3, UserPDE>(P, n_real, V, n_patches, Q, out, dt, h, ga, (hipStream_t)stream);
    }
    set_error("user PDE: no MUSCL-Hancock grid kernel for dim %d", dim);
    return -1;
}

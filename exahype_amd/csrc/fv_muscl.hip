// MUSCL-Hancock patch update (exa_fv_muscl.hpp) for the built-in term sets: Euler and the advection, 2-D and 3-D.  EulerRef2D is the reference's
// quirk set (F[4] is never written): exa_fv_plan_create refuses it in this mode.  The plane-streaming form (fv_muscl_stream_kernel) is 3-D only.
#include "exa_fv_muscl.hpp"

namespace exa {

int fv_muscl_launch(int dim, int P, int H, int n_real, int n_aux, long n_patches, int pde, double* Q, double dt, double h, const long* slot,
                    hipStream_t s, double* out) {
    const int V = n_real + n_aux;
    if (pde >= 100) return user_fv_muscl_launch(pde, dim, P, H, n_real, n_aux, n_patches, Q, dt, h, slot, s, out);
    if (dim == 2) {
        if (pde == 1) return fv_muscl_run<2, Euler>(P, H, n_real, V, n_patches, Q, dt, h, slot, s, out);
        if (pde == 2) return fv_muscl_run<2, Advection<FVM_MAXV>>(P, H, n_real, V, n_patches, Q, dt, h, slot, s, out);
    } else if (dim == 3) {
        if (pde == 1) return fv_muscl_run<3, Euler>(P, H, n_real, V, n_patches, Q, dt, h, slot, s, out);
        if (pde == 2) return fv_muscl_run<3, Advection<FVM_MAXV>>(P, H, n_real, V, n_patches, Q, dt, h, slot, s, out);
    }
    set_error("MUSCL-Hancock: no kernel for dim %d, pde %d", dim, pde);
    return -1;
}

int fv_muscl_stream_launch(int P, int H, int n_real, int n_aux, long n_patches, int pde, double* Q, double dt, double h, const long* slot, hipStream_t s,
                           double* out) {
    const int V = n_real + n_aux;
    if (pde >= 100) return user_fv_muscl_stream_launch(pde, P, H, n_real, n_aux, n_patches, Q, dt, h, slot, s, out);
    if (pde == 1) return fv_muscl_stream_run<Euler>(P, H, n_real, V, n_patches, Q, dt, h, slot, s, out);
    if (pde == 2) return fv_muscl_stream_run<Advection<FVM_MAXV>>(P, H, n_real, V, n_patches, Q, dt, h, slot, s, out);
    set_error("MUSCL-Hancock (streamed): no kernel for pde %d", pde);
    return -1;
}

int fv_muscl_grid_launch(int dim, int P, int n_real, int n_aux, long n_patches, int pde, const double* Q, double* out, double dt, double h,
                         const FvMusclGrid* grid, hipStream_t s) {
    const int V = n_real + n_aux;
    if (!grid) { set_error("MUSCL-Hancock grid step: no grid"); return -1; }
    if (pde >= 100) return user_fv_muscl_grid_launch(pde, dim, P, n_real, n_aux, n_patches, Q, out, dt, h, grid, s);
    if (dim == 2) {
        if (pde == 1) return fv_muscl_grid_run<2, Euler>(P, n_real, V, n_patches, Q, out, dt, h, *grid, s);
        if (pde == 2) return fv_muscl_grid_run<2, Advection<FVM_MAXV>>(P, n_real, V, n_patches, Q, out, dt, h, *grid, s);
    } else if (dim == 3) {
        if (pde == 1) return fv_muscl_grid_run<3, Euler>(P, n_real, V, n_patches, Q, out, dt, h, *grid, s);
        if (pde == 2) return fv_muscl_grid_run<3, Advection<FVM_MAXV>>(P, n_real, V, n_patches, Q, out, dt, h, *grid, s);
    }
    set_error("MUSCL-Hancock grid step: no kernel for dim %d, pde %d", dim, pde);
    return -1;
}

}  // namespace exa

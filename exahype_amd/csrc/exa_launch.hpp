// Host-side glue between the C-ABI (capi.cpp) and the per-(dim, pde) kernel
// instantiation units (dg_inst.hip, fv_rusanov.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "exa_dg_common.hpp"

namespace exa {

// reference-element tables for any N <= MAXN (host copy held by the plan)
struct DgOpsHost {
    int N;
    double xi[MAXN], w[MAXN], D[MAXN * MAXN], Kxi[MAXN * MAXN], phiL[MAXN], phiR[MAXN], iK1[MAXN * MAXN],
        K1[MAXN * MAXN];
    void* dev;     // DgOps<N> image in HBM (read by the kernels through the constant address space)
    void* lim;     // limiter tables in HBM: P[Ns][N] then R[N][Ns] (null until first use)
    void* scratch; // per-workgroup slabs of the level-streamed stage A (N whose cell image exceeds LDS), else null
    int stage_a_reserve;   // workgroups the persistent stage-A grids stay below the resident count (CUs left to the exchange's kernels)
    int stage_a_variant;   // 0: the build's default; 1: LDS-resident space-time image; 2: register-resident iterate (where built: 3-D, N = 6)
    double origin[3];      // physical coordinates of the block's origin and the time at the start of the step: what term sets with
    double time;           // position- / time-dependent terms (HAS_XT) are evaluated at (exa_dg_plan_set_origin_time; default 0)
};
// dg_operators_host.cpp: Gauss-Legendre nodes by Newton, barycentric derivative
// matrix, K1 inverse by Gauss-Jordan, all in long double.
int build_dg_operators(int N, DgOpsHost* out);
int build_limiter_operators(const DgOpsHost* o, int Ns, double* P, double* R);     // P[Ns][N], R[N][Ns]
// limiter.hip
struct LimGhosts { const double* layer[6]; };   // [d*2+side]: neighbour block's subcell layer at that block face, or null
int limiter_project(int dim, int N, int Ns, int nv, const long* nc, const double* u, const long* cells, long n, double* patch,
                    const double* Pdev, const LimGhosts* ghosts, hipStream_t s);
int limiter_face_layers(int dim, int N, int Ns, int nv, const long* nc, const double* u, int a, int side, const double* need,
                        double* out, const double* Pdev, hipStream_t s);
int limiter_reconstruct(int dim, int N, int Ns, int nv, const double* patch, const long* cells, long n, double* u,
                        const double* Rdev, int halo, hipStream_t s);        // halo: the patches', 1 | 2
// patches with halo 2 (the second-order patch update): face halos two layers deep, edge entries from the diagonal cells; kinds (host, null: all
// periodic) / data (device, [2 dim][nv]): FV_FACE_* of the domain faces and their signs / states
int limiter_project_halo2(int dim, int N, int nv, const long* nc, const double* u, const long* cells, long n, double* patch,
                          const double* Pdev, const int* kinds, const double* data, hipStream_t s);
// a-posteriori detection: u^n -> u_old (may be null) + bounds[cell][4]; candidate + bounds (+ neighbour blocks' bounds) -> mask bytes
int limiter_snapshot(int dim, int N, int nv, long ncells, const double* u, double* u_old, double* bounds, hipStream_t s);
int limiter_detect(int dim, int N, int nv, const long* nc, const double* u, const double* bounds, const LimGhosts* ghosts, const int* kinds,
                   double d0, double eps, double floor, unsigned char* mask, hipStream_t s);

struct StageBBox {
    long nc[3], lo[3], nb[3];
    const double* ghost[6];
    double* lam = nullptr;      // not null: the CFL scan of the corrected u rides in the launch (exa_dg_riemann_corrector_cfl); the caller zeroes it
};

struct DgLaunchTable {
    int nv;        // variables the PDE evolves
    int max_n;     // largest N instantiated
    int (*stage_a)(int N, const double* u_in, double* u_out, double* trace, long ncells, const CellBox* box, double dt,
                   const double* idx, int n_it, const DgOpsHost* ops, hipStream_t s);
    int (*stage_b)(int N, double* u, const double* trace, const StageBBox* box, long ncells, double dt,
                   const double* idx, const DgOpsHost* ops, hipStream_t s);
    int (*maxeig)(const double* u, long nnodes, double* out, hipStream_t s);
    size_t (*ops_image)(int N, const DgOpsHost* h, void* dst);   // dst == nullptr: size only
    size_t (*scratch_bytes)(int N);                               // 0: the LDS kernel serves this N
    const char* (*stage_a_name)(int N, int n_it, int variant);    // the kernel stage_a launches for these settings (profiles, bench line)
    // the step as ONE kernel: Riemann + corrector of the previous step (traces trace_in, time step dt_prev) in front of the predictor of
    // this one (traces -> trace_out, a second array); u holds u* before and after.  u_plain: where the corrected u goes too, or null
    int (*stage_ba)(int N, double* u, const double* trace_in, double* trace_out, long ncells, const CellBox* box, const double* const* ghost,
                    double dt_prev, double dt, const double* idx, int n_it, const DgOpsHost* ops, double* u_plain, hipStream_t s);
    int (*has_stage_ba)(int N, int n_it, int variant);
    // fused single-stage periodic step u_in -> u_out (2-D, n_picard = 0; exa_dg_fused.hpp), or nullptr
    int (*fused_single)(int N, const double* u_in, double* u_out, const long* nc, double dt, const double* idx,
                        const DgOpsHost* ops, hipStream_t s);
    // ghost[d*2+side] from a domain boundary condition (exa_dg_boundary.hpp; capi.cpp exa_dg_boundary_ghost): kind EXA_BC_OUTFLOW / _WALL
    // scale the block's own outward trace at that face by coeff[2 nv]; EXA_BC_DIRICHLET averages states[t][y][N][nv] over the Gauss time
    // levels (states null: the constant state coeff[nv]) and folds their largest eigenvalue into lam (if not null)
    int (*boundary)(int N, const double* trace, long ncells, const long* nc, int d, int side, int kind, const double* coeff, const double* states,
                    double dt, const DgOpsHost* ops, const double* idx, double* ghost, double* lam, hipStream_t s);
};
// returns nullptr when (dim, pde) is not built
const DgLaunchTable* dg_launch_table(int dim, int pde);

// One FV launch, for the built-in and the generated term sets alike (PdeKernels::fv, ::fv_muscl).
// slot: nullptr, or one entry per patch (< 0: patch not in use, left untouched)
// out != nullptr: out of place (QOut halo-less, [patch][P^dim][n_real + n_aux]); centre: [patch][dim] cell centres or nullptr; t: time
// grid != nullptr: the GRID step -- the patches are the cells of a Cartesian grid g[0] x g[1] (x g[2]) (row-major), Q and out are halo-less, halo
// states are taken from the neighbours' interiors (periodic wrap), results go to out (layout of Q).  bstate == null: every domain face is periodic;
// else the face (axis, side) is of kind bkind[axis * 2 + side] with its V doubles of data in bstate[(axis * 2 + side) * V ..]: EXA_FV_FACE_PERIODIC
// (data unused), _STATE (the prescribed state beyond the face) or _MIRROR (the patch's own interior layers reflected at the face, every variable
// times its sign); lam (optional): receives the largest eigenvalue of the NEW interior states (zeroed by the launcher on the stream)
constexpr int FV_FACE_PERIODIC = 0, FV_FACE_STATE = 1, FV_FACE_MIRROR = 2;
struct FvGrid {            // (an argument of fv_muscl_grid_kernel: the layout stays)
    int g[3];
    int bkind[6];
    const double* bstate;
    double* lam;
};
// forms of the MUSCL-Hancock update: the whole window resident in LDS, the 3-D window walked plane by plane (a plan of
// exa_fv_plan_create_streamed that is_streamed), the grid step on halo-less arrays (exa_fv_grid_step_muscl_device)
constexpr int FV_FORM_RESIDENT = 0, FV_FORM_STREAMED = 1, FV_FORM_GRID = 2;
struct FvLaunch {
    int mode, form;        // EXA_FV_*; FV_FORM_* (EXA_FV_MUSCL_HANCOCK only)
    int dim, P, H, n_real, n_aux;
    long n_patches;
    double* Q;             // (only read where out is given)
    double* out;
    const long* slot;
    double dt, h;
    const double* centre;
    double t;
    const FvGrid* grid;
    hipStream_t stream;
};

// Everything a term set brings, built-in (ids 0 .. 2) or generated (ids >= 100, exa_register_pde): a slot is null where the set has no such unit.
// pde_kernels() is the one lookup; the plans hold the pointer.  A side library fills its table through one extern "C" filler per unit it was built
// with (the list `fillers` in exa_register_pde); a filler leaves a table of another PDE_KERNELS_ABI alone and returns non-zero.
constexpr int PDE_KERNELS_ABI = 1;
struct PdeKernels {
    int abi;               // PDE_KERNELS_ABI of whoever filled the table
    int nv;                // variables the set evolves (the fewest an FV patch of it carries)
    int flags;             // EXA_PDE_FLAG_*
    int max_dim;           // dimensions the set's terms are written for.  Informational: no entry reads it -- a plan's creation does not refuse a 2-D
                           // set in 3-D, the slots do at the call (fv_run, fv_maxeig_run, fv_muscl_entry), as before the table existed
    int k_dmp;             // variables the limiter's discrete maximum principle watches: bounds[cell][2 k_dmp]
    const DgLaunchTable* dg[4];                                    // [dim], null: not built
    // fv_rusanov.hip: EXA_FV_FAITHFUL / EXA_FV_RUSANOV update; CFL scan -- max over the INTERIOR volumes of all patches and the directions of the
    // largest eigenvalue -> lam[0] (device); flux F / eigenvalue lam of n states (X: [n][3] positions for term sets of (x, t), or null)
    int (*fv)(const FvLaunch& a);
    int (*fv_maxeig)(int dim, int P, int H, int V, long n_patches, const double* Q, double* lam, const double* centre, double t, double h, hipStream_t s);
    int (*pde_eval)(int normal, long n, int stride, const double* Q, double* F, double* lam, const double* X, double t, hipStream_t s);
    // fv_muscl.hip / fv_muscl_user.hip: the EXA_FV_MUSCL_HANCOCK update in a.form
    int (*fv_muscl)(const FvLaunch& a);
    // lim_user.hip: the set's own a-posteriori criterion -- u^n -> u_old (may be null) + bounds; candidate + bounds (+ neighbour blocks' bounds) -> mask
    // bytes.  Null: the Euler-layout criterion of limiter.hip (limiter_snapshot / limiter_detect)
    int (*lim_snapshot)(int dim, int N, long ncells, const double* u, double* u_old, double* bounds, hipStream_t s);
    int (*lim_detect)(int dim, int N, const long* nc, const double* u, const double* bounds, const LimGhosts* ghosts, const int* kinds, double d0,
                      double eps, double floor, unsigned char* mask, hipStream_t s);
    // limiter.hip / lim_conserve_user.hip, the conservative DG / FV interface: FV face fluxes of the listed patches at the DG face nodes,
    // fvflux[slot][d*2+side][var][node]; their lift into the untroubled (mask == 0) face neighbours of the listed cells, one launch per (axis, side)
    int (*lim_face_flux)(int dim, int N, const double* patch, const long* cells, long n, double* fvflux, const double* Rdev, hipStream_t s);
    int (*lim_interface_correct)(int dim, int N, const long* nc, double* u, const double* trace, const long* cells, long n, const unsigned char* mask,
                                 const int* kinds, const double* fvflux, double dt, const double* dx, const double* w, const double* phiL,
                                 const double* phiR, hipStream_t s);
};
// capi.cpp: null with "unknown pde %d" / "pde %d is not registered"
const PdeKernels* pde_kernels(int pde);
// the built-in sets' slices, tab[pde]: fv_rusanov.hip, fv_muscl.hip, limiter.hip
void fv_fill_builtin(PdeKernels* tab);
void fv_muscl_fill_builtin(PdeKernels* tab);
void limiter_fill_builtin(PdeKernels* tab);

// fv_muscl.hip (exa_fv_muscl.hpp): the second-order MUSCL-Hancock patch update, EXA_FV_MUSCL_HANCOCK.  Its LDS plan: per patch the window
// (P + 4)^dim x V and the predictor's increments (P + 2)^dim x n_real, 8 B each; patches whose plan stays within 64 KiB share a 256-thread
// workgroup (as many as have a volume per thread), a larger one has a workgroup to itself (2-D above 80 KiB: 512 threads, since only one such
// workgroup fits a CU; the 3-D kernels need more than the 256 registers a lane of a 512-thread workgroup has).  -> false: one patch does not fit (pl->lds = the bytes it needs); exa_fv_plan_create refuses such a shape.
constexpr size_t FV_MUSCL_LDS_AVAILABLE = 160 * 1024;
struct FvMusclPlan {
    int ppb, nt;
    size_t lds;
    int ring = 0;          // window planes in LDS at a time (fv_muscl_stream_plan; 0: the whole window, fv_muscl_plan)
};
inline bool fv_muscl_plan(int dim, int P, int n_real, int V, FvMusclPlan* pl) {
    const size_t T = (size_t)P + 4, D = (size_t)P + 2;
    const size_t per = ((dim == 3 ? T * T * T : T * T) * (size_t)V + (dim == 3 ? D * D * D : D * D) * (size_t)n_real) * sizeof(double);
    const size_t ncell = dim == 3 ? (size_t)P * P * P : (size_t)P * P;
    pl->ppb = 1;
    pl->lds = per;
    pl->nt = (dim == 2 && per > 80 * 1024) ? 512 : 256;
    if (per > FV_MUSCL_LDS_AVAILABLE) return false;
    if (ncell <= 256 && 2 * per <= 64 * 1024) {
        const size_t by_threads = 256 / ncell, by_lds = 64 * 1024 / per;
        pl->ppb = (int)(by_threads < by_lds ? by_threads : by_lds);
        pl->lds = per * pl->ppb;
    }
    return true;
}
// The plan of the PLANE-STREAMING form of the 3-D update (fv_muscl_stream_kernel): one workgroup per patch walks the planes of axis 0 and keeps
// `ring` window planes (P + 4)^2 x V and three predictor planes (P + 2)^2 x n_real in LDS.  Five window planes are what an interior plane reads; a
// sixth, where it fits, takes the next plane while the oldest one is still read and saves one of the three barriers per plane.  256 threads: a plane
// has at most 19^2 interior and 21^2 predictor tasks, and the arithmetic needs more registers than a lane of a 512-thread workgroup has.
// -> false: five + three planes do not fit (pl->lds = the bytes they need)
inline bool fv_muscl_stream_plan(int P, int n_real, int V, FvMusclPlan* pl) {
    const size_t T = (size_t)P + 4, D = (size_t)P + 2;
    const size_t wpl = T * T * (size_t)V, ppl = D * D * (size_t)n_real;
    const size_t five = (5 * wpl + 3 * ppl) * sizeof(double), six = five + wpl * sizeof(double);
    pl->ppb = 1;
    pl->nt = 256;
    pl->ring = 5;
    pl->lds = five;
    if (five > FV_MUSCL_LDS_AVAILABLE) return false;
    if (six <= FV_MUSCL_LDS_AVAILABLE) { pl->ring = 6; pl->lds = six; }
    return true;
}
void set_error(const char* fmt, ...);

}  // namespace exa

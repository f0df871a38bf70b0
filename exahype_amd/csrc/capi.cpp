// C-ABI of libexahype_hip.so (include/exahype_hip.h).  Host-side only: argument
// checking, plan bookkeeping, staging for the *_host convenience calls, and
// dispatch into the kernel units.  Never throws; every failure sets the
// thread-local message behind exa_last_error().
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <new>
#include <vector>
#include <dlfcn.h>
#include "../../include/exahype_hip.h"
#include "exa_launch.hpp"

namespace exa {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define EXA_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return EXA_ERR_HIP;                                                        \
        }                                                                              \
    } while (0)

const DgLaunchTable *dg_table_2_0(), *dg_table_2_1(), *dg_table_2_2(), *dg_table_3_1(), *dg_table_3_2();

// ---- the term sets: built in (ids 0 .. 2) or registered at run time (ids >= 100; side libraries generated from SymPy expressions).  Where a term
// set's kernels are found is decided here and in exa_register_pde; everything downstream holds a PdeKernels* -----------------------------------
static std::deque<PdeKernels> g_user;       // (a deque: the plans keep pointers to its entries)

const PdeKernels* pde_kernels(int pde) {
    // nv: EulerRef2D evolves (rho, rho u, rho v, E); k_dmp: the Euler-layout criterion of limiter.hip watches density and energy
    static const struct Builtin {
        PdeKernels tab[3] = {{PDE_KERNELS_ABI, 4, 0, 2, 2}, {PDE_KERNELS_ABI, 5, 0, 3, 2}, {PDE_KERNELS_ABI, 1, 0, 3, 2}};
        Builtin() {
            tab[0].dg[2] = dg_table_2_0();
            tab[1].dg[2] = dg_table_2_1(); tab[1].dg[3] = dg_table_3_1();
            tab[2].dg[2] = dg_table_2_2(); tab[2].dg[3] = dg_table_3_2();
            fv_fill_builtin(tab);
            fv_muscl_fill_builtin(tab);
            limiter_fill_builtin(tab);
        }
    } builtin;
    if (pde >= 100) {
        if (pde - 100 < (int)g_user.size()) return &g_user[pde - 100];
        set_error("pde %d is not registered", pde);
        return nullptr;
    }
    if (pde >= 0 && pde <= 2) return &builtin.tab[pde];
    set_error("unknown pde %d", pde);
    return nullptr;
}

const DgLaunchTable* dg_launch_table(int dim, int pde) {
    const PdeKernels* k = pde_kernels(pde);
    return (k && dim >= 2 && dim <= 3) ? k->dg[dim] : nullptr;
}

// A slot of a term set's table is tested through these and nowhere else: null sets the error.
template <class F> static F slot_or_error(F f, int pde, const char* what) {
    if (!f) set_error("pde %d carries no %s", pde, what);
    return f;
}
static auto fv_muscl_slot(const PdeKernels* k, int pde) -> decltype(k->fv_muscl) {
    if (k->fv_muscl) return k->fv_muscl;
    if (pde == EXA_PDE_EULER_REF2D) set_error("EXA_FV_MUSCL_HANCOCK: EULER_REF2D is the reference's quirk set (F[4] is never written); use EXA_PDE_EULER");
    else set_error("EXA_FV_MUSCL_HANCOCK: pde %d was generated without the MUSCL-Hancock kernel; build it with SympyPDE(..., muscl_hancock=True)", pde);
    return nullptr;
}

static long lpow(long b, int e) { long r = 1; while (e-- > 0) r *= b; return r; }

}  // namespace exa

using namespace exa;

struct exa_fv_plan {
    int device, mode, dim, P, H, n_real, n_aux, pde;
    long n_patches, count;
    int streamed;          // EXA_FV_MUSCL_HANCOCK, 3-D: the plane-streaming kernel serves the plan (exa_fv_plan_create_streamed)
    const PdeKernels* k;   // the term set's kernels (pde_kernels(pde) at creation)
};

struct exa_dg_plan {
    int device, dim, N, nv, pde, n_it;
    long nc[3], ncells;
    const PdeKernels* k;   // the term set's kernels (pde_kernels(pde) at creation) and ...
    const DgLaunchTable* tab;      // ... k->dg[dim]
    DgOpsHost ops;
    double idx[3];         // 1 / dx of the last stage A: where exa_dg_boundary_ghost places the face nodes of a Dirichlet datum
};

extern "C" {

int exa_version(void) { return 100; }

const char* exa_last_error(void) { return g_err; }

int exa_device_count(int* count) {
    if (!count) { set_error("exa_device_count: NULL argument"); return EXA_ERR_INVALID; }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; set_error("hipGetDeviceCount: %s", hipGetErrorString(e)); return EXA_ERR_NO_DEVICE; }
    *count = n;
    return EXA_OK;
}

static int use_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device available (%s); libexahype_hip has no CPU fallback", e == hipSuccess ? "count 0" : hipGetErrorString(e));
        return EXA_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) { set_error("device %d out of range (0..%d)", device, n - 1); return EXA_ERR_INVALID; }
    EXA_HIP(hipSetDevice(device));
    return EXA_OK;
}

int exa_register_pde(const char* library_path, int* pde_id) {
    if (!library_path || !pde_id) { set_error("exa_register_pde: NULL argument"); return EXA_ERR_INVALID; }
    void* h = dlopen(library_path, RTLD_NOW | RTLD_LOCAL);
    if (!h) { set_error("exa_register_pde: %s", dlerror()); return EXA_ERR_INVALID; }
    PdeKernels u{};
    u.abi = PDE_KERNELS_ABI;
    u.k_dmp = 2;                                                   // (without a detector unit: the Euler-layout criterion of limiter.hip)
    typedef const void* (*tab_fn)();
    for (int d = 2; d <= 3; d++) {
        char name[64];
        snprintf(name, sizeof(name), "exa_user_dg_table_%d", d);
        tab_fn f = (tab_fn)dlsym(h, name);
        u.dg[d] = f ? static_cast<const DgLaunchTable*>(f()) : nullptr;
    }
    // one filler per unit the library was built with (fv_rusanov.hip -- in every library: it brings nv, flags and max_dim --, lim_user.hip,
    // lim_conserve_user.hip, fv_muscl_user.hip); a filler built for another table layout writes nothing and returns its PDE_KERNELS_ABI
    static const char* const fillers[] = {"exa_user_fill_fv", "exa_user_fill_lim", "exa_user_fill_lim_conserve", "exa_user_fill_fv_muscl"};
    for (const char* name : fillers) {
        int (*fill)(PdeKernels*) = (int (*)(PdeKernels*))dlsym(h, name);
        const int abi = fill ? fill(&u) : 0;
        if (abi != 0) {
            dlclose(h);
            set_error("%s was built for kernel table ABI %d, this libexahype_hip has %d: rebuild the term set (SympyPDE(...).build(force=True))", library_path,
                      abi, PDE_KERNELS_ABI);
            return EXA_ERR_INVALID;
        }
    }
    const char* missing = nullptr;
    if (!u.fv) missing = "exports no exahype_amd PDE entry points (exa_user_fill_fv; a library from before the kernel table: rebuild the term set)";
    else if ((u.flags & EXA_PDE_FLAG_ADMISSIBLE) && (!u.lim_snapshot || !u.lim_detect)) missing = "carries an admissibility criterion but no detector unit (exa_user_fill_lim)";
    else if ((u.flags & EXA_PDE_FLAG_CONSERVATIVE) && (!u.lim_face_flux || !u.lim_interface_correct))
        missing = "asks for the conservative DG / FV interface but has no such unit (exa_user_fill_lim_conserve)";
    else if ((u.flags & EXA_PDE_FLAG_MUSCL_HANCOCK) && !u.fv_muscl) missing = "asks for the MUSCL-Hancock patch update but has no such unit (exa_user_fill_fv_muscl)";
    if (missing) { dlclose(h); set_error("%s %s", library_path, missing); return EXA_ERR_INVALID; }
    g_user.push_back(u);
    *pde_id = 100 + (int)g_user.size() - 1;
    return EXA_OK;
}

int exa_pde_flags(int pde) { return (pde >= 100 && pde - 100 < (int)g_user.size()) ? g_user[pde - 100].flags : 0; }

int exa_pde_eval_device(int pde, int normal, long n, int stride, const double* Q_dev, double* F_dev, double* lambda_dev,
                        void* stream) {
    return exa_pde_eval_device_at(pde, normal, n, stride, Q_dev, nullptr, 0.0, F_dev, lambda_dev, stream);
}

int exa_pde_eval_device_at(int pde, int normal, long n, int stride, const double* Q_dev, const double* x_dev, double t, double* F_dev,
                           double* lambda_dev, void* stream) {
    if (normal < 0 || normal > 2 || n < 0 || stride < 1 || !Q_dev) { set_error("exa_pde_eval_device: bad argument"); return EXA_ERR_INVALID; }
    const PdeKernels* k = pde_kernels(pde);
    if (!k) return EXA_ERR_INVALID;
    if (pde == EXA_PDE_EULER_REF2D && (normal > 1 || stride < 4)) { set_error("EULER_REF2D needs normal < 2 and stride >= 4"); return EXA_ERR_INVALID; }
    if (pde == EXA_PDE_EULER && stride < 5) { set_error("EULER needs stride >= 5"); return EXA_ERR_INVALID; }
    const auto eval = slot_or_error(k->pde_eval, pde, "flux / eigenvalue kernel");
    return eval ? eval(normal, n, stride, Q_dev, F_dev, lambda_dev, x_dev, t, (hipStream_t)stream) : EXA_ERR_INVALID;
}

/* ---- FV ---------------------------------------------------------------------- */

// both plan entries; stream_planes: EXA_FV_STREAM_* (exa_fv_plan_create: NEVER)
static int fv_plan_create(int device, int mode, int dim, int patch_size, int halo_size, int n_real, int n_aux, long n_patches, int pde, int stream_planes,
                          exa_fv_plan** plan) {
    if (!plan) { set_error("exa_fv_plan_create: NULL plan"); return EXA_ERR_INVALID; }
    *plan = nullptr;
    // same viability rule as the reference's KernelBuilder (exahype/KernelBuilder.py:41-48) ...
    if ((dim != 2 && dim != 3) || patch_size < 1 || halo_size < 0) { set_error("check viability of inputs"); return EXA_ERR_INVALID; }
    // ... plus what the 3-point stencil itself needs
    if (halo_size < 1) { set_error("the Rusanov stencil reads one halo layer: halo_size must be >= 1"); return EXA_ERR_INVALID; }
    if (mode != EXA_FV_FAITHFUL && mode != EXA_FV_RUSANOV && mode != EXA_FV_MUSCL_HANCOCK) { set_error("unknown FV mode %d", mode); return EXA_ERR_INVALID; }
    if (mode == EXA_FV_MUSCL_HANCOCK && halo_size < 2) { set_error("MUSCL-Hancock reads two halo layers: halo_size must be >= 2"); return EXA_ERR_INVALID; }
    if (stream_planes != EXA_FV_STREAM_NEVER && stream_planes != EXA_FV_STREAM_IF_NEEDED && stream_planes != EXA_FV_STREAM_ALWAYS) {
        set_error("exa_fv_plan_create_streamed: unknown stream_planes %d (EXA_FV_STREAM_NEVER / _IF_NEEDED / _ALWAYS)", stream_planes);
        return EXA_ERR_INVALID;
    }
    if (stream_planes != EXA_FV_STREAM_NEVER && mode != EXA_FV_MUSCL_HANCOCK) {
        set_error("exa_fv_plan_create_streamed: plane streaming is a form of EXA_FV_MUSCL_HANCOCK; mode %d takes stream_planes = EXA_FV_STREAM_NEVER", mode);
        return EXA_ERR_INVALID;
    }
    if (stream_planes == EXA_FV_STREAM_ALWAYS && dim != 3) {
        set_error("exa_fv_plan_create_streamed: EXA_FV_STREAM_ALWAYS in %d-D -- the plane-streaming kernel is 3-D only (every 2-D patch up to 32^2 has a "
                  "resident plan)", dim);
        return EXA_ERR_INVALID;
    }
    if (n_real < 1 || n_real > 8 || n_aux < 0 || n_patches < 0) { set_error("n_real must be 1..8, n_aux >= 0, n_patches >= 0"); return EXA_ERR_INVALID; }
    if (pde == EXA_PDE_EULER_REF2D && (dim != 2 || n_real < 4)) { set_error("EULER_REF2D is the reference's 2-D term set (n_real >= 4)"); return EXA_ERR_INVALID; }
    if (pde == EXA_PDE_EULER && n_real < 5) { set_error("EULER needs n_real >= 5"); return EXA_ERR_INVALID; }
    const PdeKernels* k = pde_kernels(pde);
    if (!k) return EXA_ERR_INVALID;
    if (n_real < k->nv) { set_error("pde %d evolves %d variables; n_real = %d", pde, k->nv, n_real); return EXA_ERR_INVALID; }
    int streamed = 0;
    if (mode == EXA_FV_MUSCL_HANCOCK) {
        if (!fv_muscl_slot(k, pde)) return EXA_ERR_INVALID;
        FvMusclPlan pl;
        const bool resident = patch_size <= 1024 && fv_muscl_plan(dim, patch_size, n_real, n_real + n_aux, &pl);
        if (patch_size > 1024) pl.lds = (size_t)-1;
        if (dim == 3 && (stream_planes == EXA_FV_STREAM_ALWAYS || (stream_planes == EXA_FV_STREAM_IF_NEEDED && !resident))) {
            FvMusclPlan ps;
            if (patch_size > 1024 || !fv_muscl_stream_plan(patch_size, n_real, n_real + n_aux, &ps)) {
                if (patch_size > 1024) ps.lds = (size_t)-1;
                set_error("EXA_FV_MUSCL_HANCOCK: a patch of %d^3 volumes with %d + %d variables needs %zu bytes of LDS with the whole window resident and "
                          "%zu bytes plane by plane (five window planes, three predictor planes), %zu bytes are available", patch_size, n_real, n_aux,
                          pl.lds, ps.lds, FV_MUSCL_LDS_AVAILABLE);
                return EXA_ERR_INVALID;
            }
            streamed = 1;
        } else if (!resident) {
            set_error("EXA_FV_MUSCL_HANCOCK: a patch of %d^%d volumes with %d + %d variables needs %zu bytes of LDS (window and predictor), %zu bytes are "
                      "available", patch_size, dim, n_real, n_aux, pl.lds, FV_MUSCL_LDS_AVAILABLE);
            return EXA_ERR_INVALID;
        }
    }
    const long ncell = lpow(patch_size, dim);
    if (mode != EXA_FV_MUSCL_HANCOCK && ncell > 4096) { set_error("FV patch with %ld volumes exceeds the 4096 a workgroup keeps in registers", ncell); return EXA_ERR_INVALID; }
    int rc = use_device(device);
    if (rc) return rc;
    exa_fv_plan* p = new (std::nothrow) exa_fv_plan;
    if (!p) { set_error("out of host memory"); return EXA_ERR_ALLOC; }
    p->device = device; p->mode = mode; p->dim = dim; p->P = patch_size; p->H = halo_size;
    p->n_real = n_real; p->n_aux = n_aux; p->pde = pde; p->n_patches = n_patches;
    p->count = n_patches * lpow(patch_size + 2 * halo_size, dim) * (n_real + n_aux);
    p->streamed = streamed;
    p->k = k;
    *plan = p;
    return EXA_OK;
}

int exa_fv_plan_create(int device, int mode, int dim, int patch_size, int halo_size, int n_real, int n_aux,
                       long n_patches, int pde, exa_fv_plan** plan) {
    return fv_plan_create(device, mode, dim, patch_size, halo_size, n_real, n_aux, n_patches, pde, EXA_FV_STREAM_NEVER, plan);
}

int exa_fv_plan_create_streamed(int device, int mode, int dim, int patch_size, int halo_size, int n_real, int n_aux, long n_patches, int pde,
                                int stream_planes, exa_fv_plan** plan) {
    return fv_plan_create(device, mode, dim, patch_size, halo_size, n_real, n_aux, n_patches, pde, stream_planes, plan);
}

int exa_fv_plan_is_streamed(const exa_fv_plan* plan) { return plan && plan->streamed ? 1 : 0; }

int exa_fv_plan_destroy(exa_fv_plan* plan) { delete plan; return EXA_OK; }

long exa_fv_q_count(const exa_fv_plan* plan) { return plan ? plan->count : 0; }

// one launch of the plan's update through the slot of its mode.  grid: the grid step (Q halo-less and only read, out the new states).  The term sets
// of EXA_FV_MUSCL_HANCOCK see the state alone: its entry reads no centres and no time
static int fv_step(const exa_fv_plan* p, double* Q, double* out, const long* slot, const double* centre, double t, double dt, double h, const FvGrid* grid,
                   void* stream) {
    const FvLaunch a{p->mode, grid ? FV_FORM_GRID : (p->streamed ? FV_FORM_STREAMED : FV_FORM_RESIDENT), p->dim, p->P, p->H, p->n_real, p->n_aux,
                     p->n_patches, Q, out, slot, dt, h, centre, t, grid, (hipStream_t)stream};
    const auto run = p->mode == EXA_FV_MUSCL_HANCOCK ? fv_muscl_slot(p->k, p->pde) : slot_or_error(p->k->fv, p->pde, "FV patch kernel");
    return run ? run(a) : EXA_ERR_INVALID;
}

int exa_fv_time_step_device_masked(exa_fv_plan* p, double* Q_dev, const long* slot_dev, double dt, double h, void* stream) {
    if (!p || (!Q_dev && p->count > 0)) { set_error("exa_fv_time_step_device: NULL argument"); return EXA_ERR_INVALID; }
    if (p->mode == EXA_FV_RUSANOV && !(h > 0.0)) { set_error("EXA_FV_RUSANOV needs the volume size h > 0"); return EXA_ERR_INVALID; }
    if (p->mode == EXA_FV_MUSCL_HANCOCK && !(h > 0.0)) { set_error("EXA_FV_MUSCL_HANCOCK needs the volume size h > 0"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    return fv_step(p, Q_dev, nullptr, slot_dev, nullptr, 0.0, dt, h, nullptr, stream);
}

int exa_fv_time_step_device_masked_at(exa_fv_plan* p, double* Q_dev, const long* slot_dev, const double* centre_dev, double t, double dt, double h,
                                      void* stream) {
    if (!p || (!Q_dev && p->count > 0)) { set_error("exa_fv_time_step_device_masked_at: NULL argument"); return EXA_ERR_INVALID; }
    if (!(h > 0.0)) { set_error("exa_fv_time_step_device_masked_at needs the volume size h > 0 (volume centres, dt / h)"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    return fv_step(p, Q_dev, nullptr, slot_dev, centre_dev, t, dt, h, nullptr, stream);
}

int exa_fv_time_step_device_oop(exa_fv_plan* p, const double* QIn_dev, double* QOut_dev, const double* centre_dev, double t, double dt,
                                double h, void* stream) {
    if (!p || ((!QIn_dev || !QOut_dev) && p->count > 0)) { set_error("exa_fv_time_step_device_oop: NULL argument"); return EXA_ERR_INVALID; }
    if (!(h > 0.0)) { set_error("exa_fv_time_step_device_oop needs the volume size h > 0 (volume centres, dt / h)"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    // (the kernel only reads QIn: the const is cast away for the argument it shares with the in-place call)
    return fv_step(p, const_cast<double*>(QIn_dev), QOut_dev, nullptr, centre_dev, t, dt, h, nullptr, stream);
}

int exa_fv_time_step_device_at(exa_fv_plan* p, double* Q_dev, const double* centre_dev, double t, double dt, double h, void* stream) {
    if (!p || (!Q_dev && p->count > 0)) { set_error("exa_fv_time_step_device_at: NULL argument"); return EXA_ERR_INVALID; }
    if (!(h > 0.0)) { set_error("exa_fv_time_step_device_at needs the volume size h > 0 (volume centres, dt / h)"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    return fv_step(p, Q_dev, nullptr, nullptr, centre_dev, t, dt, h, nullptr, stream);
}

// face_kind[2 dim] (null: every face periodic) of the entry `who` -> bkind; a face that is not periodic needs face_data_dev.  -> *bounded: there is one.
// hints: the entry's messages end in the way out (the wording exa_fv_grid_step_muscl_device has had; the older entries keep theirs)
static int check_face_kinds(const char* who, bool hints, int dim, const int* face_kind, const double* face_data_dev, int* bkind, bool* bounded) {
    *bounded = false;
    for (int f = 0; face_kind && f < 2 * dim; f++) {
        if (face_kind[f] < EXA_FV_FACE_PERIODIC || face_kind[f] > EXA_FV_FACE_MIRROR) {
            set_error("%s: face_kind[%d] = %d is none of EXA_FV_FACE_PERIODIC / _STATE / _MIRROR", who, f, face_kind[f]);
            return EXA_ERR_INVALID;
        }
        bkind[f] = face_kind[f];
        *bounded = *bounded || face_kind[f] != EXA_FV_FACE_PERIODIC;
    }
    if (*bounded && !face_data_dev) { set_error("%s: a face that is not periodic needs face_data_dev%s", who, hints ? " (its state or its signs)" : ""); return EXA_ERR_INVALID; }
    return EXA_OK;
}

// what both grid steps ask of face_kind, face_data_dev and grid[] -> *ga; who: the entry that was called (error messages)
static int fv_grid_args(const char* who, bool hints, const exa_fv_plan* p, const long* grid, const int* face_kind, const double* face_data_dev, double* lambda_next_dev,
                        FvGrid* ga) {
    *ga = FvGrid{{1, 1, 1}, {0, 0, 0, 0, 0, 0}, nullptr, lambda_next_dev};
    bool bounded;
    int rc = check_face_kinds(who, hints, p->dim, face_kind, face_data_dev, ga->bkind, &bounded);
    if (rc) return rc;
    ga->bstate = bounded ? face_data_dev : nullptr;                // (null: the kernels take every face as periodic)
    long n = 1;
    for (int a = 0; a < p->dim; a++) {
        if (grid[a] < 1 || grid[a] > 0x7fffffffL) { set_error("%s: grid[%d] = %ld", who, a, grid[a]); return EXA_ERR_INVALID; }
        ga->g[a] = (int)grid[a];
        n *= grid[a];
    }
    if (n != p->n_patches) { set_error("%s: the grid has %ld patches, the plan %ld%s", who, n, p->n_patches, hints ? ": create the plan with n_patches = the product of grid" : ""); return EXA_ERR_INVALID; }
    // (the kernels decode a patch's grid coordinates in 32-bit arithmetic: fv_grid_coords, fv_muscl_patch_coords)
    if (n > 0xffffffffL) { set_error("%s: %ld patches -- a grid holds at most 2^32 - 1", who, n); return EXA_ERR_INVALID; }
    return EXA_OK;
}

// the grid step behind both entries of the first-order modes; who: the entry that was called (error messages)
static int fv_grid_step(const char* who, exa_fv_plan* p, const double* Q_dev, double* QNext_dev, const long* grid, const int* face_kind, const double* face_data_dev,
                        const double* centre_dev, double t, double dt, double h, double* lambda_next_dev, void* stream) {
    if (!p || !grid || ((!Q_dev || !QNext_dev) && p->count > 0)) { set_error("%s: NULL argument", who); return EXA_ERR_INVALID; }
    if (p->mode == EXA_FV_MUSCL_HANCOCK) {
        set_error("%s: the one-launch grid step takes its halo states from the face neighbours only; EXA_FV_MUSCL_HANCOCK needs the edge neighbours "
                  "(diagonal patches) too -- fill the halos of the array with halo and call exa_fv_time_step_device", who);
        return EXA_ERR_INVALID;
    }
    if (Q_dev == QNext_dev) { set_error("%s: the new states need an array of their own (the neighbours read the old ones)", who); return EXA_ERR_INVALID; }
    if (p->mode == EXA_FV_RUSANOV && !(h > 0.0)) { set_error("%s: EXA_FV_RUSANOV needs the volume size h > 0", who); return EXA_ERR_INVALID; }
    FvGrid ga;
    int rc = fv_grid_args(who, false, p, grid, face_kind, face_data_dev, lambda_next_dev, &ga);
    if (rc) return rc;
    if (p->H > p->P) { set_error("%s: halo_size %d exceeds patch_size %d (the halo would reach past the face neighbour)", who, p->H, p->P); return EXA_ERR_INVALID; }
    rc = use_device(p->device);
    if (rc) return rc;
    return fv_step(p, const_cast<double*>(Q_dev), QNext_dev, nullptr, centre_dev, t, dt, h, &ga, stream);
}

int exa_fv_grid_step_device_bc(exa_fv_plan* p, const double* Q_dev, double* QNext_dev, const long* grid, const int* face_kind, const double* face_data_dev,
                               const double* centre_dev, double t, double dt, double h, double* lambda_next_dev, void* stream) {
    return fv_grid_step("exa_fv_grid_step_device_bc", p, Q_dev, QNext_dev, grid, face_kind, face_data_dev, centre_dev, t, dt, h, lambda_next_dev, stream);
}

int exa_fv_grid_step_device(exa_fv_plan* p, const double* Q_dev, double* QNext_dev, const long* grid, const double* boundary_dev,
                            const double* centre_dev, double t, double dt, double h, double* lambda_next_dev, void* stream) {
    // every face periodic (boundary_dev NULL), or every face a prescribed state
    static const int all_state[6] = {EXA_FV_FACE_STATE, EXA_FV_FACE_STATE, EXA_FV_FACE_STATE, EXA_FV_FACE_STATE, EXA_FV_FACE_STATE, EXA_FV_FACE_STATE};
    return fv_grid_step("exa_fv_grid_step_device", p, Q_dev, QNext_dev, grid, boundary_dev ? all_state : nullptr, boundary_dev, centre_dev, t, dt, h, lambda_next_dev,
                                      stream);
}

int exa_fv_grid_step_muscl_device(exa_fv_plan* p, const double* Q_dev, double* QNext_dev, const long* grid, const int* face_kind,
                                  const double* face_data_dev, double dt, double h, double* lambda_next_dev, void* stream) {
    const char* who = "exa_fv_grid_step_muscl_device";
    if (!p || !grid || !Q_dev || !QNext_dev) { set_error("%s: NULL argument (plan, grid, Q_dev and QNext_dev are all needed)", who); return EXA_ERR_INVALID; }
    if (p->mode != EXA_FV_MUSCL_HANCOCK) {
        set_error("%s: the plan's mode is %d, this entry serves EXA_FV_MUSCL_HANCOCK plans; exa_fv_grid_step_device[_bc] is the grid step of the "
                  "other modes", who, p->mode);
        return EXA_ERR_INVALID;
    }
    if (p->streamed) {
        set_error("%s: the plan streams its patches plane by plane (exa_fv_plan_create_streamed); the one-launch gather is not built for that form -- "
                  "use the two-pass form: fill the halos of the array with halo and call exa_fv_time_step_device", who);
        return EXA_ERR_INVALID;
    }
    if (p->P < 2) {
        set_error("%s: patch_size %d -- the second halo layer would belong to the neighbour's neighbour; patch_size >= 2 is served here, a grid of "
                  "smaller patches by the two-pass form (fill the halos of the array with halo and call exa_fv_time_step_device)", who, p->P);
        return EXA_ERR_INVALID;
    }
    if (Q_dev == QNext_dev) { set_error("%s: the new states need an array of their own (the neighbours read the old ones): pass two arrays and swap them", who); return EXA_ERR_INVALID; }
    if (!(h > 0.0)) { set_error("%s: EXA_FV_MUSCL_HANCOCK needs the volume size h > 0", who); return EXA_ERR_INVALID; }
    FvGrid ga;
    int rc = fv_grid_args(who, true, p, grid, face_kind, face_data_dev, lambda_next_dev, &ga);
    if (rc) return rc;
    rc = use_device(p->device);
    if (rc) return rc;
    return fv_step(p, const_cast<double*>(Q_dev), QNext_dev, nullptr, nullptr, 0.0, dt, h, &ga, stream);
}

int exa_fv_max_eigenvalue(exa_fv_plan* p, const double* Q_dev, int halo_less, const double* centre_dev, double t, double h, double* lambda_dev,
                          void* stream) {
    if (!p || !lambda_dev || (!Q_dev && p->count > 0)) { set_error("exa_fv_max_eigenvalue: NULL argument"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    // (a halo-less array is a patch array with halo_size 0: every volume is an interior volume)
    const auto scan = slot_or_error(p->k->fv_maxeig, p->pde, "FV eigenvalue scan");
    return scan ? scan(p->dim, p->P, halo_less ? 0 : p->H, p->n_real + p->n_aux, p->n_patches, Q_dev, lambda_dev, centre_dev, t, h, (hipStream_t)stream)
                : EXA_ERR_INVALID;
}

long exa_fv_qout_count(const exa_fv_plan* plan) {
    return plan ? plan->n_patches * lpow(plan->P, plan->dim) * (plan->n_real + plan->n_aux) : 0;
}

int exa_fv_time_step_device(exa_fv_plan* p, double* Q_dev, double dt, double h, void* stream) {
    return exa_fv_time_step_device_masked(p, Q_dev, nullptr, dt, h, stream);
}

int exa_fv_time_step_host(exa_fv_plan* p, double* Q_host, double dt, double h) {
    if (!p || !Q_host) { set_error("exa_fv_time_step_host: NULL argument"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    if (p->count == 0) return EXA_OK;
    double* d = nullptr;
    const size_t bytes = (size_t)p->count * sizeof(double);
    EXA_HIP(hipMalloc(&d, bytes));
    hipError_t e = hipMemcpy(d, Q_host, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = exa_fv_time_step_device(p, d, dt, h, nullptr);
        if (rc == EXA_OK) {
            e = hipDeviceSynchronize();
            if (e == hipSuccess) e = hipMemcpy(Q_host, d, bytes, hipMemcpyDeviceToHost);
        }
    }
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("exa_fv_time_step_host: %s", hipGetErrorString(e)); return EXA_ERR_HIP; }
    return EXA_OK;
}

/* ---- DG ---------------------------------------------------------------------- */

int exa_dg_plan_create(int device, int dim, int N, int n_vars, int pde, int n_picard, const long* ncells,
                       exa_dg_plan** plan) {
    if (!plan || !ncells) { set_error("exa_dg_plan_create: NULL argument"); return EXA_ERR_INVALID; }
    *plan = nullptr;
    if (dim != 2 && dim != 3) { set_error("check viability of inputs"); return EXA_ERR_INVALID; }
    const PdeKernels* k = pde_kernels(pde);
    const DgLaunchTable* tab = k ? k->dg[dim] : nullptr;
    if (!tab) { set_error("ADER-DG: no kernels for dim %d, pde %d", dim, pde); return EXA_ERR_INVALID; }
    if (N < 2 || N > tab->max_n) {
        set_error("ADER-DG: N = %d unsupported for dim %d (2..%d)", N, dim, tab->max_n);
        return EXA_ERR_INVALID;
    }
    if (n_vars != tab->nv) { set_error("ADER-DG: pde %d evolves %d variables, got n_vars = %d", pde, tab->nv, n_vars); return EXA_ERR_INVALID; }
    long nc = 1;
    for (int d = 0; d < dim; d++) {
        if (ncells[d] < 1) { set_error("ncells[%d] = %ld", d, ncells[d]); return EXA_ERR_INVALID; }
        nc *= ncells[d];
    }
    int rc = use_device(device);
    if (rc) return rc;
    exa_dg_plan* p = new (std::nothrow) exa_dg_plan;
    if (!p) { set_error("out of host memory"); return EXA_ERR_ALLOC; }
    p->device = device; p->dim = dim; p->N = N; p->nv = n_vars; p->pde = pde;
    p->n_it = n_picard < 0 ? N : n_picard;
    p->nc[0] = ncells[0]; p->nc[1] = ncells[1]; p->nc[2] = dim == 3 ? ncells[2] : 1;
    p->ncells = nc;
    p->k = k;
    p->tab = tab;
    if (build_dg_operators(N, &p->ops) != 0) { delete p; set_error("operator construction failed for N = %d", N); return EXA_ERR_INVALID; }
    // operator block image in HBM
    p->ops.dev = nullptr;
    const size_t ob = tab->ops_image(N, &p->ops, nullptr);
    std::vector<char> img(ob);
    tab->ops_image(N, &p->ops, img.data());
    hipError_t e = hipMalloc(&p->ops.dev, ob);
    if (e == hipSuccess) e = hipMemcpy(p->ops.dev, img.data(), ob, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (p->ops.dev) (void)hipFree(p->ops.dev);
        delete p;
        set_error("operator block upload failed: %s", hipGetErrorString(e));
        return EXA_ERR_HIP;
    }
    p->ops.scratch = nullptr;
    p->ops.lim = nullptr;
    p->ops.stage_a_reserve = 0;
    p->ops.origin[0] = p->ops.origin[1] = p->ops.origin[2] = 0.0;
    p->ops.time = 0.0;
    p->idx[0] = p->idx[1] = p->idx[2] = 0.0;
    p->ops.stage_a_variant = EXA_STAGE_A_AUTO;
    if (const char* ev = getenv("EXA_STAGE_A")) {
        if (!strcmp(ev, "lds")) p->ops.stage_a_variant = EXA_STAGE_A_LDS;
        else if (!strcmp(ev, "reg")) p->ops.stage_a_variant = EXA_STAGE_A_REG;
    }
    const size_t sb = tab->scratch_bytes(N);
    if (sb > 0) {
        e = hipMalloc(&p->ops.scratch, sb);
        if (e != hipSuccess) {
            (void)hipFree(p->ops.dev);
            delete p;
            set_error("scratch slab (%zu B) allocation failed: %s", sb, hipGetErrorString(e));
            return EXA_ERR_ALLOC;
        }
    }
    *plan = p;
    return EXA_OK;
}

int exa_dg_plan_destroy(exa_dg_plan* plan) {
    if (plan) {
        if (plan->ops.scratch) (void)hipFree(plan->ops.scratch);
        if (plan->ops.lim) (void)hipFree(plan->ops.lim);
        if (plan->ops.dev) (void)hipFree(plan->ops.dev);
        delete plan;
    }
    return EXA_OK;
}

int exa_dg_plan_set_stage_a(exa_dg_plan* plan, int variant) {
    if (!plan) { set_error("exa_dg_plan_set_stage_a: NULL plan"); return EXA_ERR_INVALID; }
    if (variant != EXA_STAGE_A_AUTO && variant != EXA_STAGE_A_LDS && variant != EXA_STAGE_A_REG) {
        set_error("exa_dg_plan_set_stage_a: variant %d (EXA_STAGE_A_AUTO|LDS|REG)", variant);
        return EXA_ERR_INVALID;
    }
    plan->ops.stage_a_variant = variant;
    return EXA_OK;
}

int exa_dg_plan_set_stage_a_reserve(exa_dg_plan* plan, int workgroups) {
    if (!plan || workgroups < 0) { set_error("exa_dg_plan_set_stage_a_reserve: bad argument"); return EXA_ERR_INVALID; }
    plan->ops.stage_a_reserve = workgroups;
    return EXA_OK;
}

const char* exa_dg_stage_a_kernel(const exa_dg_plan* plan) {
    if (!plan || !plan->tab->stage_a_name) return "";
    return plan->tab->stage_a_name(plan->N, plan->n_it, plan->ops.stage_a_variant);
}

long exa_dg_dof_count(const exa_dg_plan* p) { return p ? p->ncells * lpow(p->N, p->dim) * p->nv : 0; }
long exa_dg_trace_count(const exa_dg_plan* p) { return p ? (long)p->dim * 2 * p->ncells * 2 * p->nv * lpow(p->N, p->dim - 1) : 0; }
long exa_dg_face_count(const exa_dg_plan* p, int d) {
    if (!p || d < 0 || d >= p->dim) return 0;
    return (p->ncells / p->nc[d]) * 2 * p->nv * lpow(p->N, p->dim - 1);
}

int exa_dg_operators(const exa_dg_plan* p, double* xi, double* w, double* D, double* Kxi, double* phiL, double* phiR,
                     double* iK1) {
    if (!p) { set_error("exa_dg_operators: NULL plan"); return EXA_ERR_INVALID; }
    const int N = p->N;
    if (xi) memcpy(xi, p->ops.xi, N * sizeof(double));
    if (w) memcpy(w, p->ops.w, N * sizeof(double));
    if (D) memcpy(D, p->ops.D, N * N * sizeof(double));
    if (Kxi) memcpy(Kxi, p->ops.Kxi, N * N * sizeof(double));
    if (phiL) memcpy(phiL, p->ops.phiL, N * sizeof(double));
    if (phiR) memcpy(phiR, p->ops.phiR, N * sizeof(double));
    if (iK1) memcpy(iK1, p->ops.iK1, N * N * sizeof(double));
    return EXA_OK;
}

int exa_dg_work(const exa_dg_plan* p, double* fa, double* fb, double* ba, double* bb) {
    if (!p) { set_error("exa_dg_work: NULL plan"); return EXA_ERR_INVALID; }
    // c_F = c_lambda = 20 flop
    const double d = p->dim, m = p->nv, N = p->N, cF = 20, cL = 20;
    const double Nd = (double)lpow(p->N, p->dim), Nd1 = Nd * N, Nd2 = Nd1 * N, Nf = Nd / N;
    double a;
    if (p->n_it > 0) a = p->n_it * (2 * (d + 1) * m * Nd2 + d * cF * Nd1) + 2 * (d + 1) * m * Nd1 + 2 * d * m * Nd1 + 8 * d * m * Nd;
    else a = d * cF * Nd + 2 * d * m * Nd1 + 8 * d * m * Nd;
    const double b = d * Nf * (2 * cL + 6 * m) + 4 * d * m * Nd;
    if (fa) *fa = a * p->ncells;
    if (fb) *fb = b * p->ncells;
    if (ba) *ba = (16 * m * Nd + 32 * d * m * Nf) * p->ncells;   // u read + u* written + traces written
    if (bb) *bb = (16 * m * Nd + 64 * d * m * Nf) * p->ncells;   // u* read + u written + own and neighbour traces read
    return EXA_OK;
}

static void inv_dx(const exa_dg_plan* p, const double* dx, double* idx) {
    for (int d = 0; d < 3; d++) idx[d] = d < p->dim ? 1.0 / dx[d] : 0.0;
}

static int make_box(const exa_dg_plan* p, const long* lo, const long* hi, CellBox* box) {
    box->nbox = 1;
    for (int d = 0; d < 3; d++) {
        box->nc[d] = p->nc[d];
        box->lo[d] = (lo && d < p->dim) ? lo[d] : 0;
        const long h = (hi && d < p->dim) ? hi[d] : p->nc[d];
        if (box->lo[d] < 0 || h > p->nc[d] || h < box->lo[d]) {
            set_error("cell box [%ld,%ld) outside the block in direction %d", box->lo[d], h, d);
            return EXA_ERR_INVALID;
        }
        box->nb[d] = h - box->lo[d];
        box->nbox *= box->nb[d];
    }
    return EXA_OK;
}

int exa_dg_predictor_volume_box(exa_dg_plan* p, double* u_dev, double* trace_dev, const long* lo, const long* hi, double dt,
                                const double* dx, void* stream) {
    if (!p || !u_dev || !trace_dev || !dx) { set_error("exa_dg_predictor_volume: NULL argument"); return EXA_ERR_INVALID; }
    for (int d = 0; d < p->dim; d++)
        if (!(dx[d] > 0.0)) { set_error("dx[%d] must be > 0", d); return EXA_ERR_INVALID; }
    CellBox box;
    int rc = make_box(p, lo, hi, &box);
    if (rc) return rc;
    rc = use_device(p->device);
    if (rc) return rc;
    double idx[3];
    inv_dx(p, dx, idx);
    for (int d = 0; d < 3; d++) p->idx[d] = idx[d];
    return p->tab->stage_a(p->N, u_dev, u_dev, trace_dev, p->ncells, &box, dt, idx, p->n_it, &p->ops, (hipStream_t)stream);
}

int exa_dg_predictor_volume(exa_dg_plan* p, double* u_dev, double* trace_dev, double dt, const double* dx, void* stream) {
    return exa_dg_predictor_volume_box(p, u_dev, trace_dev, nullptr, nullptr, dt, dx, stream);
}

static int riemann_corrector(exa_dg_plan* p, double* u_dev, const double* trace_dev, const double* const* ghost_dev,
                             const long* lo, const long* hi, double dt, const double* dx, double* lambda_dev, void* stream);

int exa_dg_riemann_corrector(exa_dg_plan* p, double* u_dev, const double* trace_dev, const double* const* ghost_dev,
                             const long* lo, const long* hi, double dt, const double* dx, void* stream) {
    return riemann_corrector(p, u_dev, trace_dev, ghost_dev, lo, hi, dt, dx, nullptr, stream);
}

int exa_dg_riemann_corrector_cfl(exa_dg_plan* p, double* u_dev, const double* trace_dev, const double* const* ghost_dev,
                                 const long* lo, const long* hi, double dt, const double* dx, double* lambda_dev, void* stream) {
    if (!lambda_dev) { set_error("exa_dg_riemann_corrector_cfl: NULL lambda_dev"); return EXA_ERR_INVALID; }
    if (p && (exa_pde_flags(p->pde) & EXA_PDE_FLAG_XT)) {
        set_error("exa_dg_riemann_corrector_cfl: the eigenvalue of this term set depends on position / time -- its CFL scan needs the node coordinates (exa_pde_eval_device_at)");
        return EXA_ERR_INVALID;
    }
    if (p) {
        int rc = use_device(p->device);
        if (rc) return rc;
        hipError_t e = hipMemsetAsync(lambda_dev, 0, sizeof(double), (hipStream_t)stream);
        if (e != hipSuccess) { set_error("exa_dg_riemann_corrector_cfl: memset: %s", hipGetErrorString(e)); return EXA_ERR_HIP; }
    }
    return riemann_corrector(p, u_dev, trace_dev, ghost_dev, lo, hi, dt, dx, lambda_dev, stream);
}

static int riemann_corrector(exa_dg_plan* p, double* u_dev, const double* trace_dev, const double* const* ghost_dev,
                             const long* lo, const long* hi, double dt, const double* dx, double* lambda_dev, void* stream) {
    if (!p || !u_dev || !trace_dev || !dx) { set_error("exa_dg_riemann_corrector: NULL argument"); return EXA_ERR_INVALID; }
    StageBBox box;
    box.lam = lambda_dev;
    CellBox cb;
    int rcb = make_box(p, lo, hi, &cb);
    if (rcb) return rcb;
    for (int d = 0; d < 3; d++) { box.nc[d] = cb.nc[d]; box.lo[d] = cb.lo[d]; box.nb[d] = cb.nb[d]; }
    for (int f = 0; f < 6; f++) box.ghost[f] = (ghost_dev && f < 2 * p->dim) ? ghost_dev[f] : nullptr;
    int rc = use_device(p->device);
    if (rc) return rc;
    double idx[3];
    inv_dx(p, dx, idx);
    return p->tab->stage_b(p->N, u_dev, trace_dev, &box, p->ncells, dt, idx, &p->ops, (hipStream_t)stream);
}

int exa_dg_plan_set_origin_time(exa_dg_plan* p, const double* origin, double t) {
    if (!p) { set_error("exa_dg_plan_set_origin_time: NULL plan"); return EXA_ERR_INVALID; }
    for (int d = 0; d < 3; d++) p->ops.origin[d] = (origin && d < p->dim) ? origin[d] : 0.0;
    p->ops.time = t;
    return EXA_OK;
}

int exa_dg_has_corrector_predictor(const exa_dg_plan* p) {
    return (p && p->tab->has_stage_ba) ? p->tab->has_stage_ba(p->N, p->n_it, p->ops.stage_a_variant) : 0;
}

int exa_dg_corrector_predictor(exa_dg_plan* p, double* u_dev, const double* trace_in_dev, double* trace_out_dev,
                               const double* const* ghost_dev, const long* lo, const long* hi, double dt_prev, double dt,
                               const double* dx, double* u_plain_dev, void* stream) {
    if (!p || !u_dev || !trace_in_dev || !trace_out_dev || !dx) { set_error("exa_dg_corrector_predictor: NULL argument"); return EXA_ERR_INVALID; }
    if (trace_in_dev == trace_out_dev) { set_error("exa_dg_corrector_predictor: the new traces need an array of their own"); return EXA_ERR_INVALID; }
    if (!exa_dg_has_corrector_predictor(p)) {
        set_error("exa_dg_corrector_predictor: not built for this plan (3-D, N = 6, register-resident stage A, n_picard >= 1)");
        return EXA_ERR_INVALID;
    }
    for (int d = 0; d < p->dim; d++)
        if (!(dx[d] > 0.0)) { set_error("dx[%d] must be > 0", d); return EXA_ERR_INVALID; }
    CellBox box;
    int rc = make_box(p, lo, hi, &box);
    if (rc) return rc;
    rc = use_device(p->device);
    if (rc) return rc;
    double idx[3];
    inv_dx(p, dx, idx);
    const double* gh[6];
    for (int f = 0; f < 6; f++) gh[f] = (ghost_dev && f < 2 * p->dim) ? ghost_dev[f] : nullptr;
    return p->tab->stage_ba(p->N, u_dev, trace_in_dev, trace_out_dev, p->ncells, &box, gh, dt_prev, dt, idx, p->n_it, &p->ops, u_plain_dev,
                            (hipStream_t)stream);
}

int exa_dg_pack_face(exa_dg_plan* p, const double* trace_dev, int d, int side, double* buf_dev, void* stream) {
    if (!p || !trace_dev || !buf_dev || d < 0 || d >= p->dim || side < 0 || side > 1) { set_error("exa_dg_pack_face: bad argument"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    // trace[(d*2+side)][cx][cy][cz][TS] -> the layer c_d = 0 (side 0) or nc_d-1 (side 1) as a strided 2-D copy
    const long TS = 2L * p->nv * lpow(p->N, p->dim - 1);
    long outer = 1, inner = 1;
    for (int a = 0; a < d; a++) outer *= p->nc[a];
    for (int a = d + 1; a < 3; a++) inner *= p->nc[a];
    const long layer = side ? p->nc[d] - 1 : 0;
    const double* src = trace_dev + ((long)(d * 2 + side) * p->ncells + layer * inner) * TS;
    EXA_HIP(hipMemcpy2DAsync(buf_dev, (size_t)inner * TS * sizeof(double), src, (size_t)p->nc[d] * inner * TS * sizeof(double),
                             (size_t)inner * TS * sizeof(double), (size_t)outer, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return EXA_OK;
}

int exa_dg_boundary_ghost(exa_dg_plan* p, const double* trace_dev, int d, int side, int kind, const double* coeff, const double* states_dev,
                          double dt, double* ghost_dev, double* lambda_dev, void* stream) {
    if (!p || !ghost_dev) { set_error("exa_dg_boundary_ghost: NULL plan or ghost_dev"); return EXA_ERR_INVALID; }
    if (d < 0 || d >= p->dim || side < 0 || side > 1) { set_error("exa_dg_boundary_ghost: face (d %d, side %d) outside a %d-D block", d, side, p->dim); return EXA_ERR_INVALID; }
    if (kind != EXA_BC_OUTFLOW && kind != EXA_BC_WALL && kind != EXA_BC_DIRICHLET) {
        set_error("exa_dg_boundary_ghost: kind %d (EXA_BC_OUTFLOW | EXA_BC_WALL | EXA_BC_DIRICHLET)", kind);
        return EXA_ERR_INVALID;
    }
    if (kind != EXA_BC_DIRICHLET && (!trace_dev || !coeff)) { set_error("exa_dg_boundary_ghost: outflow / wall need trace_dev and the 2*n_vars factors coeff"); return EXA_ERR_INVALID; }
    if (kind != EXA_BC_DIRICHLET && (states_dev || lambda_dev)) { set_error("exa_dg_boundary_ghost: states_dev / lambda_dev belong to EXA_BC_DIRICHLET"); return EXA_ERR_INVALID; }
    if (kind == EXA_BC_DIRICHLET && !states_dev && !coeff) { set_error("exa_dg_boundary_ghost: Dirichlet needs states_dev or the constant state coeff"); return EXA_ERR_INVALID; }
    if (kind == EXA_BC_DIRICHLET && states_dev && coeff) { set_error("exa_dg_boundary_ghost: Dirichlet takes states_dev or coeff, not both"); return EXA_ERR_INVALID; }
    if (kind == EXA_BC_DIRICHLET && (exa_pde_flags(p->pde) & EXA_PDE_FLAG_XT) && !(p->idx[0] > 0.0)) {
        set_error("exa_dg_boundary_ghost: the face nodes of this term set need the cell size of a stage A (exa_dg_predictor_volume) first");
        return EXA_ERR_INVALID;
    }
    if (!p->tab->boundary) { set_error("exa_dg_boundary_ghost: the kernels of pde %d carry no boundary entry (rebuild its library)", p->pde); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    return p->tab->boundary(p->N, trace_dev, p->ncells, p->nc, d, side, kind, coeff, states_dev, dt, &p->ops, p->idx, ghost_dev, lambda_dev,
                            (hipStream_t)stream) == 0 ? EXA_OK : EXA_ERR_HIP;
}

/* ---- FV subcell limiter glue ------------------------------------------------------ */

int exa_lim_operators(const exa_dg_plan* p, double* P, double* R) {
    if (!p || !P || !R) { set_error("exa_lim_operators: NULL argument"); return EXA_ERR_INVALID; }
    if (build_limiter_operators(&p->ops, 2 * p->N - 1, P, R) != 0) { set_error("limiter operator construction failed"); return EXA_ERR_INVALID; }
    return EXA_OK;
}

long exa_lim_patch_count(const exa_dg_plan* p) { return p ? lpow(2 * p->N + 1, p->dim) * p->nv : 0; }

static int lim_tables(exa_dg_plan* p) {
    if (p->ops.lim) return EXA_OK;
    const int N = p->N, Ns = 2 * N - 1;
    std::vector<double> t(2 * (size_t)N * Ns);
    if (build_limiter_operators(&p->ops, Ns, t.data(), t.data() + (size_t)N * Ns) != 0) { set_error("limiter operator construction failed"); return EXA_ERR_INVALID; }
    EXA_HIP(hipMalloc(&p->ops.lim, t.size() * sizeof(double)));
    EXA_HIP(hipMemcpy(p->ops.lim, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    return EXA_OK;
}

int exa_dg_project_patches_ghost(exa_dg_plan* p, const double* u_dev, const long* cells_dev, long n, double* patch_dev,
                                 const double* const* ghost_layers_dev, void* stream) {
    if (!p || !u_dev || (n > 0 && (!cells_dev || !patch_dev)) || n < 0) { set_error("exa_dg_project_patches: bad argument"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    rc = lim_tables(p);
    if (rc) return rc;
    const int Ns = 2 * p->N - 1;
    LimGhosts gh{};
    for (int f = 0; f < 6; f++) gh.layer[f] = (ghost_layers_dev && f < 2 * p->dim) ? ghost_layers_dev[f] : nullptr;
    return limiter_project(p->dim, p->N, Ns, p->nv, p->nc, u_dev, cells_dev, n, patch_dev, static_cast<const double*>(p->ops.lim), &gh,
                           (hipStream_t)stream);
}

int exa_dg_project_patches(exa_dg_plan* p, const double* u_dev, const long* cells_dev, long n, double* patch_dev, void* stream) {
    return exa_dg_project_patches_ghost(p, u_dev, cells_dev, n, patch_dev, nullptr, stream);
}

long exa_lim_face_layer_count(const exa_dg_plan* p, int d) {
    if (!p || d < 0 || d >= p->dim) return 0;
    long nt = 1;
    for (int b = 0; b < p->dim; b++)
        if (b != d) nt *= p->nc[b];
    return nt * lpow(2 * p->N - 1, p->dim - 1) * p->nv;
}

int exa_lim_face_layers(exa_dg_plan* p, const double* u_dev, int d, int side, const double* need_dev, double* out_dev, void* stream) {
    if (!p || !u_dev || !out_dev || d < 0 || d >= p->dim || side < 0 || side > 1) { set_error("exa_lim_face_layers: bad argument"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    rc = lim_tables(p);
    if (rc) return rc;
    return limiter_face_layers(p->dim, p->N, 2 * p->N - 1, p->nv, p->nc, u_dev, d, side, need_dev, out_dev,
                               static_cast<const double*>(p->ops.lim), (hipStream_t)stream);
}

int exa_dg_reconstruct_patches(exa_dg_plan* p, const double* patch_dev, const long* cells_dev, long n, double* u_dev, void* stream) {
    if (!p || !u_dev || (n > 0 && (!cells_dev || !patch_dev)) || n < 0) { set_error("exa_dg_reconstruct_patches: bad argument"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    rc = lim_tables(p);
    if (rc) return rc;
    const int Ns = 2 * p->N - 1;
    return limiter_reconstruct(p->dim, p->N, Ns, p->nv, patch_dev, cells_dev, n, u_dev,
                               static_cast<const double*>(p->ops.lim) + (size_t)p->N * Ns, 1, (hipStream_t)stream);
}

/* ---- patches with halo 2: what the second-order patch update (EXA_FV_MUSCL_HANCOCK) reads ---- */

long exa_lim_patch_count_halo(const exa_dg_plan* p, int halo) {
    if (!p || (halo != 1 && halo != 2)) { set_error("exa_lim_patch_count_halo: %s", !p ? "NULL plan" : "halo must be 1 or 2"); return EXA_ERR_INVALID; }
    return lpow(2 * p->N - 1 + 2 * halo, p->dim) * p->nv;
}

int exa_lim_project_patches_halo2(exa_dg_plan* p, const double* u_dev, const long* cells_dev, long n, double* patch_dev, const int* face_kind,
                                  const double* face_data_dev, void* stream) {
    if (!p || !u_dev || (n > 0 && (!cells_dev || !patch_dev)) || n < 0) { set_error("exa_lim_project_patches_halo2: bad argument"); return EXA_ERR_INVALID; }
    int bkind[6];
    bool bounded;
    int rc = check_face_kinds("exa_lim_project_patches_halo2", false, p->dim, face_kind, face_data_dev, bkind, &bounded);
    if (rc) return rc;
    rc = use_device(p->device);
    if (rc) return rc;
    rc = lim_tables(p);
    if (rc) return rc;
    return limiter_project_halo2(p->dim, p->N, p->nv, p->nc, u_dev, cells_dev, n, patch_dev, static_cast<const double*>(p->ops.lim), face_kind,
                                 face_kind ? face_data_dev : nullptr, (hipStream_t)stream);
}

int exa_lim_reconstruct_patches_halo(exa_dg_plan* p, const double* patch_dev, const long* cells_dev, long n, double* u_dev, int halo, void* stream) {
    if (!p || !u_dev || (n > 0 && (!cells_dev || !patch_dev)) || n < 0) { set_error("exa_lim_reconstruct_patches_halo: bad argument"); return EXA_ERR_INVALID; }
    if (halo != 1 && halo != 2) { set_error("exa_lim_reconstruct_patches_halo: halo = %d, the patches have halo 1 or 2", halo); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    rc = lim_tables(p);
    if (rc) return rc;
    const int Ns = 2 * p->N - 1;
    return limiter_reconstruct(p->dim, p->N, Ns, p->nv, patch_dev, cells_dev, n, u_dev, static_cast<const double*>(p->ops.lim) + (size_t)p->N * Ns, halo,
                               (hipStream_t)stream);
}

// (a term set without a detector unit of its own -- null slots -- is watched by the Euler-layout criterion of limiter.hip: k_dmp = 2.  So is the
// zero-filled stand-in for a plan that the tests of the argument checks hand in on a machine without a GPU, which has no table: this is the only
// read of p->k in front of a use_device, where those tests end)
long exa_lim_bounds_count(const exa_dg_plan* p) { return p ? 2L * (p->k ? p->k->k_dmp : 2) : 0; }

int exa_lim_snapshot(exa_dg_plan* p, const double* u_dev, double* u_old_dev, double* bounds_dev, void* stream) {
    const bool no_bounds = p && u_dev && exa_lim_bounds_count(p) == 0;         // (nothing watched: bounds_dev is not touched)
    if (!p || !u_dev || (!bounds_dev && !no_bounds) || u_dev == u_old_dev) { set_error("exa_lim_snapshot: bad argument (plan, u_dev or bounds_dev is NULL, or u_old_dev == u_dev)"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    if (const auto own = p->k->lim_snapshot) return own(p->dim, p->N, p->ncells, u_dev, u_old_dev, bounds_dev, (hipStream_t)stream);
    return limiter_snapshot(p->dim, p->N, p->nv, p->ncells, u_dev, u_old_dev, bounds_dev, (hipStream_t)stream);
}

int exa_lim_detect(exa_dg_plan* p, const double* u_cand_dev, const double* bounds_dev, const double* const* ghost_bounds_dev,
                   const int* face_kind, double d0, double eps, double floor, unsigned char* mask_dev, void* stream) {
    const bool no_bounds = p && u_cand_dev && mask_dev && exa_lim_bounds_count(p) == 0;
    if (!p || !u_cand_dev || (!bounds_dev && !no_bounds) || !mask_dev) { set_error("exa_lim_detect: NULL argument"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    const auto own = p->k->lim_detect;
    if (!own && p->nv < 2) { set_error("exa_lim_detect: needs a density and an energy (n_vars >= 2), the plan has %d", p->nv); return EXA_ERR_INVALID; }
    if (!(d0 >= 0.0) || !(eps >= 0.0) || floor != floor) { set_error("exa_lim_detect: d0 and eps must be >= 0 and floor a number"); return EXA_ERR_INVALID; }
    LimGhosts gb{};
    for (int f = 0; f < 2 * p->dim; f++) {
        const int kind = face_kind ? face_kind[f] : EXA_LIM_FACE_PERIODIC;
        if (kind < EXA_LIM_FACE_PERIODIC || kind > EXA_LIM_FACE_NONE) { set_error("exa_lim_detect: face_kind[%d] = %d", f, kind); return EXA_ERR_INVALID; }
        if (kind == EXA_LIM_FACE_GHOST) {
            if (no_bounds) continue;                                                   // (nothing watched: no neighbourhood)
            if (!ghost_bounds_dev || !ghost_bounds_dev[f]) { set_error("exa_lim_detect: face %d is EXA_LIM_FACE_GHOST without ghost bounds", f); return EXA_ERR_INVALID; }
            gb.layer[f] = ghost_bounds_dev[f];
        }
    }
    if (own) return own(p->dim, p->N, p->nc, u_cand_dev, bounds_dev, &gb, face_kind, d0, eps, floor, mask_dev, (hipStream_t)stream);
    return limiter_detect(p->dim, p->N, p->nv, p->nc, u_cand_dev, bounds_dev, &gb, face_kind, d0, eps, floor, mask_dev, (hipStream_t)stream);
}

// The slots of the conservative interface: the built-in Euler (5 variables) and advection (1 variable) sets have them, and registered sets that
// ask for the interface (EXA_PDE_FLAG_CONSERVATIVE: exa_register_pde has seen their unit).  -> the plan's table, or null with the message
static const PdeKernels* lim_conservative(const exa_dg_plan* p, const char* who) {
    const PdeKernels* k = p->k;
    if (k->flags & (EXA_PDE_FLAG_XT | EXA_PDE_FLAG_NCP)) {
        set_error("%s: term set %d carries position- / time-dependent terms or a non-conservative product; the conservative interface is built for "
                  "term sets of the state alone without one", who, p->pde);
        return nullptr;
    }
    if ((k->flags & EXA_PDE_FLAG_CONSERVATIVE) && p->nv != k->nv) { set_error("%s: term set %d has %d variables, the plan %d", who, p->pde, k->nv, p->nv); return nullptr; }
    if (!k->lim_face_flux || !k->lim_interface_correct || p->nv != k->nv) {
        set_error("%s: term set %d with %d variables; the conservative interface is built for the built-in Euler (pde 1, 5 variables) and advection (pde 2, 1 variable) sets "
                  "and for registered sets generated with SympyPDE(conservative_interface=True)", who, p->pde, p->nv);
        return nullptr;
    }
    return k;
}

long exa_lim_face_flux_count(const exa_dg_plan* p) { return p ? 2L * p->dim * p->nv * lpow(p->N, p->dim - 1) : 0; }

int exa_lim_face_flux(exa_dg_plan* p, const double* patch_dev, const long* cells_dev, long n, double* fvflux_dev, void* stream) {
    if (!p || n < 0 || (n > 0 && (!patch_dev || !cells_dev || !fvflux_dev))) { set_error("exa_lim_face_flux: bad argument (NULL plan or array, or n < 0)"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    const PdeKernels* k = lim_conservative(p, "exa_lim_face_flux");
    if (!k) return EXA_ERR_INVALID;
    rc = lim_tables(p);
    if (rc) return rc;
    const double* Rdev = static_cast<const double*>(p->ops.lim) + (size_t)p->N * (2 * p->N - 1);
    return k->lim_face_flux(p->dim, p->N, patch_dev, cells_dev, n, fvflux_dev, Rdev, (hipStream_t)stream) == 0 ? EXA_OK : EXA_ERR_HIP;
}

int exa_lim_interface_correct(exa_dg_plan* p, double* u_dev, const double* trace_dev, const long* cells_dev, long n, const unsigned char* mask_dev,
                              const int* face_kind, const double* fvflux_dev, double dt, const double* dx, void* stream) {
    if (!p || !u_dev || !trace_dev || !mask_dev || !dx || n < 0 || (n > 0 && (!cells_dev || !fvflux_dev))) {
        set_error("exa_lim_interface_correct: bad argument (NULL plan or array, or n < 0)");
        return EXA_ERR_INVALID;
    }
    int rc = use_device(p->device);
    if (rc) return rc;
    const PdeKernels* k = lim_conservative(p, "exa_lim_interface_correct");
    if (!k) return EXA_ERR_INVALID;
    for (int f = 0; f < 2 * p->dim; f++) {
        const int kind = face_kind ? face_kind[f] : EXA_LIM_FACE_PERIODIC;
        if (kind == EXA_LIM_FACE_GHOST) {
            set_error("exa_lim_interface_correct: face %d is EXA_LIM_FACE_GHOST; the exchange of face fluxes between blocks is not built", f);
            return EXA_ERR_INVALID;
        }
        if (kind != EXA_LIM_FACE_PERIODIC && kind != EXA_LIM_FACE_NONE) { set_error("exa_lim_interface_correct: face_kind[%d] = %d", f, kind); return EXA_ERR_INVALID; }
    }
    for (int a = 0; a < p->dim; a++)
        if (!(dx[a] > 0.0)) { set_error("exa_lim_interface_correct: dx[%d] must be positive", a); return EXA_ERR_INVALID; }
    return k->lim_interface_correct(p->dim, p->N, p->nc, u_dev, trace_dev, cells_dev, n, mask_dev, face_kind, fvflux_dev, dt, dx, p->ops.w, p->ops.phiL,
                                    p->ops.phiR, (hipStream_t)stream) == 0 ? EXA_OK : EXA_ERR_HIP;
}

int exa_dg_max_eigenvalue(exa_dg_plan* p, const double* u_dev, double* lambda_dev, void* stream) {
    if (!p || !u_dev || !lambda_dev) { set_error("exa_dg_max_eigenvalue: NULL argument"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    return p->tab->maxeig(u_dev, p->ncells * lpow(p->N, p->dim), lambda_dev, (hipStream_t)stream);
}

int exa_dg_has_fused_step(const exa_dg_plan* p) { return (p && p->n_it == 0 && p->tab->fused_single) ? 1 : 0; }

int exa_dg_step_fused(exa_dg_plan* p, const double* u_in_dev, double* u_out_dev, double dt, const double* dx, void* stream) {
    if (!p || !u_in_dev || !u_out_dev || !dx || u_in_dev == u_out_dev) { set_error("exa_dg_step_fused: bad argument (input and output must differ)"); return EXA_ERR_INVALID; }
    if (!exa_dg_has_fused_step(p)) { set_error("exa_dg_step_fused: only for the single-stage scheme (n_picard = 0) in 2-D"); return EXA_ERR_INVALID; }
    for (int d = 0; d < p->dim; d++)
        if (!(dx[d] > 0.0)) { set_error("dx[%d] must be > 0", d); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    double idx[3];
    inv_dx(p, dx, idx);
    return p->tab->fused_single(p->N, u_in_dev, u_out_dev, p->nc, dt, idx, &p->ops, (hipStream_t)stream) == 0 ? EXA_OK : EXA_ERR_HIP;
}

int exa_dg_step_periodic(exa_dg_plan* p, double* u_dev, double* trace_dev, double dt, const double* dx, int n_steps,
                         void* stream) {
    for (int s = 0; s < n_steps; s++) {
        int rc = exa_dg_predictor_volume(p, u_dev, trace_dev, dt, dx, stream);
        if (rc) return rc;
        rc = exa_dg_riemann_corrector(p, u_dev, trace_dev, nullptr, nullptr, nullptr, dt, dx, stream);
        if (rc) return rc;
    }
    return EXA_OK;
}

int exa_dg_step_host(exa_dg_plan* p, double* u_host, double dt, const double* dx, int n_steps) {
    if (!p || !u_host || !dx) { set_error("exa_dg_step_host: NULL argument"); return EXA_ERR_INVALID; }
    int rc = use_device(p->device);
    if (rc) return rc;
    double *u = nullptr, *tr = nullptr;
    const size_t ub = (size_t)exa_dg_dof_count(p) * sizeof(double), tb = (size_t)exa_dg_trace_count(p) * sizeof(double);
    EXA_HIP(hipMalloc(&u, ub));
    hipError_t e = hipMalloc(&tr, tb);
    if (e == hipSuccess) e = hipMemcpy(u, u_host, ub, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = exa_dg_step_periodic(p, u, tr, dt, dx, n_steps, nullptr);
        if (rc == EXA_OK) {
            e = hipDeviceSynchronize();
            if (e == hipSuccess) e = hipMemcpy(u_host, u, ub, hipMemcpyDeviceToHost);
        }
    }
    (void)hipFree(u);
    (void)hipFree(tr);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("exa_dg_step_host: %s", hipGetErrorString(e)); return EXA_ERR_HIP; }
    return EXA_OK;
}

}  // extern "C"

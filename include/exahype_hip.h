/*
 * exahype_hip.h -- C-ABI of libexahype_hip.so, the MI355X (gfx950) drop-in for
 * the cell-local kernel stack of xdslproject/ExaHyPE.
 *
 * Conventions
 *  - every entry point returns 0 on success, a negative EXA_ERR_* otherwise;
 *    exa_last_error() gives the thread-local message.  Nothing throws across
 *    the boundary.
 *  - plain pointers and sizes only.  `*_dev` pointers are device (HBM)
 *    addresses owned by the caller; `*_host` pointers are host memory owned by
 *    the caller.  `stream` is a hipStream_t passed as void* (NULL = default).
 *  - all arithmetic is IEEE fp64.  Arrays use the reference layout: AoS,
 *    row-major, variable fastest (reference `exahype/printers/CPPPrinter.py:247-261`).
 *      FV : Q[patch][i][j]([k])[var], halo included, var < n_real + n_aux
 *      DG : u[cell][node][var], cell = (cx*ncy+cy)*ncz+cz, node = (i*N+j)*N+k
 *    axis 0 is the reference's index `i` (normal == 0).
 *  - a plan is bound to one device; distinct plans are independent; one plan is
 *    not thread-safe.
 *
 * Reference interfaces replaced
 *  - `void time_step(double* Q, double dt);`                  Unit test/test.h:3
 *        -> exa_fv_time_step_host / exa_fv_time_step_device (mode EXA_FV_FAITHFUL)
 *  - `void Flux(const double*, int normal, double* F);`        Unit test/Functions.h:2
 *    `double maxEigenvalue(const double*, int normal);`        Unit test/Functions.h:3
 *    `double max(double*, double*);`                           Unit test/Functions.h:4
 *        -> built-in device PDE terms selected by `pde` (EXA_PDE_*), exercised
 *           point-wise through exa_pde_eval_device
 *  - the generated loop nests `Unit test/test.cpp:11-104` (what
 *    exahype/printers/CPPPrinter.py:84-90 emits per KernelBuilder statement)
 *        -> the fused FV Rusanov patch kernel behind exa_fv_time_step_*
 *  - ADER-DG stages (space-time predictor, volume integral, face extrapolation,
 *    Rusanov Riemann solve, surface corrector): NOT in the reference
 *    (SURVEY.md F2); the north-star adds them.  -> exa_dg_*
 */
#ifndef EXAHYPE_HIP_H
#define EXAHYPE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXA_OK 0
#define EXA_ERR_INVALID (-1)     /* bad argument / unsupported configuration */
#define EXA_ERR_HIP (-2)         /* a HIP runtime call failed */
#define EXA_ERR_NO_DEVICE (-3)   /* no usable GPU */
#define EXA_ERR_ALLOC (-4)

/* point-wise PDE term sets (device twins of Unit test/Functions.cpp) */
#define EXA_PDE_EULER_REF2D 0    /* Functions.cpp:9-62 as compiled by the reference (2-D branch: reads Q[0..3], writes F[0..3]) */
#define EXA_PDE_EULER 1          /* same arithmetic, (rho, m0, m1, m2, E), gamma = 1.4 */
#define EXA_PDE_ADVECTION 2      /* linear advection of every variable, a = (1, 0.5, -0.75) */

/* FV Rusanov patch-update modes */
#define EXA_FV_FAITHFUL 0        /* Unit test/test.cpp:11-104 statement for statement (zero-initialised temporaries) */
#define EXA_FV_RUSANOV 1         /* corrected Rusanov: dt/h, all n_real variables, dissipative sign */
/* Second order: minmod slopes per axis, an unsplit half-step predictor over all axes, the Rusanov flux of the predicted face states (the
 * scheme, statement by statement: exahype_amd/csrc/exa_fv_muscl.hpp).
 *   - halo_size >= 2.  An interior update reads Q at c +- e_d, c +- 2 e_d and c +- e_d +- e_e (d != e): the two halo layers next to the
 *     interior INCLUDING the edge entries (layer 1 along two axes) -- a caller that fills halos fills those too.  It never reads the entries at
 *     (+-2, +-1), the 3-D corner entries or a layer beyond the second.
 *   - served by exa_fv_time_step_host / _device / _device_masked / _device_oop and by _device_at / _device_masked_at (centres and t are
 *     ignored: the term sets of this mode see the state alone); h > 0 is required, as for EXA_FV_RUSANOV.
 *   - term sets: EXA_PDE_EULER, EXA_PDE_ADVECTION and registered ones with EXA_PDE_FLAG_MUSCL_HANCOCK: conservative terms of the state alone,
 *     or -- with EXA_PDE_FLAG_MUSCL_TERMS -- also a source S(q) and / or a non-conservative product B(q) . grad q of the state alone (Euler with
 *     a body force, two-layer-like coupling, a bathymetry carried as an evolved variable with zero flux).  Terms that depend on position / time
 *     are not served in this mode.  EXA_PDE_EULER_REF2D (F[4] never written) is refused.
 *   - exa_fv_plan_create refuses (EXA_ERR_INVALID) a shape whose LDS plan -- 8 ((patch_size + 4)^dim (n_real + n_aux) + (patch_size + 2)^dim
 *     n_real) bytes for one patch -- exceeds the 160 KiB of a compute unit; the message names both figures.  Served: 2-D patch_size <= 32
 *     with 5 variables, <= 20 with 10; 3-D patch_size <= 8 with up to 6.  Larger 3-D patches are served plane by plane, by a plan of
 *     exa_fv_plan_create_streamed (below): up to patch_size 19 with 5 variables.
 *   - exa_fv_grid_step_device[_bc] return EXA_ERR_INVALID: the one-launch grid step takes face neighbours only, this scheme needs the edge
 *     neighbours (diagonal patches); fill the halos of the array with halo and call exa_fv_time_step_device.
 *   - exa_fv_grid_step_muscl_device IS the one-launch grid step of this mode, on halo-less arrays: its kernel gathers the window of a patch from
 *     the face AND the diagonal neighbours (below, beside the grid-step entries); patch_size >= 2.
 *   - exa_fv_max_eigenvalue serves plans of this mode as it serves the others. */
#define EXA_FV_MUSCL_HANCOCK 2

typedef struct exa_fv_plan exa_fv_plan;
typedef struct exa_dg_plan exa_dg_plan;

/* ---- library ---------------------------------------------------------------- */
int exa_version(void);
const char* exa_last_error(void);
int exa_device_count(int* count);

/* ---- user PDE term sets ------------------------------------------------------- */
/* The reference resolves `Flux` / `maxEigenvalue` at link time to user C++ (Unit test/Functions.h:2-3).
 * Here a user term set is a side library generated from SymPy expressions and compiled with hipcc
 * (exahype_amd/pde_codegen.py); registering it yields a pde id >= 100 usable wherever EXA_PDE_* is.  EXA_ERR_INVALID: the file does not load, it is
 * no such library, a unit its flags ask for is missing, or it was built against another layout of the kernel table (one ABI number, checked
 * here: the message says to rebuild the term set). */
int exa_register_pde(const char* library_path, int* pde_id);
/* What a registered term set carries (0 for the built-in ones): EXA_PDE_FLAG_XT -- its terms depend on position / time (they see the
 * coordinates the kernels hand them; exa_pde_eval_device and exa_dg_max_eigenvalue, which have none, evaluate them at x = 0, t = 0:
 * use exa_pde_eval_device_at for the CFL scan of such a term set, as exahype_amd/solvers.py does);
 * EXA_PDE_FLAG_NCP -- it carries a non-conservative product;
 * EXA_PDE_FLAG_ADMISSIBLE -- it says itself what the a-posteriori limiter's detector checks (exa_lim_snapshot / exa_lim_detect below);
 * EXA_PDE_FLAG_CONSERVATIVE -- its side library carries the limiter's conservative DG / FV interface (exa_lim_face_flux /
 * exa_lim_interface_correct below): pde_codegen.SympyPDE(conservative_interface=True), never together with XT or NCP;
 * EXA_PDE_FLAG_MUSCL_HANCOCK -- its side library carries the second-order patch update (EXA_FV_MUSCL_HANCOCK):
 * pde_codegen.SympyPDE(muscl_hancock=True), terms of the state alone (never XT).  Without the next flag such a set is conservative: no NCP, no
 * source;
 * EXA_PDE_FLAG_MUSCL_TERMS -- ... and that update takes the set's source and / or non-conservative product (pde_codegen.SympyPDE(
 * muscl_hancock=True, muscl_terms=True)): the source by the midpoint rule in time, the product in the predictor, as the jump term of the
 * predicted face states and at the half-step state times the volume's slope (exahype_amd/csrc/exa_fv_muscl.hpp).  Every entry that serves an
 * EXA_FV_MUSCL_HANCOCK plan serves such a set; the a-posteriori limiter's second-order mode does not (its patch update knows neither term). */
#define EXA_PDE_FLAG_XT 1
#define EXA_PDE_FLAG_NCP 2
#define EXA_PDE_FLAG_ADMISSIBLE 4
#define EXA_PDE_FLAG_CONSERVATIVE 8
#define EXA_PDE_FLAG_MUSCL_HANCOCK 16
#define EXA_PDE_FLAG_MUSCL_TERMS 32
int exa_pde_flags(int pde);

/* ---- point-wise PDE terms (Functions.h:2-3) ---------------------------------- */
/* For n states Q_dev[n][stride] and a normal: F_dev[n][stride] (first n_flux
 * entries written) and lambda_dev[n].  Either output may be NULL. */
int exa_pde_eval_device(int pde, int normal, long n, int stride, const double* Q_dev, double* F_dev,
                        double* lambda_dev, void* stream);
/* The same with the positions of the states, x_dev [n][3] (NULL: the origin), and the time: for term sets whose terms depend on them
 * (EXA_PDE_FLAG_XT) -- the CFL scan of a host driver hands the volume centres / node coordinates here. */
int exa_pde_eval_device_at(int pde, int normal, long n, int stride, const double* Q_dev, const double* x_dev, double t, double* F_dev,
                           double* lambda_dev, void* stream);

/* ---- Finite-Volume Rusanov patch update (test.h:3) -------------------------- */
int exa_fv_plan_create(int device, int mode, int dim, int patch_size, int halo_size, int n_real, int n_aux,
                       long n_patches, int pde, exa_fv_plan** plan);
/* The same with the choice of the PLANE-STREAMING form of EXA_FV_MUSCL_HANCOCK in 3-D: one workgroup per patch walks the planes of axis 0 and
 * keeps five or six window planes (patch_size + 4)^2 (n_real + n_aux) and three predictor planes (patch_size + 2)^2 n_real in LDS instead of the
 * whole window -- 8 (5 (P + 4)^2 V + 3 (P + 2)^2 n_real) bytes must fit the 160 KiB (5 + 0 variables: patch_size <= 19).  The per-volume
 * arithmetic is the resident kernel's: where both serve a shape the results are bit-identical.
 *   EXA_FV_STREAM_NEVER      what exa_fv_plan_create does
 *   EXA_FV_STREAM_IF_NEEDED  the resident plan where it fits, the streamed one where not (3-D; in 2-D as NEVER)
 *   EXA_FV_STREAM_ALWAYS     the streamed plan wherever it exists (tests, measurements)
 * EXA_ERR_INVALID: a non-zero stream_planes with another mode; ALWAYS in 2-D; a shape whose streamed plan does not fit (the message names the bytes
 * of both plans); an unknown value.
 * A streamed plan is served by every exa_fv_time_step_* entry and by exa_fv_max_eigenvalue; exa_fv_grid_step_muscl_device refuses it (the
 * one-launch gather is not built for this form: use the two-pass form on the array with halo). */
#define EXA_FV_STREAM_NEVER 0
#define EXA_FV_STREAM_IF_NEEDED 1
#define EXA_FV_STREAM_ALWAYS 2
int exa_fv_plan_create_streamed(int device, int mode, int dim, int patch_size, int halo_size, int n_real, int n_aux,
                                long n_patches, int pde, int stream_planes, exa_fv_plan** plan);
int exa_fv_plan_is_streamed(const exa_fv_plan* plan);   /* 0 | 1 */
int exa_fv_plan_destroy(exa_fv_plan* plan);
/* doubles in one Q array: n_patches * (patch_size + 2*halo_size)^dim * (n_real + n_aux) */
long exa_fv_q_count(const exa_fv_plan* plan);
/* exact analogue of `time_step(Q, dt)`: host AoS array updated in place (interior
 * volumes only); the library stages it through HBM.  `h` (volume size) is used
 * by EXA_FV_RUSANOV only. */
int exa_fv_time_step_host(exa_fv_plan* plan, double* Q_host, double dt, double h);
/* same on a device-resident array (the hot path: no PCIe in the call) */
int exa_fv_time_step_device(exa_fv_plan* plan, double* Q_dev, double dt, double h, void* stream);
/* same over a patch array of which only some entries are in use, their number known on the device only (the
 * limiter's troubled cells): the launch covers the plan's n_patches (the array's capacity) and skips every
 * patch p with slot_dev[p] < 0.  slot_dev == NULL: all patches (== exa_fv_time_step_device). */
int exa_fv_time_step_device_masked(exa_fv_plan* plan, double* Q_dev, const long* slot_dev, double dt, double h,
                                   void* stream);
/* ... with the patch centres ([n_patches][dim], entries of unused patches ignored) and the time, for term sets whose terms depend on position /
 * time (the limiter's troubled cells of such a system: the centre of a patch is the centre of its DG cell) */
int exa_fv_time_step_device_masked_at(exa_fv_plan* plan, double* Q_dev, const long* slot_dev, const double* centre_dev, double t, double dt,
                                      double h, void* stream);

/* The `exahype2::CellData` flavour of the kernel (`examples/kernel-generator.py:6-45`; `exahype/KernelBuilder.py:217-218`: the output item is
 * indexed without the halo; `Unit test/correctness_test.cpp:142`: CellData(QIn, cellCentre, cellSize, t, dt, QOut)): QIn_dev
 * [n_patches][(P+2H)^dim][n_real+n_aux] is only read, QOut_dev [n_patches][P^dim][n_real+n_aux] (exa_fv_qout_count doubles) receives
 * the updated evolved variables and a copy of the auxiliary ones.  centre_dev: [n_patches][dim] cell centres (NULL: all at the origin)
 * and t reach PDE term sets that depend on position and time (flux / maxEigenvalue / sourceTerm(Q, x, h, t, dt, ...) of
 * `Unit test/correctness_test.cpp:16-41`; generated from SymPy expressions by exahype_amd.pde_codegen); the volume centres follow
 * exahype2::fv::getVolumeCentre: centre - P h / 2 + (index + 1/2) h. */
int exa_fv_time_step_device_oop(exa_fv_plan* plan, const double* QIn_dev, double* QOut_dev, const double* centre_dev, double t,
                                double dt, double h, void* stream);
/* The in-place update WITH the patch centres and the time (same meaning as for exa_fv_time_step_device_oop): what a host driver that keeps
 * Q with halo resident (halo fill -> update -> ...) calls for term sets whose terms depend on position / time.  exa_fv_time_step_device
 * is this call with every patch centred at the origin and t = 0. */
int exa_fv_time_step_device_at(exa_fv_plan* plan, double* Q_dev, const double* centre_dev, double t, double dt, double h, void* stream);
long exa_fv_qout_count(const exa_fv_plan* plan);

/* The patch update WITH its halo fill, on HALO-LESS arrays: the plan's patches are the cells of a Cartesian grid (grid[dim] patches per axis,
 * patch index row-major) and Q_dev / QNext_dev are [n_patches][P^dim][n_real+n_aux] (exa_fv_qout_count doubles each, the layout of the
 * CellData flavour's QOut).  What the reference leaves to the caller before `time_step` -- Peano keeps patches without halo and its enclave
 * task assembles QIn with halo from the neighbours' boundary layers (`exahype/printers/CPPPrinter.py:346`; the patch loop of
 * `Unit test/correctness_test.cpp:118-174`) -- happens inside the launch: the kernel builds the patch with halo on chip (LDS), taking the states
 * beyond a patch face from the face neighbour's interior layers in Q_dev (periodic wrap; boundary_dev != NULL: on a domain face the prescribed
 * state boundary_dev[(axis * 2 + side) * (n_real + n_aux) ..]).  Q_dev is only read; QNext_dev (a different array) receives the new states --
 * a driver swaps the two per step.  No halo pass, no halo bytes in HBM.  centre_dev, t as exa_fv_time_step_device_at.
 * lambda_next_dev (device, 1 double, or NULL): receives the largest eigenvalue of the NEW states over the directions (evaluated at t + dt) --
 * the CFL scan of the NEXT step, computed on the values the kernel holds in registers instead of by a pass of its own. */
int exa_fv_grid_step_device(exa_fv_plan* plan, const double* Q_dev, double* QNext_dev, const long* grid, const double* boundary_dev,
                            const double* centre_dev, double t, double dt, double h, double* lambda_next_dev, void* stream);
/* ... with a kind per domain face, face_kind[axis * 2 + side] (host, 2 dim entries; NULL: every face periodic), and the face's data
 * face_data_dev[(axis * 2 + side) * (n_real + n_aux) ..] (device; NULL only if every face is periodic):
 *   EXA_FV_FACE_PERIODIC  the wrap neighbour's interior layers (data unused)
 *   EXA_FV_FACE_STATE     the prescribed state (the data) in every volume beyond the face
 *   EXA_FV_FACE_MIRROR    the patch's OWN interior volume at the same distance inside the face -- halo coordinate c along the axis takes
 *                         2 H - 1 - c (low) or 2 (P + H) - 1 - c (high), transverse coordinates unchanged -- every variable times its sign
 *                         (the data: +1 / -1; all +1 is an outflow face -- the Rusanov flux becomes F(q_in) -- and -1 on the normal momentum a
 *                         reflecting wall).  The products are exact: a mirror face adds no rounding.  The signs are not checked here.
 * exa_fv_grid_step_device is this call with every kind EXA_FV_FACE_PERIODIC (boundary_dev NULL) or every kind EXA_FV_FACE_STATE.  A kind
 * outside 0 .. 2 and a non-periodic kind without face_data_dev are refused. */
#define EXA_FV_FACE_PERIODIC 0
#define EXA_FV_FACE_STATE    1
#define EXA_FV_FACE_MIRROR   2
int exa_fv_grid_step_device_bc(exa_fv_plan* plan, const double* Q_dev, double* QNext_dev, const long* grid, const int* face_kind,
                               const double* face_data_dev, const double* centre_dev, double t, double dt, double h, double* lambda_next_dev,
                               void* stream);
/* The grid step of EXA_FV_MUSCL_HANCOCK plans, ONE launch on HALO-LESS arrays: Q_dev / QNext_dev [n_patches][P^dim][n_real+n_aux] as above, Q_dev
 * only read, QNext_dev (a different array) receives the new evolved variables and a copy of the auxiliary ones; patch index row-major over
 * grid[dim].  face_kind / face_data_dev mean what they mean for exa_fv_grid_step_device_bc (NULL kinds: every face periodic); there is no centre /
 * t argument, the term sets of this mode see the state alone.  The kernel assembles the window (P + 4)^dim of every patch on chip.  A window
 * entry with interior coordinates c_a in [-2, P + 2) resolves every outside axis on its own:
 *   inside the domain, or a periodic face     the neighbour patch along that axis (wrap), in-patch coordinate c_a -+ P
 *   EXA_FV_FACE_MIRROR at the patch's face    the patch's own coordinate -1 - c_a (low) / 2 P - 1 - c_a (high), every variable times its sign
 *   EXA_FV_FACE_STATE                         the face's state
 * Where two axes are outside (the edge entries: 4 points per patch in 2-D, 12 lines in 3-D) the rules compose in axis order, the later axis last,
 * as for exa_lim_project_patches_halo2 below: the state of the highest state axis wins and is multiplied by the mirror signs of later axes only;
 * without a state axis the value is the source volume -- of the diagonal patch +- e_a +- e_b inside the domain -- times all mirror signs.  That is
 * what a halo fill axis after axis over the full transverse range leaves in an array with halo (exahype_amd.solvers.fill_halos_boundary), and the
 * arithmetic is that of exa_fv_time_step_device on such an array: the results are bit-identical.  The entries no update reads are not formed.
 * lambda_next_dev (device, 1 double, or NULL): the largest eigenvalue of the NEW states over the directions, equal bit for bit to
 * exa_fv_max_eigenvalue(plan, QNext_dev, 1, ...) (a NaN survives).  halo_size of the plan is not used (the arrays have none).
 * EXA_ERR_INVALID, with a message that names the way out: a NULL plan or pointer; a plan of another mode; patch_size < 2 (the second layer would
 * belong to the neighbour's neighbour: the two-pass form serves it); QNext_dev == Q_dev; a product of grid that is not n_patches; a kind outside
 * 0 .. 2; a non-periodic kind without data; h <= 0. */
int exa_fv_grid_step_muscl_device(exa_fv_plan* plan, const double* Q_dev, double* QNext_dev, const long* grid, const int* face_kind,
                                  const double* face_data_dev, double dt, double h, double* lambda_next_dev, void* stream);
/* CFL scan of a patch array: max over the INTERIOR volumes of all patches and over the directions of the largest eigenvalue -> lambda_dev[0]
 * (device memory; one reduction launch, nothing returns to the host).  halo_less != 0: Q_dev is a halo-less array (every volume counts).
 * centre_dev / t / h: for term sets whose terms depend on position / time. */
int exa_fv_max_eigenvalue(exa_fv_plan* plan, const double* Q_dev, int halo_less, const double* centre_dev, double t, double h, double* lambda_dev,
                          void* stream);

/* ---- ADER-DG cell kernels ---------------------------------------------------- */
/* N = order + 1 nodes per axis; n_vars must equal the PDE's variable count (5 for
 * both Euler sets, any 1..8 for advection); n_picard < 0 selects N iterations,
 * 0 the single-stage variant (qbar := u, Fbar := f(u)); ncells[dim] is the local
 * Cartesian block of cells. */
int exa_dg_plan_create(int device, int dim, int N, int n_vars, int pde, int n_picard, const long* ncells,
                       exa_dg_plan** plan);
int exa_dg_plan_destroy(exa_dg_plan* plan);
/* Which stage-A kernel the plan launches where more than one is built for its (dim, N) -- today 3-D, N = 6:
 * EXA_STAGE_A_AUTO the library's choice (the faster one as measured on MI355X; the environment variable
 * EXA_STAGE_A=lds|reg, read when the plan is created, overrides it), EXA_STAGE_A_LDS the LDS-resident space-time
 * image (one workgroup per CU), EXA_STAGE_A_REG the register-resident iterate (two workgroups per CU).  Same scheme,
 * results equal to rounding.  Other (dim, N) ignore the setting. */
#define EXA_STAGE_A_AUTO 0
#define EXA_STAGE_A_LDS 1
#define EXA_STAGE_A_REG 2
int exa_dg_plan_set_stage_a(exa_dg_plan* plan, int variant);
/* Stage A of the larger orders runs as a persistent grid that fills every CU (one or two workgroups per CU, all of its LDS or
 * registers): kernels on OTHER streams -- the face packing and the RCCL transport of a halo exchange that is meant to overlap the
 * interior cells -- then only get CUs as those workgroups retire.  `workgroups` > 0 keeps the persistent grids that many workgroups
 * below the resident count, i.e. leaves that many CUs free (0, the default: fill the chip). */
int exa_dg_plan_set_stage_a_reserve(exa_dg_plan* plan, int workgroups);
/* name of the kernel exa_dg_predictor_volume launches for this plan, as a profiler prints it without the argument list
 * (static storage, valid until the next call); for bench lines and profile summaries */
const char* exa_dg_stage_a_kernel(const exa_dg_plan* plan);
long exa_dg_dof_count(const exa_dg_plan* plan);    /* doubles in u:      ncells * N^dim * n_vars */
long exa_dg_trace_count(const exa_dg_plan* plan);  /* doubles in traces: dim*2*ncells*2*n_vars*N^(dim-1) */
long exa_dg_face_count(const exa_dg_plan* plan, int d); /* doubles in one ghost/pack buffer for direction d */
/* host copies of the reference-element tables the plan uses (each may be NULL):
 * xi[N] w[N] D[N*N] Kxi[N*N] phiL[N] phiR[N] iK1[N*N] */
int exa_dg_operators(const exa_dg_plan* plan, double* xi, double* w, double* D, double* Kxi, double* phiL,
                     double* phiR, double* iK1);
/* algorithmic work of one stage-A launch (SURVEY.md 8(d) formulas), for rooflines */
int exa_dg_work(const exa_dg_plan* plan, double* flop_stage_a, double* flop_stage_b, double* bytes_stage_a,
                double* bytes_stage_b);

/* Stage A, all local cells: space-time predictor (Picard), time averages, volume
 * integral, face extrapolation.  u_dev is updated IN PLACE to u* ; trace_dev
 * receives trace[((d*2+side)*ncells + cell)*(2*n_vars*Nf) + (field*n_vars+v)*Nf + y]
 * (field 0 = time-averaged state, 1 = time-averaged normal flux; side 0 = xi=0). */
int exa_dg_predictor_volume(exa_dg_plan* plan, double* u_dev, double* trace_dev, double dt, const double* dx,
                            void* stream);
/* Stage A restricted to the cell box [lo, hi) of the local block (NULL = whole
 * block): lets a multi-GPU driver run the block's boundary shell first, start the
 * face-trace exchange, and overlap it with the interior cells. */
int exa_dg_predictor_volume_box(exa_dg_plan* plan, double* u_dev, double* trace_dev, const long* lo, const long* hi,
                                double dt, const double* dx, void* stream);
/* Stage B on the cell box [lo, hi) of the local block: Rusanov flux on the 2*dim
 * faces of every cell and the surface corrector; u_dev (holding u*) is updated
 * in place.  ghost_dev[d*2+0] / [d*2+1] are the neighbour block's traces across
 * the low / high block face in direction d, layout [transverse cell][2*n_vars*Nf]
 * (what exa_dg_pack_face produces on the neighbour); a NULL entry means periodic
 * wrap inside the block. */
int exa_dg_riemann_corrector(exa_dg_plan* plan, double* u_dev, const double* trace_dev,
                             const double* const* ghost_dev, const long* lo, const long* hi, double dt,
                             const double* dx, void* stream);
/* The same launch with the CFL scan of the NEXT step riding in it: *lambda_dev (one double, device) receives the maximum of
 * maxEigenvalue (`Unit test/Functions.h:3`) over the nodes of the box's corrected u and the directions -- what exa_dg_max_eigenvalue
 * would return for those cells, without a pass of its own over u.  lambda_dev is set to zero on the stream first.  Term sets whose
 * eigenvalue sees position / time (EXA_PDE_FLAG_XT) are refused: their scan needs the node coordinates (exa_pde_eval_device_at). */
int exa_dg_riemann_corrector_cfl(exa_dg_plan* plan, double* u_dev, const double* trace_dev,
                                 const double* const* ghost_dev, const long* lo, const long* hi, double dt,
                                 const double* dx, double* lambda_dev, void* stream);
/* Where and when: physical coordinates of the local block's origin (dim entries, NULL = 0) and the time at the start of the next
 * step.  Only term sets whose terms depend on position / time see them (pde_codegen.SympyPDE with flux(q, x, t, d) ...: the hooks
 * `Unit test/correctness_test.cpp:16-41` declares with (Q, x, h, t, dt)): stage A evaluates them at the nodes x = origin + (cell + xi_i) dx
 * and the level times t + xi_l dt, stage B at the face nodes and t + dt / 2.  Call it before every step of such a term set. */
int exa_dg_plan_set_origin_time(exa_dg_plan* plan, const double* origin, double t);
/* The step as ONE kernel ("fused" in the north star's sense; no counterpart in the reference): on the cell box
 * [lo, hi) every cell first finishes the PREVIOUS step -- Rusanov flux on its faces from the traces that step left in
 * trace_in_dev (ghost_dev as for exa_dg_riemann_corrector) and the surface corrector with dt_prev on u_dev (holding u*) --
 * and then runs stage A with dt on the result: u_dev holds the new u* afterwards, the new traces go to trace_out_dev, a
 * SECOND array (the neighbours still read trace_in_dev).  u_plain_dev, if not NULL, receives the corrected u of the previous
 * step (a snapshot).  A run of n steps is  predictor_volume, (n - 1) x corrector_predictor, riemann_corrector.
 * exa_dg_has_corrector_predictor: 1 where the plan's settings have this kernel (3-D, N = 6, register-resident stage A,
 * n_picard >= 1), else 0 -- exa_dg_corrector_predictor then returns EXA_ERR_INVALID. */
int exa_dg_has_corrector_predictor(const exa_dg_plan* plan);
int exa_dg_corrector_predictor(exa_dg_plan* plan, double* u_dev, const double* trace_in_dev, double* trace_out_dev,
                               const double* const* ghost_dev, const long* lo, const long* hi, double dt_prev, double dt,
                               const double* dx, double* u_plain_dev, void* stream);
/* Copy the outward traces of the block's boundary layer in direction d into a
 * contiguous buffer: side 0 -> L traces of the cells with c_d == 0 (to be sent
 * to the low neighbour, which uses it as ghost_dev[d*2+1]); side 1 -> R traces
 * of the cells with c_d == ncells[d]-1 (-> the high neighbour's ghost_dev[d*2+0]). */
int exa_dg_pack_face(exa_dg_plan* plan, const double* trace_dev, int d, int side, double* buf_dev, void* stream);
/* Domain boundaries: fill ghost_dev with the state beyond the block face (d, side) that a boundary condition prescribes, in the
 * layout exa_dg_pack_face writes, ghost_dev[transverse cell][2*n_vars*Nf] with the entry (field*n_vars + v)*Nf + y (field 0 =
 * time-averaged state, 1 = time-averaged normal flux; transverse cells lexicographic over the other axes, the last fastest;
 * exa_dg_face_count(plan, d) doubles).  The result is a valid ghost_dev[d*2+side] for exa_dg_riemann_corrector[_cfl] of the same step.
 *   EXA_BC_OUTFLOW    ghost = the block's own outward traces at that face (trace_dev after stage A; coeff = 2*n_vars factors, all 1:
 *                     then bit-identical to exa_dg_pack_face(plan, trace_dev, d, side)); the Rusanov flux becomes F(q_in).
 *   EXA_BC_WALL       the same gather with coeff = (s, -s): ghost state s (.) qbar_in, ghost flux -s (.) Fbar_in (s[n_vars] = +-1).  Exact
 *                     (a mirror image of the block across the face) for term sets with F_d(S q) = -S F_d(q), S = diag(s); for Euler s
 *                     negates the normal momentum, variable 1 + d.
 *   EXA_BC_DIRICHLET  ghost = sum_l w_l (q_l, F_d(q_l, x_y, t_l)) over the Gauss time levels t_l = t + xi_l dt of the step (t: the
 *                     time of exa_dg_plan_set_origin_time), with the states states_dev[transverse cell][Nf][N][n_vars] (device) at the
 *                     face nodes x_y (origin + cell size of the last exa_dg_predictor_volume); or, with states_dev NULL, the constant state
 *                     coeff[n_vars] (host) at every node and time: the ghost state is coeff itself (not sum_l w_l coeff), the ghost flux the
 *                     same sum over the levels where the term set's flux sees x or t, and one evaluation F_d(coeff) where it does not.
 *                     lambda_dev (device, may be NULL) receives max(*lambda_dev, the largest eigenvalue of those states over the directions,
 *                     nodes and levels): not zeroed here, so several faces fold into one scalar.
 * Outflow / wall take no states_dev and no lambda_dev; wrong arguments return EXA_ERR_INVALID with a message. */
#define EXA_BC_OUTFLOW 1
#define EXA_BC_WALL 2
#define EXA_BC_DIRICHLET 3
int exa_dg_boundary_ghost(exa_dg_plan* plan, const double* trace_dev, int d, int side, int kind, const double* coeff,
                          const double* states_dev, double dt, double* ghost_dev, double* lambda_dev, void* stream);
/* FV subcell limiter glue (BASELINE configs[4]): N_s = 2N-1 subcells per axis.
 * exa_lim_operators: host copies of the projection P[N_s][N] and the mean-preserving least-squares
 * reconstruction R[N][N_s].  exa_dg_project_patches: for the n cells listed in cells_dev build FV patches
 * patch_dev[n][(N_s+2)^dim][n_vars] (patch_size N_s, halo 1: interior = projected cell, face halos = adjacent
 * subcell layer of the projected face neighbours, periodic in the block) ready for exa_fv_time_step_device;
 * exa_dg_reconstruct_patches maps the patch interiors back onto the DG nodes of those cells.
 * cells_dev[i] < 0 marks an empty slot of a capacity-sized list (patch i is then neither written nor read): the list
 * can be compacted on the device without the host ever learning how many cells are troubled. */
int exa_lim_operators(const exa_dg_plan* plan, double* P, double* R);
long exa_lim_patch_count(const exa_dg_plan* plan);
int exa_dg_project_patches(exa_dg_plan* plan, const double* u_dev, const long* cells_dev, long n, double* patch_dev,
                           void* stream);
int exa_dg_reconstruct_patches(exa_dg_plan* plan, const double* patch_dev, const long* cells_dev, long n, double* u_dev,
                               void* stream);
/* Sharded grids ("a second exchange of one subcell halo layer for troubled boundary cells").
 * exa_lim_face_layers: for the cells of the block's boundary layer at face (d, side) write the projected subcell
 * layer adjacent to that face, out_dev[transverse cell][N_s^(dim-1)][n_vars] (exa_lim_face_layer_count(plan, d)
 * doubles); need_dev[transverse cell] != 0 selects the cells whose neighbour across the face is troubled (NULL: all;
 * skipped entries are left untouched).  The neighbour passes the received buffer as ghost_layers_dev[d*2+side'] of
 * its own face (side' = 1-side) to exa_dg_project_patches_ghost; NULL entries keep the periodic wrap in the block. */
long exa_lim_face_layer_count(const exa_dg_plan* plan, int d);
int exa_lim_face_layers(exa_dg_plan* plan, const double* u_dev, int d, int side, const double* need_dev, double* out_dev,
                        void* stream);
int exa_dg_project_patches_ghost(exa_dg_plan* plan, const double* u_dev, const long* cells_dev, long n, double* patch_dev,
                                 const double* const* ghost_layers_dev, void* stream);
/* Patches with halo 2, what the second-order patch update (EXA_FV_MUSCL_HANCOCK) reads: patch_dev[n][(N_s+4)^dim][n_vars]
 * (exa_lim_patch_count_halo(plan, 2) doubles per patch; halo 1 gives exa_lim_patch_count; EXA_ERR_INVALID for a NULL plan or another halo).
 * The patch is the window of the ghost-extended global subcell array -- the projected block, extended by two layers axis by axis, in axis
 * order, over the full transverse range:
 *   interior                      the projected cell
 *   face halos, two layers        the two adjacent subcell layers of the projected face neighbour
 *   edge entries                  both halo coordinates in the first layer, along the whole edge (4 points in 2-D, 12 lines in 3-D): from the
 *                                 projection of the diagonal cell c +- e_a +- e_b
 *   everything else in the halo   (a second layer together with another halo coordinate, the 3-D corners) the nearest interior value: the
 *                                 update never reads it
 * face_kind[axis * 2 + side] (host, 2 dim entries of EXA_FV_FACE_*; NULL: every face periodic) and face_data_dev[(axis * 2 + side) * n_vars ..]
 * (device; may be NULL if every face is periodic) say what lies across a face of the block, as for exa_fv_grid_step_device_bc: across an
 * EXA_FV_FACE_MIRROR face the cell itself, its subcell rows along that axis in mirrored order (halo layer 1 takes the subcell at the face, layer 2
 * the next one), every variable times its sign (the data); across an EXA_FV_FACE_STATE face the prescribed state (the data).  Where an entry lies
 * across faces of two axes the rules compose in axis order, the later axis last: a state of the later axis wins, a mirror of the later axis
 * multiplies what the earlier axis gave (a wall-wall corner: the cell's own corner subcell times both signs).  The mirror products are exact.
 * One block only: no ghost layers of neighbour blocks.  cells_dev[i] < 0: patch i is not written.
 * exa_lim_reconstruct_patches_halo: exa_dg_reconstruct_patches for patches with `halo` (1 | 2) layers -- the interior is read at offset halo;
 * halo 1 is exa_dg_reconstruct_patches itself. */
long exa_lim_patch_count_halo(const exa_dg_plan* plan, int halo);
int exa_lim_project_patches_halo2(exa_dg_plan* plan, const double* u_dev, const long* cells_dev, long n, double* patch_dev, const int* face_kind,
                                  const double* face_data_dev, void* stream);
int exa_lim_reconstruct_patches_halo(exa_dg_plan* plan, const double* patch_dev, const long* cells_dev, long n, double* u_dev, int halo,
                                     void* stream);
/* A-posteriori (MOOD) troubled-cell detection for the limiter: the DG candidate of a step is checked AFTER the step against the
 * state it started from, and the troubled cells are redone with the FV patch update from that state.  Euler variable layout:
 * density first, energy last, min(3, n_vars - 2) momenta behind the density, gamma = 1.4.  Both are one pass over u.
 * exa_lim_snapshot: copies u_dev (u^n) to u_old_dev (may be NULL: bounds only; must not be u_dev) and writes
 * bounds_dev[cell][4] = min rho, max rho, min E, max E over the cell's nodes.
 * exa_lim_detect: mask_dev[cell] (one byte per cell) = 1 if the candidate u_cand_dev is troubled in that cell, else 0:
 *   (a) a value at a node is not finite, or rho <= floor or p <= floor at a node, p = 0.4 (E - |m|^2 / (2 rho)) (a NaN counts as troubled);
 *   (b) relaxed discrete maximum principle on rho and on E: with lo / hi the minimum / maximum of bounds_dev over the cell and its
 *       2*dim face neighbours and delta = max(d0, eps (hi - lo)), the candidate's nodal maximum exceeds hi + delta or its nodal
 *       minimum falls below lo - delta.
 * face_kind[d*2+side] (host, 2*dim entries, NULL = all periodic) says what lies across the block face (d, side):
 * EXA_LIM_FACE_PERIODIC the periodic wrap inside the block; EXA_LIM_FACE_GHOST the neighbour block, whose boundary layer's bounds
 * are in ghost_bounds_dev[d*2+side][transverse cell][4] (transverse cells lexicographic over the other axes, the last fastest);
 * EXA_LIM_FACE_NONE a domain face with a boundary condition: no neighbour, the cell's own bounds.  ghost_bounds_dev may be NULL
 * if no face is EXA_LIM_FACE_GHOST.  min / max are exact: the mask does not depend on the order of the reductions.
 * A registered term set with EXA_PDE_FLAG_ADMISSIBLE (pde_codegen.SympyPDE(admissible=..., dmp=...)) replaces the Euler layout by its own
 * criterion; both entries then dispatch to kernels in its side library, same signatures:
 *   (a) a value at a node is not finite, or !(g_k(q) > floor) for one of its K_ADM (0..4) admissibility expressions g_k (IEEE arithmetic);
 *   (b) the relaxed discrete maximum principle as above on each of its K_DMP (0..4) watched variables v_0, v_1, ... in the order given:
 *       bounds_dev[cell][2 K_DMP] = min v_0, max v_0, min v_1, ..., and ghost_bounds_dev[d*2+side][transverse cell][2 K_DMP].
 * With K_DMP = 0 nothing is watched: no bounds are written or read (bounds_dev and the ghost bounds may be NULL), (a) alone decides.
 * Such a term set may have one variable; without the flag exa_lim_detect refuses n_vars < 2 (it needs a density and an energy).
 * exa_lim_bounds_count: doubles per cell of bounds_dev (and per transverse cell of the ghost bounds): 4 without the flag, 2 K_DMP with
 * it, 0 for a NULL plan. */
long exa_lim_bounds_count(const exa_dg_plan* plan);
#define EXA_LIM_FACE_PERIODIC 0
#define EXA_LIM_FACE_GHOST 1
#define EXA_LIM_FACE_NONE 2
int exa_lim_snapshot(exa_dg_plan* plan, const double* u_dev, double* u_old_dev, double* bounds_dev, void* stream);
int exa_lim_detect(exa_dg_plan* plan, const double* u_cand_dev, const double* bounds_dev, const double* const* ghost_bounds_dev,
                   const int* face_kind, double d0, double eps, double floor, unsigned char* mask_dev, void* stream);
/* Conservative DG / FV interface for the a-posteriori limiter.  A troubled cell is redone with the FV patch update, its untroubled
 * face neighbour keeps the DG corrector: on their common face the two used different fluxes.  Served: the built-in Euler (5 variables)
 * and advection (1 variable) term sets, and a registered term set with EXA_PDE_FLAG_CONSERVATIVE
 * (pde_codegen.SympyPDE(conservative_interface=True)): both entries then dispatch to kernels in its side library, same arithmetic with
 * its flux and eigenvalue (a source term does not enter a face flux).  EXA_PDE_FLAG_XT / EXA_PDE_FLAG_NCP term sets and registered term
 * sets without the flag return EXA_ERR_INVALID; so does a variable count / order whose kernel exceeds the 64 KB of LDS a workgroup may
 * declare (3-D N = 8 from 24 variables).  -1 slots are skipped.
 * exa_lim_face_flux: BEFORE the in-place FV update of the patches (exa_fv_time_step_device overwrites their boundary layers): for each
 *   listed patch and each of its 2*dim faces the corrected-mode Rusanov flux g = (f_d(Q-) + f_d(Q+)) / 2 - max(l_d(Q-), l_d(Q+)) (Q+ - Q-) / 2
 *   between the boundary layer and the halo layer on the N_s^(dim-1) subfaces (Q-: the lower index along d), brought to the N^(dim-1) face
 *   nodes with the reconstruction operator, (R x R) g, which keeps the face mean: fvflux_dev[slot][d*2+side][var][face node],
 *   exa_lim_face_flux_count(plan) doubles per slot, the [var][node] order of one field of the trace array.
 * exa_lim_interface_correct: AFTER exa_dg_reconstruct_patches, with the trace array of the step still intact: for every face (d, side) of a
 *   listed cell T whose neighbour D across it has mask_dev[D] == 0 (the CUMULATIVE troubled mask of the step, T's own flag included), the DG
 *   face flux F* = (F- + F+) / 2 - s (q+ - q-) / 2, s the largest eigenvalue over all nodes of the face, is recomputed as the Riemann /
 *   corrector pass did, and D takes the corrector's lift of dF = fvflux - F*:  u_D -= dt/dx_d phiR_i / w_i dF (its upper face),
 *   u_D += dt/dx_d phiL_i / w_i dF (its lower face) -- its mean changes by what T's mean changed, with the opposite sign.
 *   face_kind as for exa_lim_detect: EXA_LIM_FACE_NONE faces of the block have no neighbour and are left alone, EXA_LIM_FACE_GHOST is
 *   refused (the exchange of face fluxes between blocks is not built).  One launch per (axis, side): no atomics, deterministic. */
long exa_lim_face_flux_count(const exa_dg_plan* plan);
int exa_lim_face_flux(exa_dg_plan* plan, const double* patch_dev, const long* cells_dev, long n, double* fvflux_dev, void* stream);
int exa_lim_interface_correct(exa_dg_plan* plan, double* u_dev, const double* trace_dev, const long* cells_dev, long n,
                              const unsigned char* mask_dev, const int* face_kind, const double* fvflux_dev, double dt, const double* dx,
                              void* stream);
/* max over all cells/nodes/directions of maxEigenvalue (for a CFL time step);
 * result is written to *lambda_dev (one double, device). */
int exa_dg_max_eigenvalue(exa_dg_plan* plan, const double* u_dev, double* lambda_dev, void* stream);
/* Single-stage scheme (n_picard = 0) in 2-D, alternative to predictor_volume + riemann_corrector on a periodic single
 * block: one fused launch per step with the traces kept on chip (exa_dg_fused.hpp); u_in_dev != u_out_dev (ping-pong).
 * Moves ~1.9 KB instead of 6.4 KB per cell and step through HBM at p = 3: 0.22 ms against 0.28 ms on 512 x 512 cells.
 * exa_dg_has_fused_step: 1 if the plan has this path. */
int exa_dg_has_fused_step(const exa_dg_plan* plan);
int exa_dg_step_fused(exa_dg_plan* plan, const double* u_in_dev, double* u_out_dev, double dt, const double* dx, void* stream);
/* convenience: n_steps full steps on a periodic single block (stage A + stage B) */
int exa_dg_step_periodic(exa_dg_plan* plan, double* u_dev, double* trace_dev, double dt, const double* dx,
                         int n_steps, void* stream);
/* host AoS convenience (allocates/frees HBM internally): one periodic step */
int exa_dg_step_host(exa_dg_plan* plan, double* u_host, double dt, const double* dx, int n_steps);

#ifdef __cplusplus
}
#endif
#endif

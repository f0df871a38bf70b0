// Conservative DG / FV interface of the a-posteriori subcell limiter: the two kernels and their launch helpers, templates over the term set.
// limiter.hip instantiates them for the built-in Euler and advection sets; a generated term set that asks for the interface
// (pde_codegen.SympyPDE(conservative_interface=True); exa_pde.hpp pde_has_conservative_interface) instantiates them in its side library
// (lim_conserve_user.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "exa_launch.hpp"
#include "exa_lim_detect.hpp"      // EXA_LIM_CASES
#include "exa_pde.hpp"

// F* must be stage B's to rounding: stage B (exa_dg_kernels.hpp) takes the IEEE eigenvalue member `maxeig`, which is this macro's default here
#ifndef EXA_STAGE_B_FAST_EIG
#define EXA_STAGE_B_FAST_EIG 0
#endif

namespace exa {

// ------------------------------------------------------------------------------------------------------------------
// Conservative DG / FV interface.  A troubled cell T takes the FV patch update, its untroubled face neighbour D keeps
// the DG corrector: the two used different fluxes on their common face.  Two small latency-bound kernels close the gap:
//   limiter_face_flux_kernel          BEFORE the in-place FV update: per (slot, face) the corrected-mode Rusanov flux between the patch's
//                                     boundary layer and its halo layer on the N_s^(dim-1) subfaces (minus state = lower index along d),
//                                     brought to the N^(dim-1) face nodes with the mean-preserving reconstruction, (R x R) g
//                                     -> fvflux[slot][d*2+side][var][face node], the order of one field of the trace array
//   limiter_interface_correct_kernel  AFTER the reconstruction, one launch per (axis, side): the face (d, side) of every listed cell T whose
//                                     neighbour D across it is not in the cumulative mask.  F* is recomputed from the step's traces as stage B
//                                     did (s = maximum eigenvalue over ALL nodes of the face), and D takes the corrector's own lift of
//                                     F~ - F*: its mean changes by exactly what T's mean changed, with the opposite sign.  Within one launch
//                                     a cell D is written by at most one workgroup: deterministic, no floating-point atomics.
// One workgroup per slot (x face); empty slots (-1) return at once.
// ------------------------------------------------------------------------------------------------------------------
struct LimLift { double l[MAXN], r[MAXN]; };        // phiL_i / w_i, phiR_i / w_i

template <int DIM, int N, class PDE>
__global__ void __launch_bounds__(256)
limiter_face_flux_kernel(const double* __restrict__ patch, const long* __restrict__ cells, double* __restrict__ fvflux,
                         const double* __restrict__ R) {
    constexpr int NV = PDE::NV, Ns = 2 * N - 1, S = Ns + 2;
    constexpr int SS = DIM == 3 ? S * S * S : S * S, LAYER = DIM == 3 ? Ns * Ns : Ns, NF = DIM == 3 ? N * N : N;
    __shared__ double G[LAYER * NV];
    __shared__ double H[DIM == 3 ? N * Ns * NV : 1];
    __shared__ double Rsh[N * Ns];
    const int slot = blockIdx.x / (2 * DIM), f = blockIdx.x - slot * (2 * DIM);
    if (cells[slot] < 0) return;                                   // empty slot
    const int d = f >> 1, side = f & 1;
    const double* pt = patch + (long)slot * SS * NV;
    for (int t = threadIdx.x; t < N * Ns; t += blockDim.x) Rsh[t] = R[t];
    int st[3] = {DIM == 3 ? S * S : S, DIM == 3 ? S : 1, 1};       // patch strides per axis
    for (int t = threadIdx.x; t < LAYER; t += blockDim.x) {
        // t enumerates the transverse subcells (axes != d, lexicographic)
        int r = t, flat = 0;
        for (int b = DIM - 1; b >= 0; b--) {
            if (b == d) continue;
            flat += (r % Ns + 1) * st[b];
            r /= Ns;
        }
        const double* pm = pt + (long)(flat + (side ? Ns : 0) * st[d]) * NV;     // lower index along d
        const double* pp = pm + (long)st[d] * NV;
        double qm[NV], qp[NV], Fm[NV], Fp[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) { qm[v] = pm[v]; qp[v] = pp[v]; Fm[v] = 0.0; Fp[v] = 0.0; }
        PDE::flux_rt(qm, d, Fm);
        PDE::flux_rt(qp, d, Fp);
        const double lam = fmax(PDE::maxeig(qm, d), PDE::maxeig(qp, d));
#pragma unroll
        for (int v = 0; v < NV; v++) G[t * NV + v] = 0.5 * (Fm[v] + Fp[v]) - 0.5 * lam * (qp[v] - qm[v]);
    }
    __syncthreads();
    double* out = fvflux + (long)blockIdx.x * (NV * NF);
    if constexpr (DIM == 2) {
        for (int t = threadIdx.x; t < N * NV; t += blockDim.x) {
            const int y = t / NV, v = t - y * NV;
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < Ns; c++) acc += Rsh[y * Ns + c] * G[c * NV + v];
            out[v * NF + y] = acc;
        }
    } else {
        for (int t = threadIdx.x; t < N * Ns * NV; t += blockDim.x) {          // first transverse axis: [Ns][Ns] -> [N][Ns]
            const int y0 = t / (Ns * NV), r = t - y0 * (Ns * NV);
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < Ns; c++) acc += Rsh[y0 * Ns + c] * G[c * (Ns * NV) + r];
            H[t] = acc;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < N * N * NV; t += blockDim.x) {           // second: [N][Ns] -> [N][N]
            const int y0 = t / (N * NV), r = t - y0 * (N * NV), y1 = r / NV, v = r - y1 * NV;
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < Ns; c++) acc += Rsh[y1 * Ns + c] * H[(y0 * Ns + c) * NV + v];
            out[v * NF + y0 * N + y1] = acc;
        }
    }
}

template <int DIM, int N, class PDE>
__global__ void __launch_bounds__(256)
limiter_interface_correct_kernel(long nc0, long nc1, long nc2, double* __restrict__ u, const double* __restrict__ trace,
                                 const long* __restrict__ cells, const unsigned char* __restrict__ mask, int d, int side, int kind,
                                 const double* __restrict__ fvflux, double scale, LimLift lift) {
    constexpr int NV = PDE::NV, NF = DIM == 3 ? N * N : N, NN = NF * N, TS = 2 * NV * NF;
    static_assert(NF <= 64, "a face must fit one wavefront");
    __shared__ double dF[NF * NV];
    __shared__ double cf[N];
    const long T = cells[blockIdx.x];
    if (T < 0) return;                                             // empty slot
    const long nc[3] = {nc0, nc1, DIM == 3 ? nc2 : 1};
    const long ncells = nc[0] * nc[1] * nc[2];
    long cc[3];
    { long b = T; cc[2] = b % nc[2]; b /= nc[2]; cc[1] = b % nc[1]; cc[0] = b / nc[1]; }
    if (kind != 0 && cc[d] == (side ? nc[d] - 1 : 0)) return;      // a domain face with a boundary condition: no neighbour
    long nb[3] = {cc[0], cc[1], cc[2]};
    nb[d] = (nb[d] + (side ? 1 : nc[d] - 1)) % nc[d];
    const long D = (nb[0] * nc[1] + nb[1]) * nc[2] + nb[2];
    if (mask[D]) return;                                           // FV on both sides (or T itself, one cell along d): nothing to do
    if (threadIdx.x < 64) {
        const int y = threadIdx.x;
        // minus = the lower cell's R trace, plus = the upper cell's L trace
        const double* pm = trace + (((long)d * 2 + 1) * ncells + (side ? T : D)) * TS;
        const double* pp = trace + (((long)d * 2 + 0) * ncells + (side ? D : T)) * TS;
        double qm[NV], qp[NV], Fm[NV], Fp[NV];
        double lam = 0.0;
        if (y < NF) {
#pragma unroll
            for (int v = 0; v < NV; v++) {
                qm[v] = pm[v * NF + y];
                qp[v] = pp[v * NF + y];
                Fm[v] = pm[(NV + v) * NF + y];
                Fp[v] = pp[(NV + v) * NF + y];
            }
#if EXA_STAGE_B_FAST_EIG
            lam = fmax(PDE::maxeig_fast(qm, d), PDE::maxeig_fast(qp, d));
#else
            lam = fmax(PDE::maxeig(qm, d), PDE::maxeig(qp, d));
#endif
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lam = fmax(lam, __shfl_xor(lam, o, 64));       // the face-wide maximum (inactive lanes carry 0)
        if (y < NF) {
            const double* ft = fvflux + ((long)blockIdx.x * (2 * DIM) + d * 2 + side) * (NV * NF);
#pragma unroll
            for (int v = 0; v < NV; v++) dF[y * NV + v] = ft[v * NF + y] - (0.5 * (Fm[v] + Fp[v]) - 0.5 * lam * (qp[v] - qm[v]));
        }
        // T's upper face is D's lower face: u_D += dt/dx phiL_i / w_i dF; T's lower face is D's upper face: u_D -= dt/dx phiR_i / w_i dF
        if (y < N) cf[y] = side ? scale * lift.l[y] : -scale * lift.r[y];
    }
    __syncthreads();
    double* ud = u + D * (long)(NN * NV);
    for (int e = threadIdx.x; e < NN * NV; e += blockDim.x) {
        const int n = e / NV, v = e - n * NV;
        int i, y;
        if constexpr (DIM == 3) {
            const int a = n / (N * N), b = (n / N) % N, c = n % N;
            i = d == 0 ? a : (d == 1 ? b : c);
            y = d == 0 ? b * N + c : (d == 1 ? a * N + c : a * N + b);
        } else {
            i = d == 0 ? n / N : n % N;
            y = d == 0 ? n % N : n / N;
        }
        ud[e] += cf[i] * dF[y * NV + v];
    }
}

// Static LDS of limiter_face_flux_kernel: G, H and Rsh.  3-D N = 8: (Ns^2 + N Ns) NV + N Ns doubles = 2760 NV + 960 bytes, past the 64 KB a
// workgroup may declare from NV = 24 -- such an instantiation is not compiled (the unit must still build) and the launch says so.
template <int DIM, int N, int NV> constexpr long lim_face_flux_lds() {
    constexpr long Ns = 2 * N - 1;
    return 8 * ((DIM == 3 ? Ns * Ns : Ns) * NV + (DIM == 3 ? N * Ns * NV : 1) + N * Ns);
}
template <int DIM, int N, int NV> constexpr long lim_interface_correct_lds() { return 8 * ((DIM == 3 ? N * N : N) * NV + N); }
constexpr long LIM_LDS_MAX = 65536;

// DIM = 3 exists only for term sets with MAXDIM >= 3: a 2-D set's members are never called with d >= MAXDIM
template <int DIM, int N, class PDE>
static int lim_face_flux_one(const double* patch, const long* cells, long n, double* fvflux, const double* Rdev, hipStream_t s) {
    if constexpr (DIM > PDE::MAXDIM) {
        set_error("limiter: dim = %d is not built for a term set of %d dimensions", DIM, PDE::MAXDIM);
        return -1;
    } else if constexpr (lim_face_flux_lds<DIM, N, PDE::NV>() > LIM_LDS_MAX) {
        set_error("limiter_face_flux: NV = %d at N = %d (dim %d) needs %ld bytes of LDS, a workgroup has %ld", PDE::NV, N, DIM,
                  lim_face_flux_lds<DIM, N, PDE::NV>(), LIM_LDS_MAX);
        return -1;
    } else {
        hipLaunchKernelGGL((limiter_face_flux_kernel<DIM, N, PDE>), dim3((unsigned)(n * 2 * DIM)), dim3(256), 0, s, patch, cells, fvflux, Rdev);
        return 0;
    }
}

template <class PDE>
static int lim_face_flux_pde(int dim, int N, const double* patch, const long* cells, long n, double* fvflux, const double* Rdev, hipStream_t s) {
    switch (N) {
#define X(NN_)                                                                                                  \
    case NN_:                                                                                                   \
        return dim == 2 ? lim_face_flux_one<2, NN_, PDE>(patch, cells, n, fvflux, Rdev, s)                      \
                        : lim_face_flux_one<3, NN_, PDE>(patch, cells, n, fvflux, Rdev, s);
        EXA_LIM_CASES(X)
#undef X
    default: set_error("limiter: N = %d is not built", N); return -1;
    }
}

template <int DIM, int N, class PDE>
static int lim_interface_correct_one(const long* nc, double* u, const double* trace, const long* cells, long n, const unsigned char* mask, int d,
                                     int side, int kind, const double* fvflux, double scale, const LimLift& lift, hipStream_t s) {
    if constexpr (DIM > PDE::MAXDIM) {
        set_error("limiter: dim = %d is not built for a term set of %d dimensions", DIM, PDE::MAXDIM);
        return -1;
    } else if constexpr (lim_interface_correct_lds<DIM, N, PDE::NV>() > LIM_LDS_MAX) {
        set_error("limiter_interface_correct: NV = %d at N = %d (dim %d) needs %ld bytes of LDS, a workgroup has %ld", PDE::NV, N, DIM,
                  lim_interface_correct_lds<DIM, N, PDE::NV>(), LIM_LDS_MAX);
        return -1;
    } else {
        hipLaunchKernelGGL((limiter_interface_correct_kernel<DIM, N, PDE>), dim3((unsigned)n), dim3(256), 0, s, nc[0], nc[1], DIM == 3 ? nc[2] : 1, u,
                           trace, cells, mask, d, side, kind, fvflux, scale, lift);
        return 0;
    }
}

template <class PDE>
static int lim_interface_correct_pde(int dim, int N, const long* nc, double* u, const double* trace, const long* cells, long n,
                                     const unsigned char* mask, int d, int side, int kind, const double* fvflux, double scale,
                                     const LimLift& lift, hipStream_t s) {
    switch (N) {
#define X(NN_)                                                                                                                            \
    case NN_:                                                                                                                             \
        return dim == 2 ? lim_interface_correct_one<2, NN_, PDE>(nc, u, trace, cells, n, mask, d, side, kind, fvflux, scale, lift, s)     \
                        : lim_interface_correct_one<3, NN_, PDE>(nc, u, trace, cells, n, mask, d, side, kind, fvflux, scale, lift, s);
        EXA_LIM_CASES(X)
#undef X
    default: set_error("limiter: N = %d is not built", N); return -1;
    }
}

// exa_lim_face_flux for one term set: n slots (empty ones -1)
template <class PDE>
static int lim_face_flux_all(int dim, int N, const double* patch, const long* cells, long n, double* fvflux, const double* Rdev, hipStream_t s) {
    if (n <= 0) return 0;
    const int rc = lim_face_flux_pde<PDE>(dim, N, patch, cells, n, fvflux, Rdev, s);
    if (rc) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("limiter_face_flux launch: %s", hipGetErrorString(e)); return -2; }
    return 0;
}

// exa_lim_interface_correct for one term set.  One launch per (axis, side): a cell can have troubled neighbours on several faces (with two
// cells along an axis the same one on both)
template <class PDE>
static int lim_interface_correct_all(int dim, int N, const long* nc, double* u, const double* trace, const long* cells, long n,
                                     const unsigned char* mask, const int* kinds, const double* fvflux, double dt, const double* dx,
                                     const double* w, const double* phiL, const double* phiR, hipStream_t s) {
    if (n <= 0) return 0;
    LimLift lift{};
    for (int i = 0; i < N; i++) { lift.l[i] = phiL[i] / w[i]; lift.r[i] = phiR[i] / w[i]; }
    for (int d = 0; d < dim; d++)
        for (int side = 0; side < 2; side++) {
            const int kind = kinds ? kinds[d * 2 + side] : 0;
            const int rc = lim_interface_correct_pde<PDE>(dim, N, nc, u, trace, cells, n, mask, d, side, kind, fvflux, dt / dx[d], lift, s);
            if (rc) return rc;
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) { set_error("limiter_interface_correct launch: %s", hipGetErrorString(e)); return -2; }
        }
    return 0;
}

// this unit's slice of a term set's table (exa_launch.hpp PdeKernels)
template <class PDE>
static void lim_conserve_fill(PdeKernels* k) {
    k->lim_face_flux = lim_face_flux_all<PDE>;
    k->lim_interface_correct = lim_interface_correct_all<PDE>;
}

}  // namespace exa

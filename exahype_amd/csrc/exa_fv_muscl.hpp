// Second-order MUSCL-Hancock patch update for gfx950 (EXA_FV_MUSCL_HANCOCK) -- the templates; fv_muscl.hip instantiates them
// for the built-in term sets, fv_muscl_user.hip for a generated one (pde_codegen.SympyPDE(muscl_hancock=True)).
//
// The scheme, on a patch array Q[patch][S..][V] (S = P + 2 H, H >= 2), evolved variables v < m, r = dt / h:
//   1. slopes       s_e(c) = minmod(Q_c - Q_{c-e}, Q_{c+e} - Q_c) for every axis e, for the interior volumes and their face neighbours (the "plus
//                   shape").  minmod decides by the signs of its arguments (a NaN difference: slope 0); auxiliary variables have slope 0.
//   2. predictor    delta_c = -(r/2) sum_e [f_e(Q_c + s_e/2) - f_e(Q_c - s_e/2)]                                 (unsplit, all axes)
//   3. face states  w_c^{+-d} = (Q_c +- s_d(c)/2) + delta_c
//   4. face flux    F* = (f_d(w_L) + f_d(w_R))/2 - max(l_d(w_L), l_d(w_R))/2 (w_R - w_L)     (flux_rt / maxeig: IEEE division and square root)
//   5. update       Q_c <- Q_c - r sum_d (F*_{c+1/2,d} - F*_{c-1/2,d}), interior volumes, evolved variables; everything else stays as it is.
// An interior update reads Q at c +- e_d, c +- 2 e_d and c +- e_d +- e_e (d != e): the two halo layers next to the interior INCLUDING the edge entries
// (layer 1 along two axes); never (+-2, +-1), the 3-D corners or a layer beyond the second.
//
// One workgroup owns `ppb` patches.  LDS plan: the window T = P + 4 of every patch (its interior and the two halo layers next to it, all V
// variables; H = 2: the whole patch, one contiguous block of HBM) and the predictor's delta over (P + 2)^DIM x m.  Phase 1: one task per
// plus-shape volume -> delta.  Barrier.  Phase 2: one task per interior volume rebuilds its 2 DIM + 1 slopes per axis from the window (the very
// function phase 1 ran: the same bits), takes the neighbours' delta from LDS, evaluates its 2 DIM face fluxes and stores the new state.  Both
// sides of a face evaluate fv_muscl_face on the same two states, so the flux a volume loses is bit for bit the one its neighbour gains.  The
// window is complete before the first store, so in place is safe; the unit is compiled without FMA contraction like the Rusanov unit.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "exa_launch.hpp"
#include "exa_pde.hpp"

namespace exa {

constexpr int FVM_MAXV = 8;
typedef double fvm_v2d __attribute__((ext_vector_type(2)));

template <int I, int E, class F> __device__ __forceinline__ void static_for_muscl(F&& f) {
    if constexpr (I < E) {
        f(std::integral_constant<int, I>{});
        static_for_muscl<I + 1, E>(f);
    }
}

__device__ __forceinline__ double fv_minmod(double a, double b) {
    if (a > 0.0 && b > 0.0) return a < b ? a : b;
    if (a < 0.0 && b < 0.0) return a > b ? a : b;
    return 0.0;                                                   // opposite signs, a zero, a NaN
}

// slopes of the evolved variables of the volume at q (window image) along the axis whose neighbours lie `st` doubles away
__device__ __forceinline__ void fv_muscl_slope(const double* q, int st, int m, double (&s)[FVM_MAXV]) {
#pragma unroll
    for (int v = 0; v < FVM_MAXV; v++) s[v] = v < m ? fv_minmod(q[v] - q[v - st], q[v + st] - q[v]) : 0.0;
}

// Rusanov flux of (wL, wR) along D
template <class PDE, int D>
__device__ __forceinline__ void fv_muscl_face(const double (&wL)[FVM_MAXV], const double (&wR)[FVM_MAXV], int m, double (&F)[FVM_MAXV]) {
    double fL[FVM_MAXV], fR[FVM_MAXV];
#pragma unroll
    for (int v = 0; v < FVM_MAXV; v++) { fL[v] = 0.0; fR[v] = 0.0; }
    PDE::flux_rt(wL, D, fL);
    PDE::flux_rt(wR, D, fR);
    const double hl = 0.5 * fmax(PDE::maxeig(wL, D), PDE::maxeig(wR, D));
#pragma unroll
    for (int v = 0; v < FVM_MAXV; v++) F[v] = v < m ? 0.5 * (fL[v] + fR[v]) - hl * (wR[v] - wL[v]) : 0.0;
}

template <int DIM> __host__ __device__ constexpr int fvm_pow(int b) { return DIM == 3 ? b * b * b : b * b; }

template <int DIM, class PDE, int NT>
__global__ void __launch_bounds__(NT)
fv_muscl_kernel(double* __restrict__ Q, double* __restrict__ out, const long* __restrict__ slot, int P, int H, int m, int V, double r,
                long n_patches, int ppb) {
    extern __shared__ __attribute__((aligned(16))) double fvm_lds[];
    const int S = P + 2 * H, T = P + 4, D = P + 2, off = H - 2;
    const int tvol = fvm_pow<DIM>(T), dvol = fvm_pow<DIM>(D), ncell = fvm_pow<DIM>(P);
    const long svol = DIM == 3 ? (long)S * S * S : (long)S * S;
    double* img = fvm_lds;                                        // [patch slot][T^DIM][V]
    double* del = fvm_lds + (long)ppb * tvol * V;                 // [patch slot][(P + 2)^DIM][m]
    const long first = (long)blockIdx.x * ppb;
    const int np = (int)(n_patches - first < ppb ? n_patches - first : ppb);
    const int tid = (int)threadIdx.x;

    // ---- stage the windows
    const double* src = Q + first * svol * V;
    if (off == 0) {                                               // the window is the patch: one contiguous block
        const int total = np * tvol * V;
        if ((reinterpret_cast<unsigned long long>(src) & 15) == 0) {
            const fvm_v2d* s2 = reinterpret_cast<const fvm_v2d*>(src);
            fvm_v2d* d2 = reinterpret_cast<fvm_v2d*>(img);
            for (int i = tid; i < total / 2; i += NT) d2[i] = s2[i];
            if ((total & 1) && tid == 0) img[total - 1] = src[total - 1];
        } else {
            for (int i = tid; i < total; i += NT) img[i] = src[i];
        }
    } else {                                                      // H > 2: rows of T V contiguous doubles
        const int row = T * V, rows_pp = tvol / T, nrow = np * rows_pp;
        for (int i = tid; i < nrow * row; i += NT) {
            const int rw = i / row, x = i - rw * row;
            const int pp = rw / rows_pp, rr = rw - pp * rows_pp;
            const long c = DIM == 3 ? ((long)(rr / T + off) * S + (rr % T + off)) * S + off : (long)(rr + off) * S + off;
            img[i] = src[(pp * svol + c) * V + x];
        }
    }
    __syncthreads();

    int tst[3], dst[3];                                           // volume strides of the window and of delta's box
    if constexpr (DIM == 3) { tst[0] = T * T; tst[1] = T; tst[2] = 1; dst[0] = D * D; dst[1] = D; dst[2] = 1; }
    else { tst[0] = T; tst[1] = 1; tst[2] = 0; dst[0] = D; dst[1] = 1; dst[2] = 0; }
    const double hr = 0.5 * r;

    // ---- phase 1: delta of every plus-shape volume (box coordinates 0 .. P + 1, at most one of them outside 1 .. P)
    for (int i = tid; i < np * dvol; i += NT) {
        const int pp = i / dvol, dc = i - pp * dvol;
        if (slot && slot[first + pp] < 0) continue;
        int co[3];
        if constexpr (DIM == 3) { co[0] = dc / (D * D); co[1] = (dc / D) % D; co[2] = dc % D; }
        else { co[0] = dc / D; co[1] = dc % D; co[2] = 1; }
        int outside = 0, tc = 0;
#pragma unroll
        for (int a = 0; a < DIM; a++) { outside += (co[a] < 1 || co[a] > P) ? 1 : 0; tc += (co[a] + 1) * tst[a]; }
        if (outside > 1) continue;
        const double* q = img + ((long)pp * tvol + tc) * V;
        double qc[FVM_MAXV], sum[FVM_MAXV];
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) { qc[v] = v < m ? q[v] : 0.0; sum[v] = 0.0; }
        static_for_muscl<0, DIM>([&](auto ee) {
            constexpr int e = decltype(ee)::value;
            double s[FVM_MAXV], wp[FVM_MAXV], wm[FVM_MAXV], fp[FVM_MAXV], fm[FVM_MAXV];
            fv_muscl_slope(q, tst[e] * V, m, s);
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++) { wp[v] = qc[v] + 0.5 * s[v]; wm[v] = qc[v] - 0.5 * s[v]; fp[v] = 0.0; fm[v] = 0.0; }
            PDE::flux_rt(wp, e, fp);
            PDE::flux_rt(wm, e, fm);
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++) sum[v] = e == 0 ? fp[v] - fm[v] : sum[v] + (fp[v] - fm[v]);
        });
        double* dl = del + ((long)pp * dvol + dc) * m;
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++)
            if (v < m) dl[v] = -hr * sum[v];
    }
    __syncthreads();

    // ---- phase 2: the interior volumes
    for (int i = tid; i < np * ncell; i += NT) {
        const int pp = i / ncell, id = i - pp * ncell;
        const long patch = first + pp;
        if (slot && slot[patch] < 0) continue;
        int co[3];                                                // interior coordinates 0 .. P - 1
        if constexpr (DIM == 3) { co[0] = id / (P * P); co[1] = (id / P) % P; co[2] = id % P; }
        else { co[0] = id / P; co[1] = id % P; co[2] = 0; }
        int tc = 0, dc = 0;
#pragma unroll
        for (int a = 0; a < DIM; a++) { tc += (co[a] + 2) * tst[a]; dc += (co[a] + 1) * dst[a]; }
        const double* q = img + ((long)pp * tvol + tc) * V;
        const double* dl = del + ((long)pp * dvol + dc) * m;
        double qc[FVM_MAXV], dC[FVM_MAXV], acc[FVM_MAXV];
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) { qc[v] = v < m ? q[v] : 0.0; dC[v] = v < m ? dl[v] : 0.0; acc[v] = 0.0; }
        static_for_muscl<0, DIM>([&](auto dd) {
            constexpr int d = decltype(dd)::value;
            const int qs = tst[d] * V, ds = dst[d] * m;
            double sC[FVM_MAXV], sN[FVM_MAXV], wCp[FVM_MAXV], wCm[FVM_MAXV], wN[FVM_MAXV], Fp[FVM_MAXV], Fm[FVM_MAXV];
            fv_muscl_slope(q, qs, m, sC);
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++) { wCp[v] = (qc[v] + 0.5 * sC[v]) + dC[v]; wCm[v] = (qc[v] - 0.5 * sC[v]) + dC[v]; }
            fv_muscl_slope(q + qs, qs, m, sN);                    // the plus-side neighbour's minus state
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++) wN[v] = v < m ? (q[qs + v] - 0.5 * sN[v]) + dl[ds + v] : 0.0;
            fv_muscl_face<PDE, d>(wCp, wN, m, Fp);
            fv_muscl_slope(q - qs, qs, m, sN);                    // the minus-side neighbour's plus state
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++) wN[v] = v < m ? (q[v - qs] + 0.5 * sN[v]) + dl[v - ds] : 0.0;
            fv_muscl_face<PDE, d>(wN, wCm, m, Fm);
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++) acc[v] = d == 0 ? Fp[v] - Fm[v] : acc[v] + (Fp[v] - Fm[v]);
        });
        if (out) {                                                // halo-less QOut [patch][P^DIM][V]: auxiliary variables copied
            double* o = out + (patch * ncell + id) * V;
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++)
                if (v < m) o[v] = qc[v] - r * acc[v];
            for (int v = m; v < V; v++) o[v] = q[v];
        } else {
            const long c = DIM == 3 ? ((long)(co[0] + H) * S + (co[1] + H)) * S + (co[2] + H) : (long)(co[0] + H) * S + (co[1] + H);
            double* o = Q + (patch * svol + c) * V;
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++)
                if (v < m) o[v] = qc[v] - r * acc[v];
        }
    }
}

// launch for one (DIM, PDE); the plan (patches per workgroup, LDS bytes) is fv_muscl_plan's, which exa_fv_plan_create has checked
template <int DIM, class PDE>
int fv_muscl_run(int P, int H, int m, int V, long n_patches, double* Q, double dt, double h, const long* slot, hipStream_t s, double* out) {
    FvMusclPlan pl;
    if (!fv_muscl_plan(DIM, P, m, V, &pl)) {
        set_error("MUSCL-Hancock: the patch needs %zu B of LDS, %zu B are available", pl.lds, FV_MUSCL_LDS_AVAILABLE);
        return -1;
    }
    if (H < 2) { set_error("MUSCL-Hancock reads two halo layers"); return -1; }
    if (m > FVM_MAXV) { set_error("n_real = %d exceeds %d", m, FVM_MAXV); return -1; }
    if (n_patches <= 0) return 0;
    const long nblk = (n_patches + pl.ppb - 1) / pl.ppb;
    if (nblk > 0x7fffffffL) { set_error("MUSCL-Hancock: %ld patches are more than one launch covers", n_patches); return -1; }
    const double r = dt / h;
    auto go = [&](auto kern, int nt) -> int {
        if (pl.lds > 64 * 1024) {
            hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
            if (ea != hipSuccess) { set_error("hipFuncSetAttribute(fv muscl, %zu B LDS): %s", pl.lds, hipGetErrorString(ea)); return -2; }
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(nt), pl.lds, s, Q, out, slot, P, H, m, V, r, n_patches, pl.ppb);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_error("fv_muscl launch: %s", hipGetErrorString(e)); return -2; }
        return 0;
    };
    if constexpr (DIM == 2) {                                     // (fv_muscl_plan asks for 512 threads in 2-D only)
        if (pl.nt == 512) return go(fv_muscl_kernel<DIM, PDE, 512>, 512);
    }
    return go(fv_muscl_kernel<DIM, PDE, 256>, 256);
}

}  // namespace exa

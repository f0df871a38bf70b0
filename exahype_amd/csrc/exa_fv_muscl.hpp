// Second-order MUSCL-Hancock patch update for gfx950 (EXA_FV_MUSCL_HANCOCK) -- the templates; fv_muscl.hip instantiates them
// for the built-in term sets, fv_muscl_user.hip for a generated one (pde_codegen.SympyPDE(muscl_hancock=True[, muscl_terms=True])).
//
// The scheme, on a patch array Q[patch][S..][V] (S = P + 2 H, H >= 2), evolved variables v < m, r = dt / h:
//   1. slopes       s_e(c) = minmod(Q_c - Q_{c-e}, Q_{c+e} - Q_c) for every axis e, for the interior volumes and their face neighbours (the "plus
//                   shape").  minmod decides by the signs of its arguments (a NaN difference: slope 0); auxiliary variables have slope 0.
//   2. predictor    delta_c = -(r/2) sum_e [f_e(Q_c + s_e/2) - f_e(Q_c - s_e/2)]                                 (unsplit, all axes)
//   3. face states  w_c^{+-d} = (Q_c +- s_d(c)/2) + delta_c
//   4. face flux    F* = (f_d(w_L) + f_d(w_R))/2 - max(l_d(w_L), l_d(w_R))/2 (w_R - w_L)     (flux_rt / maxeig: IEEE division and square root)
//   5. update       Q_c <- Q_c - r sum_d (F*_{c+1/2,d} - F*_{c-1/2,d}), interior volumes, evolved variables; everything else stays as it is.
// A term set with a source S(q) and / or a non-conservative product B_d(q) dq of the state alone (HAS_MUSCL_TERMS; pde_codegen.SympyPDE(muscl_hancock=
// True, muscl_terms=True)) adds, under `if constexpr` -- the instantiations without them are what they were, operation for operation:
//   2. predictor    ... - (r/2) sum_e B_e(Q_c) s_e(c) + (dt/2) S(Q_c)
//   4. face jump    D_{c+1/2,d} = B_d((w_L + w_R)/2) (w_R - w_L) on the predicted face states (fv_muscl_jump: the form of the Rusanov kernel)
//   5. update       ... - r sum_d [1/2 (D_{c+1/2,d} + D_{c-1/2,d}) + B_d(Q_c + delta_c) s_d(c)] + dt S(Q_c + delta_c)      (midpoint rule in time)
// Every quantity is at hand in the phase that needs it: the LDS plan and the staging are the same.  The terms see 0 for auxiliary variables.
// An interior update reads Q at c +- e_d, c +- 2 e_d and c +- e_d +- e_e (d != e): the two halo layers next to the interior INCLUDING the edge entries
// (layer 1 along two axes); never (+-2, +-1), the 3-D corners or a layer beyond the second.
//
// One workgroup owns `ppb` patches.  LDS plan: the window T = P + 4 of every patch (its interior and the two halo layers next to it, all V
// variables; H = 2: the whole patch, one contiguous block of HBM) and the predictor's delta over (P + 2)^DIM x m.  Phase 1: one task per
// plus-shape volume -> delta.  Barrier.  Phase 2: one task per interior volume rebuilds its 2 DIM + 1 slopes per axis from the window (the very
// function phase 1 ran: the same bits), takes the neighbours' delta from LDS, evaluates its 2 DIM face fluxes and stores the new state.  Both
// sides of a face evaluate fv_muscl_face on the same two states, so the flux a volume loses is bit for bit the one its neighbour gains.  The
// window is complete before the first store, so in place is safe; the unit is compiled without FMA contraction like the Rusanov unit.
//
// fv_muscl_grid_kernel (further down) is the GRID form on halo-less arrays: the same plan and the same two phases (fv_muscl_predict,
// fv_muscl_correct -- the device functions both kernels call, so the results are bit-identical), another staging -- the window is gathered from the
// patch, its face neighbours and its diagonal neighbours -- and the next step's CFL scan reduced from the values phase 2 stores.
//
// fv_muscl_stream_kernel is the PLANE-STREAMING form for 3-D patches whose window does not fit (P >= 10 at five variables; up to P = 19): a ring of
// five or six window planes and three predictor planes instead of the whole window, one walk along axis 0.  The loop bodies of both phases are the
// per-volume functions fv_muscl_predict_volume / fv_muscl_correct_volume, which all three kernels call: a volume's neighbours are described by their
// distances (FvMusclNbr), uniform strides in the resident and the grid kernel, ring-slot distances along axis 0 in the streamed one.
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

// slopes of the evolved variables of the volume at q along the axis whose minus neighbour stands sm doubles below it, the plus neighbour sp above
__device__ __forceinline__ void fv_muscl_slope(const double* q, int sm, int sp, int m, double (&s)[FVM_MAXV]) {
#pragma unroll
    for (int v = 0; v < FVM_MAXV; v++) s[v] = v < m ? fv_minmod(q[v] - q[v - sm], q[v + sp] - q[v]) : 0.0;
}

// where a volume finds its neighbours along every axis e, as distances in doubles: the window entry at -1 stands qm[e] below the volume's own, the
// one at -2 qmm[e] below THAT; qp[e] / qpp[e] likewise upwards; the predictor's increments at -1 / +1 stand dm[e] below / dp[e] above.  The resident
// and the grid kernel fill all of them with the axis' stride; in the streamed kernel the axis-0 neighbours stand in other ring slots, at distances
// of their own (of either sign)
struct FvMusclNbr {
    int qmm[3], qm[3], qp[3], qpp[3];
    int dm[3], dp[3];
};

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

// path-conservative jump term of the face (wL, wR) along D: B_D at the mean state times the jump (half of it goes to either side)
template <class PDE, int D>
__device__ __forceinline__ void fv_muscl_jump(const double (&wL)[FVM_MAXV], const double (&wR)[FVM_MAXV], int m, double (&out)[FVM_MAXV]) {
    double qa[FVM_MAXV], dq[FVM_MAXV];
#pragma unroll
    for (int v = 0; v < FVM_MAXV; v++) { qa[v] = 0.5 * (wL[v] + wR[v]); dq[v] = wR[v] - wL[v]; out[v] = 0.0; }
    PDE::ncp(qa, dq, D, out);
#pragma unroll
    for (int v = 0; v < FVM_MAXV; v++) out[v] = v < m ? out[v] : 0.0;
}

template <int DIM> __host__ __device__ constexpr int fvm_pow(int b) { return DIM == 3 ? b * b * b : b * b; }

// volume strides of the window and of delta's box
template <int DIM> __device__ __forceinline__ void fv_muscl_strides(int T, int D, int (&tst)[3], int (&dst)[3]) {
    if constexpr (DIM == 3) { tst[0] = T * T; tst[1] = T; tst[2] = 1; dst[0] = D * D; dst[1] = D; dst[2] = 1; }
    else { tst[0] = T; tst[1] = 1; tst[2] = 0; dst[0] = D; dst[1] = 1; dst[2] = 0; }
}

// the predictor of ONE plus-shape volume at q (neighbours nb.qm, nb.qp) -> dl[0 .. m); hr = r / 2
template <int DIM, class PDE>
__device__ __forceinline__ void fv_muscl_predict_volume(const double* q, const FvMusclNbr& nb, double* dl, int m, double hr, [[maybe_unused]] double dt) {
    double qc[FVM_MAXV], sum[FVM_MAXV];
#pragma unroll
    for (int v = 0; v < FVM_MAXV; v++) { qc[v] = v < m ? q[v] : 0.0; sum[v] = 0.0; }
    static_for_muscl<0, DIM>([&](auto ee) {
        constexpr int e = decltype(ee)::value;
        double s[FVM_MAXV], wp[FVM_MAXV], wm[FVM_MAXV], fp[FVM_MAXV], fm[FVM_MAXV];
        fv_muscl_slope(q, nb.qm[e], nb.qp[e], m, s);
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) { wp[v] = qc[v] + 0.5 * s[v]; wm[v] = qc[v] - 0.5 * s[v]; fp[v] = 0.0; fm[v] = 0.0; }
        PDE::flux_rt(wp, e, fp);
        PDE::flux_rt(wm, e, fm);
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) sum[v] = e == 0 ? fp[v] - fm[v] : sum[v] + (fp[v] - fm[v]);
        if constexpr (pde_has_ncp<PDE>::value) {                  // + B_e(Q_c) s_e(c)
            double nc[FVM_MAXV];
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++) nc[v] = 0.0;
            PDE::ncp(qc, s, e, nc);
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++) sum[v] += nc[v];
        }
    });
    if constexpr (pde_has_source<PDE>::value) {                   // + (dt/2) S(Q_c)
        double Sq[FVM_MAXV];
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) Sq[v] = 0.0;
        PDE::source(qc, Sq);
        const double hdt = 0.5 * dt;
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++)
            if (v < m) dl[v] = -hr * sum[v] + hdt * Sq[v];
    } else {
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++)
            if (v < m) dl[v] = -hr * sum[v];
    }
}

// the corrector of ONE interior volume at q with its predictor increments at dl.  Both sides of a face evaluate fv_muscl_face on the same two states.
// store(updated) is called once at the end and writes the volume where its kernel keeps it: updated(v) is the new value of evolved variable v < m
template <int DIM, class PDE, class Store>
__device__ __forceinline__ void fv_muscl_correct_volume(const double* q, const double* dl, const FvMusclNbr& nb, int m, double r, [[maybe_unused]] double dt,
                                                        Store&& store) {
    double qc[FVM_MAXV], dC[FVM_MAXV], acc[FVM_MAXV];
#pragma unroll
    for (int v = 0; v < FVM_MAXV; v++) { qc[v] = v < m ? q[v] : 0.0; dC[v] = v < m ? dl[v] : 0.0; acc[v] = 0.0; }
    [[maybe_unused]] double qh[FVM_MAXV];                         // the half-step state Q_c + delta_c, where the volume's own terms are taken
    if constexpr (pde_has_ncp<PDE>::value || pde_has_source<PDE>::value) {
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) qh[v] = qc[v] + dC[v];
    }
    static_for_muscl<0, DIM>([&](auto dd) {
        constexpr int d = decltype(dd)::value;
        const int qmm = nb.qmm[d], qm = nb.qm[d], qp = nb.qp[d], qpp = nb.qpp[d], dm = nb.dm[d], dp = nb.dp[d];
        double sC[FVM_MAXV], sN[FVM_MAXV], wCp[FVM_MAXV], wCm[FVM_MAXV], wN[FVM_MAXV], Fp[FVM_MAXV], Fm[FVM_MAXV];
        fv_muscl_slope(q, qm, qp, m, sC);
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) { wCp[v] = (qc[v] + 0.5 * sC[v]) + dC[v]; wCm[v] = (qc[v] - 0.5 * sC[v]) + dC[v]; }
        fv_muscl_slope(q + qp, qp, qpp, m, sN);                             // the plus-side neighbour's minus state
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) wN[v] = v < m ? (q[qp + v] - 0.5 * sN[v]) + dl[dp + v] : 0.0;
        fv_muscl_face<PDE, d>(wCp, wN, m, Fp);
        [[maybe_unused]] double Dp[FVM_MAXV], Dm[FVM_MAXV];
        if constexpr (pde_has_ncp<PDE>::value) fv_muscl_jump<PDE, d>(wCp, wN, m, Dp);
        fv_muscl_slope(q - qm, qmm, qm, m, sN);                             // the minus-side neighbour's plus state
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) wN[v] = v < m ? (q[v - qm] + 0.5 * sN[v]) + dl[v - dm] : 0.0;
        fv_muscl_face<PDE, d>(wN, wCm, m, Fm);
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) acc[v] = d == 0 ? Fp[v] - Fm[v] : acc[v] + (Fp[v] - Fm[v]);
        if constexpr (pde_has_ncp<PDE>::value) {                  // + (D_{c+1/2} + D_{c-1/2}) / 2 + B_d(Q_c + delta_c) s_d(c)
            double Bs[FVM_MAXV];
            fv_muscl_jump<PDE, d>(wN, wCm, m, Dm);
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++) Bs[v] = 0.0;
            PDE::ncp(qh, sC, d, Bs);
#pragma unroll
            for (int v = 0; v < FVM_MAXV; v++)
                if (v < m) acc[v] += (0.5 * Dp[v] + 0.5 * Dm[v]) + Bs[v];
        }
    });
    [[maybe_unused]] double Sq[FVM_MAXV];                         // S(Q_c + delta_c): the source at the half-step state
    if constexpr (pde_has_source<PDE>::value) {
#pragma unroll
        for (int v = 0; v < FVM_MAXV; v++) Sq[v] = 0.0;
        PDE::source(qh, Sq);
    }
    store([&](int v) -> double {
        if constexpr (pde_has_source<PDE>::value) return (qc[v] - r * acc[v]) + dt * Sq[v];
        else return qc[v] - r * acc[v];
    });
}

// phase 1 of a workgroup whose `np` windows stand in img: delta of every plus-shape volume (box coordinates 0 .. P + 1, at most one of them
// outside 1 .. P) -> del
template <int DIM, class PDE, int NT>
__device__ __forceinline__ void fv_muscl_predict(const double* img, double* del, const long* __restrict__ slot, long first, int np, int P, int m, int V,
                                                 double r, [[maybe_unused]] double dt) {
    const int T = P + 4, D = P + 2;
    const int tvol = fvm_pow<DIM>(T), dvol = fvm_pow<DIM>(D);
    const int tid = (int)threadIdx.x;
    int tst[3], dst[3];
    fv_muscl_strides<DIM>(T, D, tst, dst);
    const double hr = 0.5 * r;
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
        FvMusclNbr nb;
#pragma unroll
        for (int e = 0; e < DIM; e++) nb.qm[e] = nb.qp[e] = tst[e] * V;
        fv_muscl_predict_volume<DIM, PDE>(q, nb, del + ((long)pp * dvol + dc) * m, m, hr, dt);
    }
}

// phase 2: the interior volumes of the `np` patches.  out == nullptr: in place into Q (layout with halo H); else halo-less out [patch][P^DIM][V],
// auxiliary variables copied.  LAM: -> the largest eigenvalue over the directions of the NEW states this lane stored (nan_max: a NaN survives),
// evaluated on the values as the arrays hold them -- what a scan of `out` would read
template <int DIM, class PDE, int NT, bool LAM>
__device__ __forceinline__ double fv_muscl_correct(const double* img, const double* del, double* __restrict__ Q, double* __restrict__ out,
                                                   const long* __restrict__ slot, long first, int np, int P, int H, int m, int V, double r,
                                                   [[maybe_unused]] double dt) {
    const int S = P + 2 * H, T = P + 4, D = P + 2;
    const int tvol = fvm_pow<DIM>(T), dvol = fvm_pow<DIM>(D), ncell = fvm_pow<DIM>(P);
    const long svol = DIM == 3 ? (long)S * S * S : (long)S * S;
    const int tid = (int)threadIdx.x;
    int tst[3], dst[3];
    fv_muscl_strides<DIM>(T, D, tst, dst);
    [[maybe_unused]] double lmax = 0.0;
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
        FvMusclNbr nb;
#pragma unroll
        for (int d = 0; d < DIM; d++) {
            const int qs = tst[d] * V, ds = dst[d] * m;
            nb.qmm[d] = nb.qm[d] = nb.qp[d] = nb.qpp[d] = qs;
            nb.dm[d] = nb.dp[d] = ds;
        }
        fv_muscl_correct_volume<DIM, PDE>(q, dl, nb, m, r, dt, [&](auto updated) {
            if (out) {                                            // halo-less QOut [patch][P^DIM][V]: auxiliary variables copied
                double* o = out + (patch * ncell + id) * V;
#pragma unroll
                for (int v = 0; v < FVM_MAXV; v++)
                    if (v < m) o[v] = updated(v);
                for (int v = m; v < V; v++) o[v] = q[v];
                if constexpr (LAM) {
                    double qn[FVM_MAXV];
#pragma unroll
                    for (int v = 0; v < FVM_MAXV; v++) qn[v] = v < m ? updated(v) : (v < V ? q[v] : 0.0);
#pragma unroll
                    for (int d = 0; d < DIM; d++) lmax = nan_max(lmax, PDE::maxeig(qn, d));
                }
            } else {
                const long c = DIM == 3 ? ((long)(co[0] + H) * S + (co[1] + H)) * S + (co[2] + H) : (long)(co[0] + H) * S + (co[1] + H);
                double* o = Q + (patch * svol + c) * V;
#pragma unroll
                for (int v = 0; v < FVM_MAXV; v++)
                    if (v < m) o[v] = updated(v);
            }
        });
    }
    return lmax;
}

template <int DIM, class PDE, int NT>
__global__ void __launch_bounds__(NT)
fv_muscl_kernel(double* __restrict__ Q, double* __restrict__ out, const long* __restrict__ slot, int P, int H, int m, int V, double r,
                long n_patches, int ppb, double dt) {
    extern __shared__ __attribute__((aligned(16))) double fvm_lds[];
    const int S = P + 2 * H, T = P + 4, off = H - 2;
    const int tvol = fvm_pow<DIM>(T);
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

    fv_muscl_predict<DIM, PDE, NT>(img, del, slot, first, np, P, m, V, r, dt);
    __syncthreads();
    fv_muscl_correct<DIM, PDE, NT, false>(img, del, Q, out, slot, first, np, P, H, m, V, r, dt);
}

// ---- the PLANE-STREAMING form (3-D; a plan of exa_fv_plan_create_streamed): for patches whose whole window does not fit a compute unit's LDS.  One
// workgroup per patch walks the planes of axis 0 once and keeps a ring of `ring` window planes [T][T][V] and three predictor planes [D][D][m]:
//   step s = 0 .. T - 1:   stage window plane s                     (H = 2: one contiguous block of the patch, 16-byte loads; else row by row)
//                          barrier
//                          predictor plane s - 2                    (box plane d reads window planes d .. d + 2; the plus-shape rule as ever)
//                          barrier
//                          interior plane s - 4: compute and store  (interior plane i reads window planes i .. i + 4, predictor planes i .. i + 2)
//                          ring == 5: barrier                       (the next stage overwrites window plane s - 4, which this step still read)
// With a sixth slot the next stage overwrites plane s - 5, which nobody reads any more: two barriers per plane, and the loads of plane s + 1 are on
// their way while the slower lanes still finish plane s - 4.  The per-volume arithmetic is fv_muscl_predict_volume / fv_muscl_correct_volume -- the
// functions of the resident kernel on the same operands, so the results are bit-identical wherever both serve a shape; only the axis-0 neighbours
// stand at the distances of their ring slots.
// IN PLACE IS SAFE BECAUSE every plane of the patch is read from HBM before its interior is written: window plane w is staged in step w, the interior
// of that plane (interior plane w - 2) is stored in step w + 2, and from its staging on the plane is read from the ring only.  Nothing may read Q
// behind the walk.
template <class PDE, int NT>
__global__ void __launch_bounds__(NT)
fv_muscl_stream_kernel(double* __restrict__ Q, double* __restrict__ out, const long* __restrict__ slot, int P, int H, int m, int V, double r, int ring,
                       double dt) {
    extern __shared__ __attribute__((aligned(16))) double fvm_lds[];
    const long patch = (long)blockIdx.x;
    if (slot && slot[patch] < 0) return;                          // the whole workgroup, before any load and any barrier
    const int S = P + 2 * H, T = P + 4, D = P + 2, off = H - 2;
    const int wpl = T * T * V, ppl = D * D * m;                   // doubles of a window plane / a predictor plane
    const long svol = (long)S * S * S;
    double* win = fvm_lds;                                        // [ring][T][T][V]
    double* pre = fvm_lds + (long)ring * wpl;                     // [3][D][D][m]
    const double* src = Q + patch * svol * V;
    const int tid = (int)threadIdx.x;
    const double hr = 0.5 * r;
    for (int s = 0; s < T; s++) {
        // ---- stage window plane s
        double* dst = win + (s % ring) * wpl;
        if (off == 0) {                                           // the plane is one contiguous block of the patch
            const double* sp = src + (long)s * wpl;
            const unsigned long long sa = reinterpret_cast<unsigned long long>(sp), da = reinterpret_cast<unsigned long long>(dst);
            if (((sa ^ da) & 15) == 0) {                          // both reach a 16-byte boundary after the same `head` doubles
                const int head = (int)((sa >> 3) & 1), nv = (wpl - head) / 2;
                const fvm_v2d* s2 = reinterpret_cast<const fvm_v2d*>(sp + head);
                fvm_v2d* d2 = reinterpret_cast<fvm_v2d*>(dst + head);
                for (int i = tid; i < nv; i += NT) d2[i] = s2[i];
                if (tid == 0) {
                    if (head) dst[0] = sp[0];
                    if ((wpl - head) & 1) dst[wpl - 1] = sp[wpl - 1];
                }
            } else {
                for (int i = tid; i < wpl; i += NT) dst[i] = sp[i];
            }
        } else {                                                  // H > 2: rows of T V contiguous doubles
            const int row = T * V;
            for (int i = tid; i < wpl; i += NT) {
                const int rw = i / row, x = i - rw * row;
                dst[i] = src[(((long)(s + off) * S + (rw + off)) * S + off) * V + x];
            }
        }
        __syncthreads();

        // ---- predictor plane d0 = s - 2 (box coordinates): window plane d0 + 1, neighbours in planes d0 and d0 + 2
        if (s >= 2) {
            const int d0 = s - 2, o0 = (d0 < 1 || d0 > P) ? 1 : 0;
            const int w0 = d0 % ring, w1 = (d0 + 1) % ring, w2 = (d0 + 2) % ring;
            const double* wc = win + w1 * wpl;
            double* pc = pre + (d0 % 3) * ppl;
            FvMusclNbr nb;
            nb.qm[0] = (w1 - w0) * wpl; nb.qp[0] = (w2 - w1) * wpl;
            nb.qm[1] = nb.qp[1] = T * V;
            nb.qm[2] = nb.qp[2] = V;
            for (int i = tid; i < D * D; i += NT) {
                const int y = i / D, x = i - y * D;
                if (o0 + ((y < 1 || y > P) ? 1 : 0) + ((x < 1 || x > P) ? 1 : 0) > 1) continue;
                fv_muscl_predict_volume<3, PDE>(wc + ((y + 1) * T + (x + 1)) * V, nb, pc + (y * D + x) * m, m, hr, dt);
            }
        }
        __syncthreads();

        // ---- interior plane i0 = s - 4: window plane i0 + 2 with planes i0 .. i0 + 4 around it, predictor plane i0 + 1 between i0 and i0 + 2
        if (s >= 4) {
            const int i0 = s - 4;
            int w[5], p[3];
#pragma unroll
            for (int k = 0; k < 5; k++) w[k] = (i0 + k) % ring;
#pragma unroll
            for (int k = 0; k < 3; k++) p[k] = (i0 + k) % 3;
            const double* wc = win + w[2] * wpl;
            const double* pc = pre + p[1] * ppl;
            FvMusclNbr nb;
            nb.qmm[0] = (w[1] - w[0]) * wpl; nb.qm[0] = (w[2] - w[1]) * wpl; nb.qp[0] = (w[3] - w[2]) * wpl; nb.qpp[0] = (w[4] - w[3]) * wpl;
            nb.dm[0] = (p[1] - p[0]) * ppl; nb.dp[0] = (p[2] - p[1]) * ppl;
            nb.qmm[1] = nb.qm[1] = nb.qp[1] = nb.qpp[1] = T * V;
            nb.qmm[2] = nb.qm[2] = nb.qp[2] = nb.qpp[2] = V;
            nb.dm[1] = nb.dp[1] = D * m;
            nb.dm[2] = nb.dp[2] = m;
            for (int i = tid; i < P * P; i += NT) {
                const int y = i / P, x = i - y * P;
                const double* q = wc + ((y + 2) * T + (x + 2)) * V;
                fv_muscl_correct_volume<3, PDE>(q, pc + ((y + 1) * D + (x + 1)) * m, nb, m, r, dt, [&](auto updated) {
                    if (out) {                                    // halo-less QOut [patch][P^3][V]: auxiliary variables copied
                        double* o = out + ((patch * P + i0) * (long)(P * P) + i) * V;
#pragma unroll
                        for (int v = 0; v < FVM_MAXV; v++)
                            if (v < m) o[v] = updated(v);
                        for (int v = m; v < V; v++) o[v] = q[v];
                    } else {                                      // in place: this plane of Q was staged two steps ago (see above)
                        double* o = Q + (patch * svol + ((long)(i0 + H) * S + (y + H)) * S + (x + H)) * V;
#pragma unroll
                        for (int v = 0; v < FVM_MAXV; v++)
                            if (v < m) o[v] = updated(v);
                    }
                });
            }
        }
        if (ring == 5) __syncthreads();                           // (the next stage reuses the slot of window plane s - 4)
    }
}

// ---- the GRID step (exa_fv_grid_step_muscl_device): the patches are the cells of a Cartesian grid g[0] x g[1] (x g[2]), patch index row-major,
// Q and out are HALO-LESS [patch][P^DIM][V] (P >= 2), Q is only read.  Only the staging differs from fv_muscl_kernel: the window of a patch is
// gathered from the patch, its face neighbours AND its diagonal neighbours (the edge entries), every outside axis resolved on its own --
//   inside the domain or a periodic face   the neighbour patch along that axis (wrap), in-patch coordinate c -+ P
//   FV_FACE_MIRROR at the patch's domain face   the patch's own coordinate -1 - c (low) / 2 P - 1 - c (high), every variable times the face's sign
//   FV_FACE_STATE                               the face's state
// -- and two outside axes composed in axis order, the later axis last (what a halo fill axis after axis over the full transverse range leaves,
// solvers.fill_halos_boundary; the rule of exa_lim_project_patches_halo2): walking from the last axis down, the first state met is the value, times
// the signs of the mirrors met before it; without a state the source volume times all mirror signs.  The entries no update reads (a second layer
// together with another outside coordinate, the 3-D corners) are not written: phase 1 keeps to the plus shape, phase 2 to what the header lists.
// Neighbours live in other workgroups, which is why the new states go to a second array.

// grid coordinates of a patch (32-bit arithmetic; the launcher has checked n_patches < 2^32)
template <int DIM> __device__ __forceinline__ void fv_muscl_patch_coords(const FvGrid& ga, long patch, int (&pg)[3]) {
    unsigned x = (unsigned)patch;
    if constexpr (DIM == 3) { pg[2] = (int)(x % (unsigned)ga.g[2]); x /= (unsigned)ga.g[2]; } else pg[2] = 0;
    pg[1] = (int)(x % (unsigned)ga.g[1]);
    pg[0] = (int)(x / (unsigned)ga.g[1]);
}

// where the window entry at interior coordinates c (each in -2 .. P + 1) of the patch at pg finds its V doubles; mirrors: bit (axis * 2 + side) set
// for every mirror face whose signs multiply them.  fbits: two bits per face, 0 where every face is periodic
template <int DIM>
__device__ __forceinline__ const double* fv_muscl_grid_source(const double* __restrict__ Q, const FvGrid& ga, unsigned fbits, const int (&pg)[3],
                                                              const int (&c)[3], int P, int V, unsigned& mirrors) {
    int pn[3] = {pg[0], pg[1], pg[2]}, cn[3] = {c[0], c[1], c[2]};
    mirrors = 0u;
    const double* state = nullptr;
    static_for_muscl<0, DIM>([&](auto kk) {
        constexpr int a = DIM - 1 - decltype(kk)::value;          // the later axis first: it was filled last
        if (state || (c[a] >= 0 && c[a] < P)) return;
        const int side = c[a] < 0 ? 0 : 1, face = a * 2 + side;
        const bool at_face = side == 0 ? pg[a] == 0 : pg[a] == ga.g[a] - 1;
        const int kind = at_face ? (int)((fbits >> (2 * face)) & 3u) : FV_FACE_PERIODIC;
        if (kind == FV_FACE_STATE) { state = ga.bstate + face * V; return; }
        if (kind == FV_FACE_MIRROR) {
            cn[a] = (side == 0 ? -1 : 2 * P - 1) - c[a];
            mirrors |= 1u << face;
            return;
        }
        pn[a] += side == 0 ? -1 : 1;
        if (pn[a] < 0) pn[a] += ga.g[a];
        if (pn[a] >= ga.g[a]) pn[a] -= ga.g[a];
        cn[a] = side == 0 ? c[a] + P : c[a] - P;
    });
    if (state) return state;
    const long np = DIM == 3 ? ((long)pn[0] * ga.g[1] + pn[1]) * ga.g[2] + pn[2] : (long)pn[0] * ga.g[1] + pn[1];
    const int cl = DIM == 3 ? (cn[0] * P + cn[1]) * P + cn[2] : cn[0] * P + cn[1];
    return Q + (np * fvm_pow<DIM>(P) + cl) * V;
}

// wave-level maximum -> one integer atomic max per wave, issued only where it exceeds what is there (non-negative doubles order like their bit
// patterns, a NaN lies above them all; the launcher zeroed lam)
__device__ __forceinline__ void fv_muscl_lam_commit(double* lam, double mx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = nan_max(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* at = reinterpret_cast<unsigned long long*>(lam);
        const unsigned long long bits = (unsigned long long)__double_as_longlong(mx);
        if (bits > __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(at, bits);
    }
}

template <int DIM, class PDE, int NT>
__global__ void __launch_bounds__(NT)
fv_muscl_grid_kernel(const double* __restrict__ Q, double* __restrict__ out, int P, int m, int V, double r, long n_patches, int ppb, FvGrid ga,
                     double dt) {
    extern __shared__ __attribute__((aligned(16))) double fvm_lds[];
    const int T = P + 4;
    const int tvol = fvm_pow<DIM>(T);
    double* img = fvm_lds;                                        // [patch slot][T^DIM][V]
    double* del = fvm_lds + (long)ppb * tvol * V;                 // [patch slot][(P + 2)^DIM][m]
    const long first = (long)blockIdx.x * ppb;
    const int np = (int)(n_patches - first < ppb ? n_patches - first : ppb);
    const int tid = (int)threadIdx.x;
    unsigned fbits = 0u;                                          // kinds of the domain faces (launch-uniform)
    if (ga.bstate) {
#pragma unroll
        for (int f = 0; f < 2 * DIM; f++) fbits |= (unsigned)ga.bkind[f] << (2 * f);
    }

    // ---- stage the windows: one task per window volume, V doubles each
    for (int i = tid; i < np * tvol; i += NT) {
        const int pp = i / tvol, tv = i - pp * tvol;
        int c[3];                                                 // interior coordinates -2 .. P + 1
        if constexpr (DIM == 3) { c[0] = tv / (T * T) - 2; c[1] = (tv / T) % T - 2; c[2] = tv % T - 2; }
        else { c[0] = tv / T - 2; c[1] = tv % T - 2; c[2] = 0; }
        int outside = 0, second = 0;
#pragma unroll
        for (int a = 0; a < DIM; a++) { outside += (c[a] < 0 || c[a] >= P) ? 1 : 0; second += (c[a] < -1 || c[a] > P) ? 1 : 0; }
        if (outside > 2 || (outside == 2 && second > 0)) continue;            // no update reads it
        int pg[3];
        fv_muscl_patch_coords<DIM>(ga, first + pp, pg);
        unsigned mirrors;
        const double* src = fv_muscl_grid_source<DIM>(Q, ga, fbits, pg, c, P, V, mirrors);
        double* dst = img + (long)i * V;
        if (mirrors == 0u) {
            for (int v = 0; v < V; v++) dst[v] = src[v];
        } else {
            for (int v = 0; v < V; v++) {
                double x = src[v];
#pragma unroll
                for (int f = 0; f < 2 * DIM; f++)
                    if ((mirrors >> f) & 1u) x *= ga.bstate[f * V + v];
                dst[v] = x;
            }
        }
    }
    __syncthreads();

    fv_muscl_predict<DIM, PDE, NT>(img, del, nullptr, first, np, P, m, V, r, dt);
    __syncthreads();
    const double lmax = fv_muscl_correct<DIM, PDE, NT, true>(img, del, nullptr, out, nullptr, first, np, P, 2, m, V, r, dt);
    if (ga.lam) fv_muscl_lam_commit(ga.lam, lmax);
}

// ---- host side: the one entry of this update (PdeKernels::fv_muscl) for a term set.  It selects the form (a.form: FV_FORM_*) and the dimension; the
// plan (patches per workgroup, threads, LDS bytes, ring) is fv_muscl_plan's / fv_muscl_stream_plan's, which exa_fv_plan_create[_streamed] has
// checked.  The term sets of this mode see the state alone: a.centre and a.t are not read.
template <class PDE>
int fv_muscl_entry(const FvLaunch& a) {
    const int P = a.P, m = a.n_real, V = a.n_real + a.n_aux;
    const bool streamed = a.form == FV_FORM_STREAMED, grid = a.form == FV_FORM_GRID;
    FvMusclPlan pl;
    if (streamed) {
        if (P < 1 || P > 1024 || !fv_muscl_stream_plan(P, m, V, &pl)) {
            set_error("MUSCL-Hancock (streamed): five window planes and three predictor planes need %zu B of LDS, %zu B are available",
                      P >= 1 && P <= 1024 ? pl.lds : (size_t)-1, FV_MUSCL_LDS_AVAILABLE);
            return -1;
        }
    } else if (!fv_muscl_plan(a.dim, P, m, V, &pl)) {
        set_error("MUSCL-Hancock: the patch needs %zu B of LDS, %zu B are available", pl.lds, FV_MUSCL_LDS_AVAILABLE);
        return -1;
    }
    if (grid && P < 2) { set_error("MUSCL-Hancock grid step: patch_size must be >= 2"); return -1; }
    if (!grid && a.H < 2) { set_error("MUSCL-Hancock reads two halo layers"); return -1; }
    if (m > FVM_MAXV) { set_error("n_real = %d exceeds %d", m, FVM_MAXV); return -1; }
    if (grid) {
        if (!a.grid) { set_error("MUSCL-Hancock grid step: no grid"); return -1; }
        if (!a.Q || !a.out || a.Q == a.out) { set_error("MUSCL-Hancock grid step: the new states need an array of their own"); return -1; }
        if (a.n_patches > 0xffffffffL) { set_error("MUSCL-Hancock grid step: %ld patches -- a grid holds at most 2^32 - 1", a.n_patches); return -1; }
        if (a.grid->lam) {
            hipError_t e0 = hipMemsetAsync(a.grid->lam, 0, sizeof(double), a.stream);
            if (e0 != hipSuccess) { set_error("memset: %s", hipGetErrorString(e0)); return -2; }
        }
    }
    if (a.n_patches <= 0) return 0;
    const long nblk = (a.n_patches + pl.ppb - 1) / pl.ppb;
    if (nblk > 0x7fffffffL) { set_error("MUSCL-Hancock: %ld patches are more than one launch covers", a.n_patches); return -1; }
    const double r = a.dt / a.h;
    // form: "", " stream", " grid" (error messages); args: the kernel's
    auto launch = [&](const char* form, auto kern, int nt, auto... args) -> int {
        if (pl.lds > 64 * 1024) {
            hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds);
            if (ea != hipSuccess) { set_error("hipFuncSetAttribute(fv muscl%s, %zu B LDS): %s", form, pl.lds, hipGetErrorString(ea)); return -2; }
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(nt), pl.lds, a.stream, args...);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_error("fv_muscl%s launch: %s", form, hipGetErrorString(e)); return -2; }
        return 0;
    };
    auto in_dim = [&](auto dim_c) -> int {
        constexpr int DIM = decltype(dim_c)::value;
        if (streamed) {
            if constexpr (DIM == 3) return launch(" stream", fv_muscl_stream_kernel<PDE, 256>, pl.nt, a.Q, a.out, a.slot, P, a.H, m, V, r, pl.ring, a.dt);
            set_error("MUSCL-Hancock (streamed): the plane-streaming kernel is 3-D only");
            return -1;
        }
        const double* Qin = a.Q;                                  // (the grid kernel only reads Q)
        if constexpr (DIM == 2) {                                 // (fv_muscl_plan asks for 512 threads in 2-D only)
            if (pl.nt == 512)
                return grid ? launch(" grid", fv_muscl_grid_kernel<DIM, PDE, 512>, 512, Qin, a.out, P, m, V, r, a.n_patches, pl.ppb, *a.grid, a.dt)
                            : launch("", fv_muscl_kernel<DIM, PDE, 512>, 512, a.Q, a.out, a.slot, P, a.H, m, V, r, a.n_patches, pl.ppb, a.dt);
        }
        return grid ? launch(" grid", fv_muscl_grid_kernel<DIM, PDE, 256>, 256, Qin, a.out, P, m, V, r, a.n_patches, pl.ppb, *a.grid, a.dt)
                    : launch("", fv_muscl_kernel<DIM, PDE, 256>, 256, a.Q, a.out, a.slot, P, a.H, m, V, r, a.n_patches, pl.ppb, a.dt);
    };
    if (a.dim == 2) return in_dim(std::integral_constant<int, 2>{});
    if constexpr (PDE::MAXDIM >= 3) {
        if (a.dim == 3) return in_dim(std::integral_constant<int, 3>{});
    }
    set_error("MUSCL-Hancock: the term set has no kernel for dim %d", a.dim);
    return -1;
}

}  // namespace exa

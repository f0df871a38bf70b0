// A-posteriori (MOOD) detection for the subcell limiter: two HBM-bound passes over u[cell][node][var], a cell's contiguous block per
// workgroup (N^dim > 64 nodes) or per wave (four cells per workgroup).
//   limiter_snapshot_kernel   u^n -> u_old (skipped if null) and bounds[cell][2 K_DMP] = min, max of every watched variable
//   limiter_detect_kernel     candidate -> mask byte: a value not finite / a node not admissible, or the nodal range of a watched variable
//                             leaves [lo - delta, hi + delta] of the bounds of the cell and its face neighbours
// What "admissible" means and which variables the relaxed discrete maximum principle (DMP) watches is a CRITERION type:
//   static constexpr int NV       variables per node, 0: run-time (the kernel's nv_rt argument)
//   static constexpr int K_DMP    watched variables (0: positivity and finiteness only -- no bounds, no neighbourhood loop)
//   dmp_var(k, nv)                the k-th watched variable
//   troubled(s, nv, floor)        the node with state s[nv] is not admissible (written so that NaN counts as troubled)
// LimEulerCrit is the built-in one (limiter.hip instantiates it); LimPdeCrit<PDE> takes all of it from a generated term set that carries
// HAS_ADMISSIBLE (pde_codegen.py; instantiated in the term set's side library by lim_user.hip), with everything a compile-time constant.
// Minima travel negated so that one max-reduction serves every value; min / max are exact, so the result does not depend on the
// reduction order.
#pragma once
#include <hip/hip_runtime.h>
#include "exa_launch.hpp"
#include "exa_pde.hpp"

namespace exa {

#define EXA_LIM_CASES(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

struct LimFaceKinds { int k[6]; };          // include/exahype_hip.h EXA_LIM_FACE_*

template <int DIM, int N> struct LimScan {
    static constexpr int NN = DIM == 3 ? N * N * N : N * N;
    static constexpr int TPC = NN <= 64 ? 64 : 256;                // threads per cell
    static constexpr int CPB = 256 / TPC;                          // cells per workgroup
};

// Euler layout: rho first, energy last, min(3, nv - 2) momenta behind rho, gamma = 1.4; the DMP watches rho and E
template <int NV_> struct LimEulerCrit {
    static constexpr int NV = NV_;
    static constexpr int K_DMP = 2;
    __device__ static inline int dmp_var(int k, int nv) { return k == 0 ? 0 : nv - 1; }
    __device__ static inline bool troubled(const double* s, int nv, double floor) {
        const int nm = nv - 2 < 3 ? nv - 2 : 3;
        const double rho = s[0];
        double ke = 0.0;
        for (int a = 0; a < nm; a++) ke += s[1 + a] * s[1 + a];
        const double p = 0.4 * (s[nv - 1] - 0.5 * ke / rho);
        return !(rho > floor) || !(p > floor);
    }
};

// a generated term set's own criterion: every g_k(q) > floor (PDE::admissible), DMP on PDE::DMP_VAR
template <class PDE> struct LimPdeCrit {
    static_assert(pde_has_admissible<PDE>::value, "the term set carries no admissibility criterion");
    static constexpr int NV = PDE::NV;
    static constexpr int K_DMP = PDE::K_DMP;
    __device__ static inline int dmp_var(int k, int) { return PDE::dmp_var(k); }
    __device__ static inline bool troubled(const double* s, int, double floor) {
        if constexpr (PDE::K_ADM > 0) {
            double g[PDE::K_ADM];
            PDE::admissible(s, g);
            bool bad = false;
#pragma unroll
            for (int k = 0; k < PDE::K_ADM; k++) bad = bad || !(g[k] > floor);
            return bad;
        } else {
            return false;
        }
    }
};

__device__ inline double lim_max(double a, double b) { return a > b ? a : b; }

// max over the TPC threads of a cell; every thread of the cell gets the result.  red: [4 waves][K]
template <int K, int TPC>
__device__ inline void lim_reduce_max(double (&m)[K], double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < K; k++) m[k] = lim_max(m[k], __shfl_xor(m[k], off, 64));
    if constexpr (TPC == 256) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0)
#pragma unroll
            for (int k = 0; k < K; k++) red[wave * K + k] = m[k];
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; w++)
#pragma unroll
            for (int k = 0; k < K; k++) m[k] = lim_max(m[k], red[w * K + k]);
    }
}

// lo / hi [K]: minimum / maximum of bounds[..][2 K] over the cell and its 2 DIM face neighbours -- the periodic wrap inside the block, the
// neighbour block's bounds (EXA_LIM_FACE_GHOST: gb.layer[face][transverse cell][2 K]), or no neighbour at all (EXA_LIM_FACE_NONE)
template <int DIM, int K>
__device__ inline void lim_neighbourhood(long cell, const long (&nc)[3], const double* __restrict__ bounds, const LimGhosts& gb,
                                         const LimFaceKinds& fk, double (&lo)[K], double (&hi)[K]) {
    long cc[3];
    { long b = cell; cc[2] = b % nc[2]; b /= nc[2]; cc[1] = b % nc[1]; cc[0] = b / nc[1]; }
    const double* own = bounds + cell * (2 * K);
#pragma unroll
    for (int k = 0; k < K; k++) { lo[k] = own[2 * k]; hi[k] = own[2 * k + 1]; }
    for (int a = 0; a < DIM; a++)
        for (int side = 0; side < 2; side++) {
            const double* b;
            const int kind = fk.k[a * 2 + side];
            if (kind != 0 && cc[a] == (side ? nc[a] - 1 : 0)) {
                if (kind != 1) continue;                       // a face with a boundary condition: no neighbour
                long tc = 0;
                for (int c = 0; c < DIM; c++)
                    if (c != a) tc = tc * nc[c] + cc[c];
                b = gb.layer[a * 2 + side] + tc * (2 * K);     // the neighbour block's bounds arrived by exchange
            } else {
                long nb[3] = {cc[0], cc[1], cc[2]};
                nb[a] = (nb[a] + (side ? 1 : nc[a] - 1)) % nc[a];
                b = bounds + ((nb[0] * nc[1] + nb[1]) * nc[2] + nb[2]) * (2 * K);
            }
#pragma unroll
            for (int k = 0; k < K; k++) {
                lo[k] = b[2 * k] < lo[k] ? b[2 * k] : lo[k];
                hi[k] = b[2 * k + 1] > hi[k] ? b[2 * k + 1] : hi[k];
            }
        }
}

template <int DIM, int N, class Crit>
__global__ void __launch_bounds__(256)
limiter_snapshot_kernel(int nv_rt, long ncells, const double* __restrict__ u, double* __restrict__ u_old, double* __restrict__ bounds) {
    using LS = LimScan<DIM, N>;
    constexpr int TPC = LS::TPC, KD = Crit::K_DMP, KM = KD > 0 ? 2 * KD : 1;
    __shared__ double red[4 * KM];
    const int nv = Crit::NV ? Crit::NV : nv_rt;
    const int len = LS::NN * nv;
    const int t = threadIdx.x % TPC;
    const long cell = (long)blockIdx.x * LS::CPB + threadIdx.x / TPC;
    const bool live = cell < ncells;
    const double ninf = -__builtin_huge_val();
    double m[KM];                                                  // per watched variable: -min, max
#pragma unroll
    for (int k = 0; k < KM; k++) m[k] = ninf;
    if (live) {
        const double* src = u + cell * len;
        double* dst = u_old ? u_old + cell * len : nullptr;
#pragma unroll 4
        for (int i = t; i < len; i += TPC) {
            const double x = src[i];
            if (dst) dst[i] = x;
            if constexpr (KD > 0) {
                const int v = i % nv;
#pragma unroll
                for (int k = 0; k < KD; k++)
                    if (v == Crit::dmp_var(k, nv)) { m[2 * k] = lim_max(m[2 * k], -x); m[2 * k + 1] = lim_max(m[2 * k + 1], x); }
            }
        }
    }
    if constexpr (KD > 0) {
        lim_reduce_max<KM, TPC>(m, red);
        if (live && t == 0) {
            double* b = bounds + cell * (2 * KD);
#pragma unroll
            for (int k = 0; k < KD; k++) { b[2 * k] = -m[2 * k]; b[2 * k + 1] = m[2 * k + 1]; }
        }
    }
}

template <int DIM, int N, class Crit>
__global__ void __launch_bounds__(256)
limiter_detect_kernel(int nv_rt, long nc0, long nc1, long nc2, const double* __restrict__ u, const double* __restrict__ bounds,
                      LimGhosts gb, LimFaceKinds fk, double d0, double eps, double floor, unsigned char* __restrict__ mask) {
    using LS = LimScan<DIM, N>;
    constexpr int TPC = LS::TPC, NN = LS::NN, KD = Crit::K_DMP, KM = 2 * KD + 1;
    extern __shared__ __attribute__((aligned(16))) double lim_sm[];            // [cells per workgroup][NN][nv]
    __shared__ double red[4 * KM];
    const int nv = Crit::NV ? Crit::NV : nv_rt;
    const int len = NN * nv;
    const int t = threadIdx.x % TPC;
    const long nc[3] = {nc0, nc1, DIM == 3 ? nc2 : 1};
    const long ncells = nc[0] * nc[1] * nc[2];
    const long cell = (long)blockIdx.x * LS::CPB + threadIdx.x / TPC;
    const bool live = cell < ncells;
    double* q = lim_sm + (size_t)(threadIdx.x / TPC) * len;
    const double ninf = -__builtin_huge_val();
    double m[KM];                                                  // per watched variable: -min, max; the last: troubled
#pragma unroll
    for (int k = 0; k < 2 * KD; k++) m[k] = ninf;
    m[2 * KD] = 0.0;
    if (live) {
        const double* src = u + cell * len;
#pragma unroll 4
        for (int i = t; i < len; i += TPC) {
            const double x = src[i];
            q[i] = x;
            if (!(__builtin_fabs(x) <= 1.7976931348623157e308)) m[2 * KD] = 1.0;      // NaN, +-inf
            if constexpr (KD > 0) {
                const int v = i % nv;
#pragma unroll
                for (int k = 0; k < KD; k++)
                    if (v == Crit::dmp_var(k, nv)) { m[2 * k] = lim_max(m[2 * k], -x); m[2 * k + 1] = lim_max(m[2 * k + 1], x); }
            }
        }
    }
    __syncthreads();
    if (live) {
        for (int n = t; n < NN; n += TPC)
            if (Crit::troubled(q + n * nv, nv, floor)) m[2 * KD] = 1.0;
    }
    lim_reduce_max<KM, TPC>(m, red);
    if (live && t == 0) {
        bool bad = m[2 * KD] != 0.0;
        if constexpr (KD > 0) {
            double lo[KD], hi[KD];
            lim_neighbourhood<DIM, KD>(cell, nc, bounds, gb, fk, lo, hi);
#pragma unroll
            for (int k = 0; k < KD; k++) {
                const double delta = lim_max(d0, eps * (hi[k] - lo[k]));
                const double cmin = -m[2 * k], cmax = m[2 * k + 1];
                if (!(cmax <= hi[k] + delta) || !(cmin >= lo[k] - delta)) bad = true;
            }
        }
        mask[cell] = bad ? 1 : 0;
    }
}

// u^n -> u_old (may be null) + bounds[cell][2 K_DMP]
template <class Crit>
int lim_snapshot_launch(int dim, int N, int nv, long ncells, const double* u, double* u_old, double* bounds, hipStream_t s) {
    if (ncells <= 0) return 0;
    if (Crit::K_DMP == 0 && !u_old) return 0;                      // nothing to write
    switch (N) {
#define X(NN_)                                                                                                                         \
    case NN_: {                                                                                                                        \
        const unsigned g2 = (unsigned)((ncells + LimScan<2, NN_>::CPB - 1) / LimScan<2, NN_>::CPB);                                    \
        const unsigned g3 = (unsigned)((ncells + LimScan<3, NN_>::CPB - 1) / LimScan<3, NN_>::CPB);                                    \
        if (dim == 2) hipLaunchKernelGGL((limiter_snapshot_kernel<2, NN_, Crit>), dim3(g2), dim3(256), 0, s, nv, ncells, u, u_old, bounds); \
        else hipLaunchKernelGGL((limiter_snapshot_kernel<3, NN_, Crit>), dim3(g3), dim3(256), 0, s, nv, ncells, u, u_old, bounds);     \
        break;                                                                                                                         \
    }
        EXA_LIM_CASES(X)
#undef X
    default: set_error("limiter: N = %d is not built", N); return -1;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("limiter_snapshot launch: %s", hipGetErrorString(e)); return -2; }
    return 0;
}

// candidate + bounds (+ neighbour blocks' bounds) -> mask bytes
template <class Crit>
int lim_detect_launch(int dim, int N, int nv, const long* nc, const double* u, const double* bounds, const LimGhosts* ghosts, const int* kinds,
                      double d0, double eps, double floor, unsigned char* mask, hipStream_t s) {
    const long nc2 = dim == 3 ? nc[2] : 1;
    const long ncells = nc[0] * nc[1] * nc2;
    if (ncells <= 0) return 0;
    LimGhosts gb{};
    if (ghosts) gb = *ghosts;
    LimFaceKinds fk{};
    for (int f = 0; f < 2 * dim; f++) fk.k[f] = kinds ? kinds[f] : 0;
    long nn = 1;
    for (int a = 0; a < dim; a++) nn *= N;
    const size_t bytes = sizeof(double) * (size_t)nn * nv * (nn <= 64 ? 4 : 1);
    if (bytes > 64 * 1024) { set_error("limiter_detect: a cell of %ld nodes x %d variables does not fit the kernel's LDS buffer", nn, nv); return -1; }
    switch (N) {
#define X(NN_)                                                                                                                         \
    case NN_: {                                                                                                                        \
        const unsigned g2 = (unsigned)((ncells + LimScan<2, NN_>::CPB - 1) / LimScan<2, NN_>::CPB);                                    \
        const unsigned g3 = (unsigned)((ncells + LimScan<3, NN_>::CPB - 1) / LimScan<3, NN_>::CPB);                                    \
        if (dim == 2) hipLaunchKernelGGL((limiter_detect_kernel<2, NN_, Crit>), dim3(g2), dim3(256), bytes, s, nv, nc[0], nc[1], nc2, u, bounds, gb, fk, d0, eps, floor, mask); \
        else hipLaunchKernelGGL((limiter_detect_kernel<3, NN_, Crit>), dim3(g3), dim3(256), bytes, s, nv, nc[0], nc[1], nc2, u, bounds, gb, fk, d0, eps, floor, mask);     \
        break;                                                                                                                         \
    }
        EXA_LIM_CASES(X)
#undef X
    default: set_error("limiter: N = %d is not built", N); return -1;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("limiter_detect launch: %s", hipGetErrorString(e)); return -2; }
    return 0;
}

}  // namespace exa

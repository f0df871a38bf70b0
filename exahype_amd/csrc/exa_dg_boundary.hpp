// Domain-boundary ghosts of the ADER-DG stage B (no counterpart in the reference).
//
// Stage B reads the state beyond a block face from ghost[d*2+side], layout [transverse cell][2*NV*NF] with the entry
// (field*NV + v)*NF + y (field 0 = time-averaged state, 1 = time-averaged normal flux) -- what exa_dg_pack_face writes.  A halo exchange
// fills those buffers from the neighbour block; the two kernels here fill them from a boundary condition instead:
//   dg_bc_gather_kernel     ghost = c (.) the block's own outward trace at that face; one factor per (field, v): all 1 = outflow,
//                           (s, -s) = reflecting wall (exact where F_d(S q) = -S F_d(q), S = diag(s))
//   dg_bc_dirichlet_kernel  ghost = the time average of a prescribed state and of its normal flux over the step's Gauss time levels
//                           (or one constant state), and the largest eigenvalue of those states folded into an optional device scalar.
// Both are element-wise over the face (no LDS); every store is a vector store of one lane.
#pragma once
#include <hip/hip_runtime.h>
#include "exa_dg_common.hpp"
#include "exa_pde.hpp"

namespace exa {

// the face (d, side) of a block nc[3]: transverse cell t (lexicographic over the other axes, last fastest) -> cell index / coordinates
struct BcFace {
    long nc[3];
    long ncells;
    int d, side;
    __host__ __device__ inline long inner() const { long r = 1; for (int a = d + 1; a < 3; a++) r *= nc[a]; return r; }
    __host__ __device__ inline long ntrans() const { return ncells / nc[d]; }
    __device__ inline long cell(long t) const {
        const long in = inner(), o = t / in, i = t - o * in;
        return (o * nc[d] + (side ? nc[d] - 1 : 0)) * in + i;
    }
    __device__ inline void coords(long t, long* cc) const {
        const long c = cell(t);
        cc[2] = c % nc[2];
        cc[1] = (c / nc[2]) % nc[1];
        cc[0] = c / (nc[1] * nc[2]);
    }
};

template <int NV> struct BcScale { double c[2 * NV]; };   // factor of (field, v)

// one lane per (transverse cell, field, v, y): ghost[t][r] = c[r / NF] * trace[(d*2+side)][cell(t)][r], r over 2*NV*NF (coalesced)
template <int NV>
__global__ void __launch_bounds__(256)
dg_bc_gather_kernel(const double* __restrict__ trace, double* __restrict__ ghost, BcFace f, int NF, BcScale<NV> sc) {
    const long TS = 2L * NV * NF;
    const long n = f.ntrans() * TS;
    for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < n; g += (long)gridDim.x * blockDim.x) {
        const long t = g / TS;
        const int r = (int)(g - t * TS), fv = r / NF;
        double k = sc.c[0];                                   // (a select chain: no run-time index into the argument block)
#pragma unroll
        for (int j = 1; j < 2 * NV; j++) k = fv == j ? sc.c[j] : k;
        ghost[g] = k * trace[((long)(f.d * 2 + f.side) * f.ncells + f.cell(t)) * TS + r];
    }
}

template <int N> struct BcLevels {
    double w[N];        // time weights (Gauss-Legendre on [0, 1]; one level: 1)
    double t[N];        // level times t0 + xi_l dt (one level: t0 + dt / 2)
};
template <int NV> struct BcState { double q[NV]; };

// one lane per (transverse cell, face node y): states[t][y][l][NV] (or the constant state), L = N time levels (or 1);
// ghost[t][(field*NV + v)*NF + y] = sum_l w_l (q_l, F_d(q_l, x_y, t_l)); lam (optional) = max(lam, max_{l, d'} lambda_d'(q_l))
template <int DIM, int N, class PDE>
__global__ void __launch_bounds__(256)
dg_bc_dirichlet_kernel(const double* __restrict__ states, BcState<PDE::NV> cq, double* __restrict__ ghost, BcFace f, BcLevels<N> lv,
                       PlainGeo geo, double* lam) {
    constexpr int NV = PDE::NV, NF = ipow(N, DIM - 1), TS = 2 * NV * NF;
    const long n = f.ntrans() * NF;
    double m = 0.0;
    for (long g = blockIdx.x * (long)blockDim.x + threadIdx.x; g < n; g += (long)gridDim.x * blockDim.x) {
        const long t = g / NF;
        const int y = (int)(g - t * NF);
        double x[3] = {0.0, 0.0, 0.0};
        if constexpr (pde_has_xt<PDE>::value) {                // face node position, as stage B places it (face_node_coords)
            long cc[3];
            f.coords(t, cc);
#pragma unroll
            for (int a = 0; a < DIM; a++) {
                const int j = a < f.d ? a : a - 1;             // rank of axis a among the transverse ones
                const int i = DIM == 3 ? (j == 0 ? y / N : y % N) : y;
                x[a] = a == f.d ? geo.x0[a] + (double)(cc[a] + f.side) * geo.h[a] : geo.x0[a] + ((double)cc[a] + xi_of<N>(geo, i)) * geo.h[a];
            }
        }
        double qs[NV], Fs[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) { qs[v] = 0.0; Fs[v] = 0.0; }
        // a constant state: one level of weight 1 -- unless the flux sees x / t, then F(q, x_y, t_l) is averaged over the levels like a
        // function's (the interior's flux is Gauss-averaged too) while the state stays q itself, not sum_l w_l q
        constexpr bool XT = pde_has_xt<PDE>::value;
        const int L = (states || XT) ? N : 1;
#pragma unroll
        for (int l = 0; l < N; l++) {
            if (l >= L) break;
            double q[NV], F[NV];
#pragma unroll
            for (int v = 0; v < NV; v++) {
                q[v] = states ? states[((t * NF + y) * N + l) * NV + v] : cq.q[v];
                F[v] = 0.0;                                   // (a term set may write only its first NFLUX entries)
            }
            const double wl = L > 1 ? lv.w[l] : 1.0, tl = lv.t[l];
            fv_flux<PDE>(q, x, tl, f.d, F);
#pragma unroll
            for (int v = 0; v < NV; v++) {
                qs[v] = states ? qs[v] + wl * q[v] : q[v];
                Fs[v] += wl * F[v];
            }
            if (lam) {
#pragma unroll
                for (int a = 0; a < DIM; a++) m = nan_max(m, fv_eig<PDE>(q, x, tl, a));
            }
        }
        double* out = ghost + t * TS + y;
#pragma unroll
        for (int v = 0; v < NV; v++) {
            out[v * NF] = qs[v];
            out[(NV + v) * NF] = Fs[v];
        }
    }
    if (lam) {                                                // as stage_b_cfl_scan: wave maximum, one integer atomic per wave
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
        if ((threadIdx.x & 63) == 0) {
            unsigned long long* lb = reinterpret_cast<unsigned long long*>(lam);
            const unsigned long long mine = (unsigned long long)__double_as_longlong(m);
            if (mine > __hip_atomic_load(lb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(lb, mine);
        }
    }
}

}  // namespace exa

// FV subcell limiter glue for the ADER-DG path (BASELINE configs[4]; no counterpart in the
// reference).  The kernels around the fused FV Rusanov patch kernel (fv_rusanov.hip, the reference's kernel
// shape with patch_size = 2p+1, halo_size = 1):
//   limiter_project_halo1_kernel    troubled cell -> FV patch: interior = (P x P x P) u, face halos = the adjacent
//                                   subcell layer of the face neighbours' projections (periodic in the block, or the ghost layer
//                                   of a sharded grid's block face), edge and corner halo entries = nearest interior value
//                                   (never read by the 7-point stencil)
//   limiter_face_layers_kernel      the subcell layers at a block face that the neighbour block's patches take as ghost layers
//   limiter_reconstruct_halo_kernel FV patch interior -> DG nodes: u = (R x R x R) v; a template over the patches' halo (1 | 2)
// and, for the second-order patch update (exa_fv_muscl.hpp: halo_size = 2, reads the edge entries),
//   limiter_project_halo2_kernel    troubled cell -> FV patch with halo 2: face halos two layers deep, edge entries from the diagonal
//                                   cells, mirror / state domain faces
// One workgroup per troubled cell (face layers: per cell of the block's boundary layer).  One form for every variable count: a lane
// carries NV variables of an output element through lim_apply_v, the nv variables go in nv / NV rounds (lim_launch picks NV = 5 or 1).
// One per-variable kernel of the earlier generation stays, limiter_reconstruct_kernel<3, 8, H> (NOT MERGED, further down).
// The kernels are instantiated per order (N, N_s compile-time): with run-time extents every output element paid three integer
// divisions (~100 instructions) for its 8 FMAs -- 7.6 ms per step for the 13 K patches of cfg 4's per-GPU shape, 8 % of the step.
#include <cstdio>
#include <cstdlib>
#include "exa_launch.hpp"
#include "exa_lim_conserve.hpp"
#include "exa_lim_detect.hpp"
#include "exa_pde.hpp"

namespace exa {

// ------------------------------------------------------------------------------------------------------------------
// A lane carries NV variables of an output element.  With NV = nv = 5 the cell's u, the patch and the face layers move as
// contiguous AoS runs; with NV = 1 every global access is an 8-byte element at a stride of nv doubles.  The last pass of every
// product writes straight to global memory, and a projected cell costs 29 barriers per round.  LDS: two buffers, max(N^3, N_s^2 N)
// and N_s N^2 elements of NV doubles (110 KB at N = 8, NV = 5: one workgroup per CU), and the operator.  Summation order, in
// every instantiation: acc = 0, c ascending, acc += m * in -- the results do not depend on NV, bit for bit.
// ------------------------------------------------------------------------------------------------------------------
template <int DIM, int N> struct LimBuf {
    // one workgroup per CU at the large orders (LDS): give it the waves.  cfg 4's shape (N = 8, 13 K patches), per launch:
    // project 3.76 / 2.90 / 2.46 ms and reconstruct 1.92 / 1.61 / 1.65 ms with 256 / 512 / 1024 threads (per-variable kernels: 5.41, 2.15)
    static constexpr int NT = (DIM == 3 && N >= 5) ? 1024 : 256;             // projection
    static constexpr int NT_R = (DIM == 3 && N >= 5) ? 512 : 256;            // reconstruction
    // the halo-1 projection with one variable per lane (22 KB of LDS at N = 8): several workgroups share a CU, and NT threads only lengthen
    // their barriers -- 3-D N = 8, one | two variables, 13 K patches: 1.10 | 2.07 ms with NT threads, 0.42 | 1.00 ms with 256; the
    // reconstruction is the other way round (two variables: 0.86 ms with NT_R threads, 1.57 ms with 256): profiles/limiter_unit_refactor.txt
    static constexpr int NT1 = 256;                                          // halo-1 projection with NV = 1; face layers
    static constexpr int Ns = 2 * N - 1;
    static constexpr int NN = DIM == 3 ? N * N * N : N * N;
    static constexpr int B1 = DIM == 3 ? (NN > Ns * Ns * N ? NN : Ns * Ns * N) : Ns * N;  // project: in | after two passes; reconstruct: after one
    static constexpr int B2 = DIM == 3 ? Ns * N * N : Ns * N;                               // project: after one pass; reconstruct: after two
    static constexpr int F1 = NN, F2 = NN / N;                               // face layers: in | after one pass (one row of P); 3-D: N_s N <= N^3 after two
};

// out(t, acc[NV]) for t over (outer, nr, inner);  acc[v] = sum_c M[r0 + rstep r][c] * in((o*C + c)*inner + in_i, v)
// rstep = -1: the rows in descending order (a mirror image across a domain face); same sums, same order
template <int C, int NV, class In, class Out>
__device__ inline void lim_apply_v(const double* M, int ldm, int r0, int nr, int dim, const int* e, int axis, In in, Out out, int rstep = 1) {
    unsigned inner = 1, outer = 1;
    for (int a = axis + 1; a < dim; a++) inner *= e[a];
    for (int a = 0; a < axis; a++) outer *= e[a];
    const unsigned total = outer * nr * inner;
    for (unsigned t = threadIdx.x; t < total; t += blockDim.x) {
        const unsigned q = t / inner, in_i = t - q * inner;
        const unsigned o = q / (unsigned)nr, r = q - o * nr;
        const double* mr = M + (r0 + rstep * (int)r) * ldm;
        double acc[NV];
#pragma unroll
        for (int v = 0; v < NV; v++) acc[v] = 0.0;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const double m = mr[c];
            const unsigned src = (o * C + c) * inner + in_i;
#pragma unroll
            for (int v = 0; v < NV; v++) acc[v] += m * in(src, v);
        }
        out(t, acc);
    }
}

template <int DIM, int N, int NV, bool ONE>
__global__ void __launch_bounds__((NV == 1 ? LimBuf<DIM, N>::NT1 : LimBuf<DIM, N>::NT))
limiter_project_halo1_kernel(int nv, long nc0, long nc1, long nc2, const double* __restrict__ u, const long* __restrict__ cells,
                             double* __restrict__ patch, const double* __restrict__ P_global, LimGhosts gh) {
    extern __shared__ __attribute__((aligned(16))) double lim_sm[];
    const int nvs = ONE ? NV : nv;                                 // ONE: nv == NV, one round, the stride a compile-time value
    using LB = LimBuf<DIM, N>;
    constexpr int Ns = LB::Ns, S = Ns + 2, NN = LB::NN;
    constexpr int SS = DIM == 3 ? S * S * S : S * S, LAYER = DIM == 3 ? Ns * Ns : Ns;
    double* X = lim_sm;
    double* Y = lim_sm + (size_t)LB::B1 * NV;
    __shared__ double Psh[Ns * N];                                 // the operator: every FMA reads an entry (a few distinct ones per wave)
    const long cell = cells[blockIdx.x];
    if (cell < 0) return;                                          // empty slot of a capacity-sized cell list
    for (int t = threadIdx.x; t < Ns * N; t += blockDim.x) Psh[t] = P_global[t];
    const double* P = Psh;                                         // (visible after the barrier behind the first load of u)
    double* pt = patch + (long)blockIdx.x * SS * nvs;
    const long nc[3] = {nc0, nc1, nc2};
    long cc[3];
    { long b = cell; cc[2] = DIM == 3 ? b % nc2 : 0; if (DIM == 3) b /= nc2; cc[1] = b % nc1; cc[0] = b / nc1; }
    auto fromX = [&](unsigned i, int v) { return X[i * NV + v]; };
    auto fromY = [&](unsigned i, int v) { return Y[i * NV + v]; };
    auto toX = [&](unsigned t, const double (&a)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; v++) X[t * NV + v] = a[v];
    };
    auto toY = [&](unsigned t, const double (&a)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; v++) Y[t * NV + v] = a[v];
    };
    for (int v0 = 0; v0 < nvs; v0 += NV) {
        auto load_cell = [&](long c) {                             // X <- the NV variables of cell c (NV == nv: one contiguous run)
            __syncthreads();                                       // X and Y are free (the previous product has written its result)
            for (int t = threadIdx.x; t < NN * NV; t += blockDim.x) X[t] = u[(c * NN + t / NV) * nvs + v0 + t % NV];
            __syncthreads();
        };
        // ---- own projection: u -> X -> Y (-> X) -> patch interior
        load_cell(cell);
        {
            int e[3] = {N, N, N};
            lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, 0, fromX, toY);
            e[0] = Ns;
            __syncthreads();
            auto to_patch = [&](unsigned t, const double (&a)[NV]) {
                unsigned r = t;
                long flat = 0, mul = 1;
#pragma unroll
                for (int ax = DIM - 1; ax >= 0; ax--) { flat += (long)(r % Ns + 1) * mul; mul *= S; r /= Ns; }
#pragma unroll
                for (int v = 0; v < NV; v++) pt[flat * nvs + v0 + v] = a[v];
            };
            if constexpr (DIM == 3) {
                lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, 1, fromY, toX);
                e[1] = Ns;
                __syncthreads();
                lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, 2, fromX, to_patch);
            } else {
                lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, 1, fromY, to_patch);
            }
        }
        __syncthreads();                                           // the interior is in global memory, visible to the workgroup
        // edge and corner halo entries (>= 2 halo coordinates; never read by the 7-point stencil): nearest interior value
        for (int t = threadIdx.x; t < SS; t += blockDim.x) {
            int I[3] = {0, 0, 0}, r = t, nh = 0;
            for (int a = DIM - 1; a >= 0; a--) { I[a] = r % S; r /= S; nh += (I[a] == 0 || I[a] == S - 1) ? 1 : 0; }
            if (nh < 2) continue;
            long flat = 0;
            for (int a = 0; a < DIM; a++) {
                const int ci = I[a] < 1 ? 1 : (I[a] > Ns ? Ns : I[a]);
                flat = flat * S + ci;
            }
#pragma unroll
            for (int v = 0; v < NV; v++) pt[(long)t * nvs + v0 + v] = pt[flat * nvs + v0 + v];
        }
        // ---- face halos: the adjacent subcell layer of the face neighbours' projections
        for (int a = 0; a < DIM; a++)
            for (int side = 0; side < 2; side++) {
                auto to_layer = [&](unsigned t, const double (&acc)[NV]) {   // t enumerates the transverse subcells (axes != a, lexicographic)
                    unsigned r = t;
                    int idx[3] = {0, 0, 0};
                    for (int b = DIM - 1; b >= 0; b--) {
                        if (b == a) continue;
                        idx[b] = r % Ns + 1;
                        r /= Ns;
                    }
                    idx[a] = side ? S - 1 : 0;
                    long flat = 0;
                    for (int b = 0; b < DIM; b++) flat = flat * S + idx[b];
#pragma unroll
                    for (int v = 0; v < NV; v++) pt[flat * nvs + v0 + v] = acc[v];
                };
                const double* g = gh.layer[a * 2 + side];
                if (g && cc[a] == (side ? nc[a] - 1 : 0)) {
                    // block boundary of a sharded grid: the neighbour's adjacent subcell layer arrived by exchange,
                    // layout [transverse cell][transverse subcell][var] (limiter_face_layers_kernel on the neighbour)
                    long tc = 0;
                    for (int b = 0; b < DIM; b++)
                        if (b != a) tc = tc * nc[b] + cc[b];
                    const double* gl = g + tc * LAYER * nvs;
                    for (int t = threadIdx.x; t < LAYER; t += blockDim.x) {
                        double acc[NV];
#pragma unroll
                        for (int v = 0; v < NV; v++) acc[v] = gl[(long)t * nvs + v0 + v];
                        to_layer(t, acc);
                    }
                    continue;
                }
                long nb[3] = {cc[0], cc[1], cc[2]};
                nb[a] = (nb[a] + (side ? 1 : nc[a] - 1)) % nc[a];
                load_cell((nb[0] * nc1 + nb[1]) * (DIM == 3 ? nc2 : 1) + nb[2]);
                int e2[3] = {N, N, N};
                const int b0 = a, b1 = (a + 1) % DIM, b2 = (a + 2) % DIM;
                lim_apply_v<N, NV>(P, N, side ? 0 : Ns - 1, 1, DIM, e2, b0, fromX, toY);  // normal axis first: the adjacent layer only
                e2[b0] = 1;
                __syncthreads();
                if constexpr (DIM == 3) {
                    lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e2, b1, fromY, toX);
                    e2[b1] = Ns;
                    __syncthreads();
                    lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e2, b2, fromX, to_layer);
                } else {
                    lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e2, b1, fromY, to_layer);
                }
            }
    }
}

// Sharded grids: the subcell layer next to the block face (a, side) of every cell of the block's boundary layer whose
// neighbour across the face is troubled (need[t] != 0; need == nullptr: all) -- what that neighbour's patch needs as
// halo.  out[transverse cell][transverse subcell][var]; one workgroup per transverse cell.  The sums and their order are those of
// the face halos of the projection kernels: a layer that travels as a ghost buffer equals the periodic one bit for bit.
template <int DIM, int N, int NV, bool ONE>
__global__ void __launch_bounds__((LimBuf<DIM, N>::NT1))
limiter_face_layers_kernel(int nv, long nc0, long nc1, long nc2, const double* __restrict__ u, int a, int side,
                           const double* __restrict__ need, double* __restrict__ out, const double* __restrict__ P_global) {
    extern __shared__ __attribute__((aligned(16))) double lim_sm[];
    const int nvs = ONE ? NV : nv;                                 // ONE: nv == NV, one round, the stride a compile-time value
    using LB = LimBuf<DIM, N>;
    constexpr int Ns = LB::Ns, NN = LB::NN, LAYER = DIM == 3 ? Ns * Ns : Ns;
    double* X = lim_sm;
    double* Y = lim_sm + (size_t)LB::F1 * NV;
    __shared__ double Psh[Ns * N];
    const long tc = blockIdx.x;
    if (need && need[tc] == 0.0) return;                           // nobody across the face takes this cell's layer
    for (int t = threadIdx.x; t < Ns * N; t += blockDim.x) Psh[t] = P_global[t];
    const double* P = Psh;                                         // (visible after the barrier behind the first load of u)
    const long nc[3] = {nc0, nc1, nc2};
    long cc[3] = {0, 0, 0};
    { long r = tc; for (int b = DIM - 1; b >= 0; b--) { if (b == a) continue; cc[b] = r % nc[b]; r /= nc[b]; } }
    cc[a] = side ? nc[a] - 1 : 0;
    const long cell = (cc[0] * nc1 + cc[1]) * (DIM == 3 ? nc2 : 1) + cc[2];
    auto fromX = [&](unsigned i, int v) { return X[i * NV + v]; };
    auto fromY = [&](unsigned i, int v) { return Y[i * NV + v]; };
    auto toX = [&](unsigned t, const double (&acc)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; v++) X[t * NV + v] = acc[v];
    };
    auto toY = [&](unsigned t, const double (&acc)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; v++) Y[t * NV + v] = acc[v];
    };
    for (int v0 = 0; v0 < nvs; v0 += NV) {
        __syncthreads();                                           // X and Y are free (the previous round has written its result)
        for (int t = threadIdx.x; t < NN * NV; t += blockDim.x) X[t] = u[(cell * NN + t / NV) * nvs + v0 + t % NV];
        __syncthreads();
        auto to_out = [&](unsigned t, const double (&acc)[NV]) {   // t enumerates the transverse subcells (axes != a, lexicographic)
#pragma unroll
            for (int v = 0; v < NV; v++) out[(tc * LAYER + t) * nvs + v0 + v] = acc[v];
        };
        int e[3] = {N, N, N};
        const int b0 = a, b1 = (a + 1) % DIM, b2 = (a + 2) % DIM;
        lim_apply_v<N, NV>(P, N, side ? Ns - 1 : 0, 1, DIM, e, b0, fromX, toY);           // normal axis first: the layer at the face only
        e[b0] = 1;
        __syncthreads();
        if constexpr (DIM == 3) {
            lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, b1, fromY, toX);
            e[b1] = Ns;
            __syncthreads();
            lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, b2, fromX, to_out);
        } else {
            lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, b1, fromY, to_out);
        }
    }
}

// H: halo layers of the patches (1: the first-order update's, 2: the second-order update's); the interior is read at offset H
template <int DIM, int N, int NV, bool ONE, int H>
__global__ void __launch_bounds__((LimBuf<DIM, N>::NT_R))
limiter_reconstruct_halo_kernel(int nv, const double* __restrict__ patch, const long* __restrict__ cells, double* __restrict__ u,
                                const double* __restrict__ R_global) {
    extern __shared__ __attribute__((aligned(16))) double lim_sm[];
    const int nvs = ONE ? NV : nv;                                 // ONE: nv == NV, one round, the stride a compile-time value
    using LB = LimBuf<DIM, N>;
    constexpr int Ns = LB::Ns, S = Ns + 2 * H, NN = LB::NN;
    constexpr int SS = DIM == 3 ? S * S * S : S * S;
    double* X = lim_sm;                                            // N_s^2 N (3-D) | N_s N (2-D): after one pass
    double* Y = lim_sm + (size_t)LB::B1 * NV;                      // N_s N^2: after two
    __shared__ double Rsh[N * Ns];
    const long cell = cells[blockIdx.x];
    if (cell < 0) return;                                          // empty slot
    for (int t = threadIdx.x; t < N * Ns; t += blockDim.x) Rsh[t] = R_global[t];
    const double* R = Rsh;
    const double* pt = patch + (long)blockIdx.x * SS * nvs;
    auto fromX = [&](unsigned i, int v) { return X[i * NV + v]; };
    auto fromY = [&](unsigned i, int v) { return Y[i * NV + v]; };
    auto toX = [&](unsigned t, const double (&a)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; v++) X[t * NV + v] = a[v];
    };
    auto toY = [&](unsigned t, const double (&a)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; v++) Y[t * NV + v] = a[v];
    };
    for (int v0 = 0; v0 < nvs; v0 += NV) {
        auto from_patch = [&](unsigned i, int v) {                 // logical N_s^DIM index -> interior of the padded patch
            unsigned r = i;
            long flat = 0, mul = 1;
#pragma unroll
            for (int a = DIM - 1; a >= 0; a--) { flat += (long)(r % Ns + H) * mul; mul *= S; r /= Ns; }
            return pt[flat * nvs + v0 + v];
        };
        auto to_u = [&](unsigned t, const double (&a)[NV]) {
#pragma unroll
            for (int v = 0; v < NV; v++) u[(cell * NN + t) * nvs + v0 + v] = a[v];
        };
        __syncthreads();                                           // the operator's copy is visible; X and Y are free (the previous round has written its result)
        int e[3] = {Ns, Ns, Ns};
        lim_apply_v<Ns, NV>(R, Ns, 0, N, DIM, e, 0, from_patch, toX);
        e[0] = N;
        __syncthreads();
        if constexpr (DIM == 3) {
            lim_apply_v<Ns, NV>(R, Ns, 0, N, DIM, e, 1, fromX, toY);
            e[1] = N;
            __syncthreads();
            lim_apply_v<Ns, NV>(R, Ns, 0, N, DIM, e, 2, fromY, to_u);
        } else {
            lim_apply_v<Ns, NV>(R, Ns, 0, N, DIM, e, 1, fromX, to_u);
        }
    }
}

// NOT MERGED (profiles/limiter_unit_refactor.txt): the reconstruction at 3-D N = 8 of variable counts that five does not divide, other than
// one.  limiter_reconstruct_halo_kernel<3, 8, 1, false, H> reads the patch from global memory in its first pass, N times per entry at a run-time
// stride, and the compiler issues those loads two at a time between their address arithmetic: 0.86 ms against 0.73 ms per launch at two variables.
// The kernel below, the one that served every variable count but five before, copies the patch interior into LDS once per variable and runs the
// three passes there (one variable at a time through two static buffers).  Same sums, same order.  Instantiated for <3, 8, H> only.
constexpr int LIM_MAX = 15 * 15 * 15;      // largest intermediate: Ns^3 at N = 8

// out[.., r, ..] = sum_c M[r][c] in[.., c, ..] along `axis` of a row-major array with extents e[0..dim) (C along `axis` on input, nr on output)
template <int C>
__device__ inline void lim_apply(const double* __restrict__ M, int nr, const double* in, double* out, int dim, const int* e, int axis) {
    unsigned inner = 1, outer = 1;
    for (int a = axis + 1; a < dim; a++) inner *= e[a];
    for (int a = 0; a < axis; a++) outer *= e[a];
    const unsigned total = outer * nr * inner;
    for (unsigned t = threadIdx.x; t < total; t += blockDim.x) {
        const unsigned q = t / inner, in_i = t - q * inner;
        const unsigned o = q / (unsigned)nr, r = q - o * nr;
        const double* mr = M + r * C;
        const double* ip = in + (o * C) * inner + in_i;
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < C; c++) acc += mr[c] * ip[c * inner];
        out[t] = acc;
    }
}

template <int DIM, int N, int H>
__global__ void __launch_bounds__(256)
limiter_reconstruct_kernel(int nv, const double* __restrict__ patch, const long* __restrict__ cells, double* __restrict__ u,
                           const double* __restrict__ R) {
    __shared__ double A[LIM_MAX], B[LIM_MAX];
    constexpr int Ns = 2 * N - 1;
    const long cell = cells[blockIdx.x];
    if (cell < 0) return;                                          // empty slot
    const int S = Ns + 2 * H;
    long NN = 1, SS = 1, NsD = 1;
    for (int a = 0; a < DIM; a++) { NN *= N; SS *= S; NsD *= Ns; }
    const double* pt = patch + (long)blockIdx.x * SS * nv;
    for (int v = 0; v < nv; v++) {
        for (int t = threadIdx.x; t < NsD; t += blockDim.x) {
            int r = t;
            long flat = 0, mul = 1;
            for (int a = DIM - 1; a >= 0; a--) { flat += (long)(r % Ns + H) * mul; mul *= S; r /= Ns; }
            A[t] = pt[flat * nv + v];
        }
        __syncthreads();
        int e[3] = {Ns, Ns, Ns};
        double *src = A, *dst = B;
        for (int a = 0; a < DIM; a++) {
            lim_apply<Ns>(R, N, src, dst, DIM, e, a);
            e[a] = N;
            __syncthreads();
            double* tmp = src; src = dst; dst = tmp;
        }
        for (int t = threadIdx.x; t < NN; t += blockDim.x) u[(cell * NN + t) * nv + v] = src[t];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Patches with halo 2 for the second-order patch update (EXA_FV_MUSCL_HANCOCK).  The patch [(N_s+4)^DIM][nv] is the
// window of the ghost-extended global subcell array (the projected block, extended by two layers axis by axis, in axis order, over the
// full transverse range -- solvers.fill_halos_boundary):
//   interior                        (P x .. x P) u of the cell
//   face halos, two layers          the two adjacent subcell layers of the face neighbour's projection (normal axis first, two rows of P)
//   edge entries at depth (1, 1)    from the diagonal cell c +- e_a +- e_b: both normal axes first, one row of P each (4 points in 2-D,
//                                   12 lines in 3-D; one cell load and O(N^2 nv) FMAs each)
//   everything else in the halo     nearest interior value (depth 2 x halo, 3-D corners: never read by the update)
// Domain faces: kind[a*2+side] (FV_FACE_*) and data[a*2+side][nv].  Across a MIRROR face the source cell stays, the subcell rows along
// that axis come in mirrored order (lim_apply_v's row step -1) and the value is multiplied by the face's signs; across a STATE face the
// value is the face's state.  The rules of two axes compose in axis order, the later axis last: STATE on the later axis wins, a mirror
// on the later axis multiplies what the earlier axis gave (its state included).
// The rounds over the variables are those of the kernels above.  LDS: the two buffers of LimBuf -- two normal rows instead of one only enlarge the small intermediates (2 N^2 <= N_s N^2).
// ------------------------------------------------------------------------------------------------------------------
struct LimFaces {
    int kind[6];
    const double* data;
};

template <int DIM, int N, int NV, bool ONE>
__global__ void __launch_bounds__((LimBuf<DIM, N>::NT))
limiter_project_halo2_kernel(int nv, long nc0, long nc1, long nc2, const double* __restrict__ u, const long* __restrict__ cells,
                             double* __restrict__ patch, const double* __restrict__ P_global, LimFaces fk) {
    extern __shared__ __attribute__((aligned(16))) double lim_sm[];
    const int nvs = ONE ? NV : nv;                                 // ONE: nv == NV, one round, the stride a compile-time value
    using LB = LimBuf<DIM, N>;
    constexpr int Ns = LB::Ns, S = Ns + 4, NN = LB::NN;
    constexpr int SS = DIM == 3 ? S * S * S : S * S, LAYER = DIM == 3 ? Ns * Ns : Ns;
    double* X = lim_sm;
    double* Y = lim_sm + (size_t)LB::B1 * NV;
    __shared__ double Psh[Ns * N];
    const long cell = cells[blockIdx.x];
    if (cell < 0) return;                                          // empty slot of a capacity-sized cell list
    for (int t = threadIdx.x; t < Ns * N; t += blockDim.x) Psh[t] = P_global[t];
    const double* P = Psh;                                         // (visible after the barrier behind the first load of u)
    double* pt = patch + (long)blockIdx.x * SS * nvs;
    const long nc[3] = {nc0, nc1, nc2};
    long cc[3];
    { long b = cell; cc[2] = DIM == 3 ? b % nc2 : 0; if (DIM == 3) b /= nc2; cc[1] = b % nc1; cc[0] = b / nc1; }
    auto fromX = [&](unsigned i, int v) { return X[i * NV + v]; };
    auto fromY = [&](unsigned i, int v) { return Y[i * NV + v]; };
    auto toX = [&](unsigned t, const double (&a)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; v++) X[t * NV + v] = a[v];
    };
    auto toY = [&](unsigned t, const double (&a)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; v++) Y[t * NV + v] = a[v];
    };
    // what lies across face (a, side) of THIS cell: the face's kind at the domain face, the periodic wrap / the neighbour cell elsewhere
    auto kind_of = [&](int a, int side) { return cc[a] == (side ? nc[a] - 1 : 0) ? fk.kind[a * 2 + side] : FV_FACE_PERIODIC; };
    for (int v0 = 0; v0 < nvs; v0 += NV) {
        auto load_cell = [&](long c) {                             // X <- the NV variables of cell c (NV == nv: one contiguous run)
            __syncthreads();                                       // X and Y are free (the previous product has written its result)
            for (int t = threadIdx.x; t < NN * NV; t += blockDim.x) X[t] = u[(c * NN + t / NV) * nvs + v0 + t % NV];
            __syncthreads();
        };
        // ---- own projection: u -> X -> Y (-> X) -> patch interior
        load_cell(cell);
        {
            int e[3] = {N, N, N};
            lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, 0, fromX, toY);
            e[0] = Ns;
            __syncthreads();
            auto to_patch = [&](unsigned t, const double (&a)[NV]) {
                unsigned r = t;
                long flat = 0, mul = 1;
#pragma unroll
                for (int ax = DIM - 1; ax >= 0; ax--) { flat += (long)(r % Ns + 2) * mul; mul *= S; r /= Ns; }
#pragma unroll
                for (int v = 0; v < NV; v++) pt[flat * nvs + v0 + v] = a[v];
            };
            if constexpr (DIM == 3) {
                lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, 1, fromY, toX);
                e[1] = Ns;
                __syncthreads();
                lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, 2, fromX, to_patch);
            } else {
                lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e, 1, fromY, to_patch);
            }
        }
        __syncthreads();                                           // the interior is in global memory, visible to the workgroup
        // halo entries the update never reads (a second layer together with another halo coordinate, 3-D corners): nearest interior value
        for (int t = threadIdx.x; t < SS; t += blockDim.x) {
            int I[3] = {0, 0, 0}, r = t, nh = 0, deep = 0;
            for (int a = DIM - 1; a >= 0; a--) {
                I[a] = r % S;
                r /= S;
                nh += (I[a] < 2 || I[a] > Ns + 1) ? 1 : 0;
                deep += (I[a] == 0 || I[a] == S - 1) ? 1 : 0;
            }
            if (nh < 2 || (nh == 2 && deep == 0)) continue;        // interior, face halos, edge entries: written elsewhere
            long flat = 0;
            for (int a = 0; a < DIM; a++) {
                const int ci = I[a] < 2 ? 2 : (I[a] > Ns + 1 ? Ns + 1 : I[a]);
                flat = flat * S + ci;
            }
#pragma unroll
            for (int v = 0; v < NV; v++) pt[(long)t * nvs + v0 + v] = pt[flat * nvs + v0 + v];
        }
        // ---- face halos: two layers
        for (int a = 0; a < DIM; a++)
            for (int side = 0; side < 2; side++) {
                const int f = a * 2 + side, kind = kind_of(a, side);
                const double* fd = fk.data ? fk.data + (long)f * nvs + v0 : nullptr;
                const bool mirror = kind == FV_FACE_MIRROR;
                // t enumerates (axis 0, .., axis DIM-1) lexicographically with extent 2 along a: layer i of the halo, outwards at the high side
                auto to_layers = [&](unsigned t, const double (&acc)[NV]) {
                    unsigned r = t;
                    int idx[3] = {0, 0, 0};
                    for (int b = DIM - 1; b >= 0; b--) {
                        const unsigned ext = b == a ? 2 : Ns;
                        const int i = r % ext;
                        r /= ext;
                        idx[b] = b == a ? (side ? Ns + 2 + i : i) : i + 2;
                    }
                    long flat = 0;
                    for (int b = 0; b < DIM; b++) flat = flat * S + idx[b];
#pragma unroll
                    for (int v = 0; v < NV; v++) pt[flat * nvs + v0 + v] = mirror ? acc[v] * fd[v] : acc[v];
                };
                if (kind == FV_FACE_STATE) {
                    for (int t = threadIdx.x; t < 2 * LAYER; t += blockDim.x) {
                        double acc[NV];
#pragma unroll
                        for (int v = 0; v < NV; v++) acc[v] = fd[v];
                        to_layers(t, acc);
                    }
                    continue;
                }
                long nb[3] = {cc[0], cc[1], cc[2]};
                if (!mirror) nb[a] = (nb[a] + (side ? 1 : nc[a] - 1)) % nc[a];
                load_cell((nb[0] * nc1 + nb[1]) * (DIM == 3 ? nc2 : 1) + nb[2]);
                // rows of the source along a for the layers i = 0, 1: wrap low Ns-2, Ns-1; wrap high 0, 1; mirror low 1, 0; mirror high Ns-1, Ns-2
                const int r0 = mirror ? (side ? Ns - 1 : 1) : (side ? 0 : Ns - 2), rstep = mirror ? -1 : 1;
                int e2[3] = {N, N, N};
                const int b0 = a, b1 = (a + 1) % DIM, b2 = (a + 2) % DIM;
                lim_apply_v<N, NV>(P, N, r0, 2, DIM, e2, b0, fromX, toY, rstep);              // normal axis first: the two adjacent layers only
                e2[b0] = 2;
                __syncthreads();
                if constexpr (DIM == 3) {
                    lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e2, b1, fromY, toX);
                    e2[b1] = Ns;
                    __syncthreads();
                    lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e2, b2, fromX, to_layers);
                } else {
                    lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e2, b1, fromY, to_layers);
                }
            }
        // ---- edge entries: first halo layer along a and b (a < b), the whole line along the third axis
        for (int a = 0; a < DIM; a++)
            for (int b = a + 1; b < DIM; b++)
                for (int sides = 0; sides < 4; sides++) {
                    const int sa = sides >> 1, sb = sides & 1;
                    const int ka = kind_of(a, sa), kb = kind_of(b, sb);
                    const double* da = fk.data ? fk.data + (long)(a * 2 + sa) * nvs + v0 : nullptr;
                    const double* db = fk.data ? fk.data + (long)(b * 2 + sb) * nvs + v0 : nullptr;
                    const int c3 = DIM == 3 ? 3 - a - b : -1;      // the axis the line runs along
                    auto to_line = [&](unsigned t, const double (&acc)[NV]) {
                        int idx[3] = {0, 0, 0};
                        idx[a] = sa ? Ns + 2 : 1;
                        idx[b] = sb ? Ns + 2 : 1;
                        if (DIM == 3) idx[c3] = (int)t + 2;
                        long flat = 0;
                        for (int x = 0; x < DIM; x++) flat = flat * S + idx[x];
#pragma unroll
                        for (int v = 0; v < NV; v++) pt[flat * nvs + v0 + v] = acc[v];
                    };
                    if (kb == FV_FACE_STATE || ka == FV_FACE_STATE) {
                        // the later axis is applied last: its state wins; its mirror multiplies the earlier axis's state
                        for (int t = threadIdx.x; t < (DIM == 3 ? Ns : 1); t += blockDim.x) {
                            double acc[NV];
#pragma unroll
                            for (int v = 0; v < NV; v++) acc[v] = kb == FV_FACE_STATE ? db[v] : (kb == FV_FACE_MIRROR ? da[v] * db[v] : da[v]);
                            to_line(t, acc);
                        }
                        continue;
                    }
                    long nb[3] = {cc[0], cc[1], cc[2]};
                    if (ka == FV_FACE_PERIODIC) nb[a] = (nb[a] + (sa ? 1 : nc[a] - 1)) % nc[a];
                    if (kb == FV_FACE_PERIODIC) nb[b] = (nb[b] + (sb ? 1 : nc[b] - 1)) % nc[b];
                    load_cell((nb[0] * nc1 + nb[1]) * (DIM == 3 ? nc2 : 1) + nb[2]);
                    // the one row next to the face: the neighbour's nearest (wrap) or the cell's own nearest (mirror)
                    const int ra = (ka == FV_FACE_MIRROR) == (sa == 1) ? Ns - 1 : 0;
                    const int rb = (kb == FV_FACE_MIRROR) == (sb == 1) ? Ns - 1 : 0;
                    auto to_line_signed = [&](unsigned t, const double (&acc)[NV]) {
                        double sg[NV];
#pragma unroll
                        for (int v = 0; v < NV; v++) {
                            sg[v] = acc[v];
                            if (ka == FV_FACE_MIRROR) sg[v] *= da[v];
                            if (kb == FV_FACE_MIRROR) sg[v] *= db[v];
                        }
                        to_line(t, sg);
                    };
                    int e2[3] = {N, N, N};
                    lim_apply_v<N, NV>(P, N, ra, 1, DIM, e2, a, fromX, toY);
                    e2[a] = 1;
                    __syncthreads();
                    if constexpr (DIM == 3) {
                        lim_apply_v<N, NV>(P, N, rb, 1, DIM, e2, b, fromY, toX);
                        e2[b] = 1;
                        __syncthreads();
                        lim_apply_v<N, NV>(P, N, 0, Ns, DIM, e2, c3, fromX, to_line_signed);
                    } else {
                        lim_apply_v<N, NV>(P, N, rb, 1, DIM, e2, b, fromY, to_line_signed);
                    }
                }
    }
}

// A kernel family, as lim_launch takes it: the instantiation for (DIM, N, NV), its workgroup size, its LDS elements per variable
struct LimProjectHalo1 {
    template <int DIM, int N, int NV, bool ONE> static auto kernel() { return limiter_project_halo1_kernel<DIM, N, NV, ONE>; }
    template <int DIM, int N, int NV> static constexpr int threads = NV == 1 ? LimBuf<DIM, N>::NT1 : LimBuf<DIM, N>::NT;
    template <int DIM, int N> static constexpr int lds = LimBuf<DIM, N>::B1 + LimBuf<DIM, N>::B2;
};
struct LimProjectHalo2 {
    template <int DIM, int N, int NV, bool ONE> static auto kernel() { return limiter_project_halo2_kernel<DIM, N, NV, ONE>; }
    template <int DIM, int N, int NV> static constexpr int threads = LimBuf<DIM, N>::NT;
    template <int DIM, int N> static constexpr int lds = LimBuf<DIM, N>::B1 + LimBuf<DIM, N>::B2;
};
struct LimFaceLayers {
    template <int DIM, int N, int NV, bool ONE> static auto kernel() { return limiter_face_layers_kernel<DIM, N, NV, ONE>; }
    template <int DIM, int N, int NV> static constexpr int threads = LimBuf<DIM, N>::NT1;
    template <int DIM, int N> static constexpr int lds = LimBuf<DIM, N>::F1 + LimBuf<DIM, N>::F2;
};
template <int H> struct LimReconstruct {
    template <int DIM, int N, int NV, bool ONE> static auto kernel() { return limiter_reconstruct_halo_kernel<DIM, N, NV, ONE, H>; }
    template <int DIM, int N, int NV> static constexpr int threads = LimBuf<DIM, N>::NT_R;
    template <int DIM, int N> static constexpr int lds = LimBuf<DIM, N>::B1 + LimBuf<DIM, N>::B2;
};

// EXA_LIM_PER_VARIABLE=1 in the environment: NV = 1 rounds even where five divides nv, so that one process can compare the two
// instantiations (tests/test_limiter.py).  Read at every call: it is a test switch.
static bool lim_per_variable() {
    const char* e = getenv("EXA_LIM_PER_VARIABLE");
    return e && e[0] == '1';
}

// n workgroups of family F's kernel for (DIM, N): five variables at a time if `five` and the LDS holds them, else one at a time;
// the instantiation with a compile-time stride where that is all of them (nv == NV).  The <.., 5, false> instantiations (nv = 10, 15, ..)
// are unexercised: no built-in or generated term set has such a count and no test launches them (the NV = 1 multi-round text with another NV)
template <class F, int DIM, int N, class... Args>
static int lim_launch_at(const char* who, bool five, int nv, long n, hipStream_t s, Args... args) {
    constexpr size_t per_variable = sizeof(double) * F::template lds<DIM, N>;
    five = five && 5 * per_variable + 2048 <= 160 * 1024;          // (+ the operator copy and alignment)
    const bool one = nv == (five ? 5 : 1);
    auto kern = five ? (one ? F::template kernel<DIM, N, 5, true>() : F::template kernel<DIM, N, 5, false>())
                     : (one ? F::template kernel<DIM, N, 1, true>() : F::template kernel<DIM, N, 1, false>());
    const size_t bytes = per_variable * (five ? 5 : 1);
    static bool attr_dev[4][64] = {};                              // [instantiation][device], per (F, DIM, N)
    bool* attr = attr_dev[2 * five + one];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 ||
        (!attr[dev] && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)) {
        set_error("%s: the kernel's LDS attribute could not be set", who);
        return -2;
    }
    attr[dev] = true;
    hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(five ? F::template threads<DIM, N, 5> : F::template threads<DIM, N, 1>), bytes, s, nv, args...);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s launch: %s", who, hipGetErrorString(e)); return -2; }
    return 0;
}

// The one way to a kernel of this file.  NV = 5 where five divides nv, the LDS fits and the test switch is off, else NV = 1.
// args: the kernel's arguments after the leading nv
template <class F, class... Args>
static int lim_launch(const char* who, int dim, int N, int nv, long n, hipStream_t s, Args... args) {
    const bool five = nv % 5 == 0 && !lim_per_variable();
    switch (N) {
#define X(NN_)                                                                                                                         \
    case NN_:                                                                                                                          \
        return dim == 2 ? lim_launch_at<F, 2, NN_>(who, five, nv, n, s, args...) : lim_launch_at<F, 3, NN_>(who, five, nv, n, s, args...);
        EXA_LIM_CASES(X)
#undef X
    default: set_error("limiter: N = %d is not built", N); return -1;
    }
}

int limiter_project(int dim, int N, int Ns, int nv, const long* nc, const double* u, const long* cells, long n, double* patch,
                    const double* Pdev, const LimGhosts* ghosts, hipStream_t s) {
    if (n <= 0) return 0;
    LimGhosts gh{};
    if (ghosts) gh = *ghosts;
    return lim_launch<LimProjectHalo1>("limiter_project", dim, N, nv, n, s, nc[0], nc[1], dim == 3 ? nc[2] : 1L, u, cells, patch, Pdev, gh);
}

int limiter_face_layers(int dim, int N, int Ns, int nv, const long* nc, const double* u, int a, int side, const double* need,
                        double* out, const double* Pdev, hipStream_t s) {
    long nt = 1;
    for (int b = 0; b < dim; b++)
        if (b != a) nt *= nc[b];
    if (nt <= 0) return 0;
    return lim_launch<LimFaceLayers>("limiter_face_layers", dim, N, nv, nt, s, nc[0], nc[1], dim == 3 ? nc[2] : 1L, u, a, side, need, out, Pdev);
}

// halo: the halo layers of the patches, 1 | 2
int limiter_reconstruct(int dim, int N, int Ns, int nv, const double* patch, const long* cells, long n, double* u,
                        const double* Rdev, int halo, hipStream_t s) {
    if (n <= 0) return 0;
    if (dim == 3 && N == 8 && nv > 1 && nv % 5 != 0) {             // NOT MERGED: see limiter_reconstruct_kernel
        if (halo == 2) hipLaunchKernelGGL((limiter_reconstruct_kernel<3, 8, 2>), dim3((unsigned)n), dim3(256), 0, s, nv, patch, cells, u, Rdev);
        else hipLaunchKernelGGL((limiter_reconstruct_kernel<3, 8, 1>), dim3((unsigned)n), dim3(256), 0, s, nv, patch, cells, u, Rdev);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { set_error("limiter_reconstruct launch: %s", hipGetErrorString(e)); return -2; }
        return 0;
    }
    return halo == 2 ? lim_launch<LimReconstruct<2>>("limiter_reconstruct", dim, N, nv, n, s, patch, cells, u, Rdev)
                     : lim_launch<LimReconstruct<1>>("limiter_reconstruct", dim, N, nv, n, s, patch, cells, u, Rdev);
}

// kinds: FV_FACE_* of the 2 dim domain faces (null: all periodic); data: device, [2 dim][nv] (signs of a mirror face, state of a state face)
int limiter_project_halo2(int dim, int N, int nv, const long* nc, const double* u, const long* cells, long n, double* patch,
                          const double* Pdev, const int* kinds, const double* data, hipStream_t s) {
    if (n <= 0) return 0;
    LimFaces fk{};
    for (int f = 0; f < 6; f++) fk.kind[f] = (kinds && f < 2 * dim) ? kinds[f] : FV_FACE_PERIODIC;
    fk.data = data;
    return lim_launch<LimProjectHalo2>("limiter_project_halo2", dim, N, nv, n, s, nc[0], nc[1], dim == 3 ? nc[2] : 1L, u, cells, patch, Pdev, fk);
}


// ------------------------------------------------------------------------------------------------------------------
// A-posteriori (MOOD) detection: the kernels live in exa_lim_detect.hpp, parameterised by a criterion type.  Here: the built-in
// criterion -- Euler layout with a run-time variable count (five variables: compile-time), bounds[cell][4] = min rho, max rho, min E, max E.
// Generated term sets that carry their own criterion instantiate the same kernels in their side library (lim_user.hip).
// ------------------------------------------------------------------------------------------------------------------
int limiter_snapshot(int dim, int N, int nv, long ncells, const double* u, double* u_old, double* bounds, hipStream_t s) {
    return nv == 5 ? lim_snapshot_launch<LimEulerCrit<5>>(dim, N, nv, ncells, u, u_old, bounds, s)
                   : lim_snapshot_launch<LimEulerCrit<0>>(dim, N, nv, ncells, u, u_old, bounds, s);
}

int limiter_detect(int dim, int N, int nv, const long* nc, const double* u, const double* bounds, const LimGhosts* ghosts, const int* kinds,
                   double d0, double eps, double floor, unsigned char* mask, hipStream_t s) {
    return nv == 5 ? lim_detect_launch<LimEulerCrit<5>>(dim, N, nv, nc, u, bounds, ghosts, kinds, d0, eps, floor, mask, s)
                   : lim_detect_launch<LimEulerCrit<0>>(dim, N, nv, nc, u, bounds, ghosts, kinds, d0, eps, floor, mask, s);
}


// ------------------------------------------------------------------------------------------------------------------
// Conservative DG / FV interface: the kernels live in exa_lim_conserve.hpp, templates over the term set.  Here: the
// built-in Euler (5 variables) and advection (1 variable) sets; EulerRef2D has none.  A generated term set that asks for the interface
// instantiates them in its side library (lim_conserve_user.hip).
// ------------------------------------------------------------------------------------------------------------------
void limiter_fill_builtin(PdeKernels* tab) {
    lim_conserve_fill<Euler>(&tab[1]);
    lim_conserve_fill<Advection<1>>(&tab[2]);
}

}  // namespace exa

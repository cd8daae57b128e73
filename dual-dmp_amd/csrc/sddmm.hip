// Per-entry gradient of the aggregation (SDDMM over the CSR):  G[e] = sum_c dY[row e, c] * H[col e, c]
//
// dL/dA of Y = A H for every stored entry of A: what the edge_weight gradient of GCNConv starts from.  A gather
// with the SpMM's access pattern and the SpMM's work layout (spmm_lean.inc):
//   * a workgroup (4 waves) owns a chunk of 64 consecutive rows; blockIdx -> chunk is XCD-aware like the gather's, so the ~deg
//     re-reads of a neighbour row by neighbouring output rows hit that XCD's L2;
//   * 8 lanes x float4 cover one 128-byte slab of a row, 8 rows per wave step, two steps per chunk;
//   * a row's entries are taken 8 at a time: their 8 neighbour-row addresses are formed once, then the lane walks the C / 32 slabs
//     with one accumulator per entry -- per slab ONE 16-byte load of the row's own dY slab, reused for all entries of the batch, and
//     up to 8 independent 16-byte neighbour loads in flight.  Mesh rows (4 and ~7 entries) are one batch: dY is read exactly once;
//   * the 8 lanes' partial sums are combined by a fixed xor tree (1, 2, 4), lane k of the group stores entry k: one coalesced
//     32-byte store per row and batch.  No atomics, no LDS, no barrier: float32 products and sums in a fixed order, bitwise
//     reproducible.
// Widths that are not a multiple of 4 (or unaligned operands) take a scalar kernel with the same column order per entry.
#include "ddmp_common.h"

#include <type_traits>

namespace {

using namespace ddmp;

constexpr int kRB = 64;
constexpr int kEB = 8;             // entries per batch

__global__ __launch_bounds__(256) void sddmm_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                    const float* __restrict__ dY, int64_t lddy, const float* __restrict__ H, int64_t ldh,
                                                    float* __restrict__ G, int n_rows, int C, int chunks_per_xcd, int n_chunks) {
    const int chunk = (blockIdx.x & (kXcd - 1)) * chunks_per_xcd + (blockIdx.x >> 3);
    if (chunk >= n_chunks) return;
    const int r0 = chunk * kRB;
    const int nr = min(kRB, n_rows - r0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> 3, sl = lane & 7;
#pragma unroll 1
    for (int qq = 0; qq < 2; ++qq) {
        const int lr = wave * 8 + grp + qq * 32;
        if (lr >= nr) continue;                                  // (the 8 lanes of a row group leave together)
        const int row = r0 + lr;
        const int rbase = rowptr[row];
        const int nn = rowptr[row + 1] - rbase;
        const float* yp = dY + (int64_t)row * lddy + sl * 4;
#pragma unroll 1
        for (int b0 = 0; b0 < nn; b0 += kEB) {
            // Entry slots this wave step uses: the LONGEST row's count (wave-uniform, from ballots).  The batch is compiled per
            // count with unconditional loads: a per-lane predicate on a load puts a branch and a full wait behind every one of
            // them, and the loads of a batch must be in flight together.  A lane whose row is shorter re-reads its last entry (an
            // L1 hit; that sum is not stored).  Regular meshes: the face graph runs the 4-slot body, the vertex graph the 7-slot one.
            int ne_w = 0;
#pragma unroll
            for (int k = 0; k < kEB; ++k) ne_w += __any(b0 + k < nn) ? 1 : 0;
            auto batch = [&](auto ne_tag) {
                constexpr int NE = decltype(ne_tag)::value;
                const float* hp[NE];
                float acc[NE];
#pragma unroll
                for (int k = 0; k < NE; ++k) {
                    const int c = col[rbase + min(b0 + k, nn - 1)];
                    hp[k] = H + (int64_t)c * ldh + sl * 4;
                    acc[k] = 0.f;
                }
                for (int c0 = 0; c0 + sl * 4 < C; c0 += 32) {
                    const float4 y = *reinterpret_cast<const float4*>(yp + c0);
                    float4 h[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) h[k] = *reinterpret_cast<const float4*>(hp[k] + c0);
#pragma unroll
                    for (int k = 0; k < NE; ++k)
                        acc[k] = fmaf(y.w, h[k].w, fmaf(y.z, h[k].z, fmaf(y.y, h[k].y, fmaf(y.x, h[k].x, acc[k]))));
                }
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < NE; ++k) {
                    float t = acc[k];
                    t += __shfl_xor(t, 1, 64);
                    t += __shfl_xor(t, 2, 64);
                    t += __shfl_xor(t, 4, 64);
                    v = sl == k ? t : v;
                }
                if (b0 + sl < nn) G[rbase + b0 + sl] = v;
            };
            switch (ne_w) {
                case 1: batch(std::integral_constant<int, 1>()); break;
                case 2: batch(std::integral_constant<int, 2>()); break;
                case 3: batch(std::integral_constant<int, 3>()); break;
                case 4: batch(std::integral_constant<int, 4>()); break;
                case 5: batch(std::integral_constant<int, 5>()); break;
                case 6: batch(std::integral_constant<int, 6>()); break;
                case 7: batch(std::integral_constant<int, 7>()); break;
                default: batch(std::integral_constant<int, 8>()); break;
            }
        }
    }
}

// any width / alignment: one thread per row, the entry's columns in ascending order
__global__ __launch_bounds__(256) void sddmm_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const float* __restrict__ dY, int64_t lddy, const float* __restrict__ H,
                                                           int64_t ldh, float* __restrict__ G, int n_rows, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const float* y = dY + (int64_t)row * lddy;
    for (int e = rowptr[row]; e < rowptr[row + 1]; ++e) {
        const float* h = H + (int64_t)col[e] * ldh;
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(y[c], h[c], acc);
        G[e] = acc;
    }
}

}  // namespace

extern "C" int ddmp_sddmm_f32(const ddmp_graph* g, const float* dY, int64_t lddy, const float* H, int64_t ldh, int C, float* G,
                              ddmp_stream stream) {
    ARG_TRY(g && dY && H && G && C > 0 && lddy >= C && ldh >= C);
    hipStream_t st = (hipStream_t)stream;
    if (g->nnz == 0) return DDMP_OK;
    const int n = (int)g->n_rows;
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (C % 4 == 0 && lddy % 4 == 0 && ldh % 4 == 0 && al16(dY) && al16(H)) {
        const int n_chunks = (int)cdiv(n, kRB);
        const int cpx = (int)cdiv(n_chunks, kXcd);
        hipLaunchKernelGGL(sddmm_kernel, dim3(cpx * kXcd), dim3(256), 0, st, g->rowptr, g->col, dY, lddy, H, ldh, G, n, C, cpx, n_chunks);
    } else {
        hipLaunchKernelGGL(sddmm_scalar_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, g->rowptr, g->col, dY, lddy, H, ldh, G, n, C);
    }
    LAUNCH_TRY();
    return DDMP_OK;
}

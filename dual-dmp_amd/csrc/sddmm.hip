// Per-entry gradient of the aggregation (SDDMM over the CSR):  G[e] = sum_c dY[row e, c] * H[col e, c]
//
// dL/dA of Y = A H for every stored entry of A: what the edge_weight gradient of GCNConv starts from.  A gather
// with the SpMM's access pattern on the row-gather layout (row_gather.h), without heads:
//   * a row's entries are taken 8 at a time: their 8 neighbour-row addresses are formed once, then the lane walks the C / 32 slabs
//     with one accumulator per entry -- per slab ONE 16-byte load of the row's own dY slab, reused for all entries of the batch, and
//     up to 8 independent 16-byte neighbour loads in flight.  Mesh rows (4 and ~7 entries) are one batch: dY is read exactly once
//     (regular meshes: the face graph runs the 4-slot body, the vertex graph the 7-slot one);
//   * the 8 lanes' partial sums are combined by the fixed xor tree (1, 2, 4), lane k of the group stores entry k: one coalesced
//     32-byte store per row and batch (the sum of a re-read last entry is not stored).  No LDS, no barrier: float32 products and
//     sums in a fixed order.
// The scalar kernel takes an entry's columns in the same ascending order.
#include "row_gather.h"

namespace {

__global__ __launch_bounds__(256) void sddmm_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                    const float* __restrict__ dY, int64_t lddy, const float* __restrict__ H, int64_t ldh,
                                                    float* __restrict__ G, int n_rows, int C, int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    FOR_CHUNK_ROW_ENTRIES {
        const float* yp = dY + (int64_t)row * lddy + sl * 4;
#pragma unroll 1
        for (int b0 = 0; b0 < nn; b0 += kEB) {
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
                    const float4 y = ld4(yp + c0);
                    float4 h[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) h[k] = ld4(hp[k] + c0);
#pragma unroll
                    for (int k = 0; k < NE; ++k) acc[k] = dot4(y, h[k], acc[k]);
                }
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < NE; ++k) {
                    const float t = red_sum(acc[k], 8);
                    v = sl == k ? t : v;
                }
                if (b0 + sl < nn) G[rbase + b0 + sl] = v;
            };
            ROW_BATCH_SWITCH(b0, nn, batch)
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
    if (g->nnz == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddy % 4 == 0 && ldh % 4 == 0 && al16(dY) && al16(H);
    return launch_rows((hipStream_t)stream, (int)g->n_rows, vec, sddmm_kernel, sddmm_scalar_kernel, g->rowptr, g->col, dY, lddy, H, ldh,
                       G, (int)g->n_rows, C);
}

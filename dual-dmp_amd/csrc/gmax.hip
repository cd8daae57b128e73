// Max aggregation with its winner (EdgeConv): the fused arg-max gather and its one-launch backward.
//
//   Y[i,c]   = A[i,c] + max_{e in row i} B[col e, c],   arg[i,c] = col e of the winning entry   (a row without entries: 0 and -1)
//   dA[j,:]  = dG[j,:] (0 for a row without entries)
//   dB[j,c]  = sum_{e' in row j} (arg[col e', c] == j ? dG[col e', c] : 0)
//
// over the COALESCED CSR of a valued graph (the graph of gat.hip / feast.hip; its values are not read: a duplicate edge cannot
// change a maximum).  The backward relies on the SYMMETRIC structure: row j's own entries enumerate the rows j feeds, and arg
// holds node ids, so no mirror map is read.  Ties go to the first entry in CSR order (the smallest source id): the running
// maximum starts at the row's first entry and is replaced on a strict > only.
// On the row-gather layout (row_gather.h) without heads: the 8 lanes of a row group walk the C / 4 float4 of the row 8 at a time.
// A shorter row's re-read last entry can neither win a strict > nor -- masked -- add to a sum.  The running maximum and its id
// (forward) and the sum (backward) stay in registers over ALL entries of the row: the 1200-entry hub row is exact like any other.
// No LDS, no barrier.
#include "row_gather.h"

namespace {

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void gather_max_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                         const float* __restrict__ B, int64_t ldb, const float* __restrict__ A,
                                                         int64_t lda, float* __restrict__ Y, int64_t ldy, int* __restrict__ arg,
                                                         int64_t ldg, int n_rows, int C, int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        float* yrow = Y + (int64_t)row * ldy;
        int* grow = arg ? arg + (int64_t)row * ldg : nullptr;
        if (nn == 0) {                                            // a row without entries: 0, not A (the edge function never ran)
            for (int q = sl; q < W; q += 8) {
                *reinterpret_cast<float4*>(yrow + q * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
                if (grow) *reinterpret_cast<int4*>(grow + q * 4) = make_int4(-1, -1, -1, -1);
            }
            continue;
        }
        const int j0 = col[rbase];
        for (int q = sl; q < W; q += 8) {
            float4 m = ld4(B + (int64_t)j0 * ldb + q * 4);
            int4 id = make_int4(j0, j0, j0, j0);
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    int j[NE];
                    float4 x[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) j[k] = col[rbase + min(b0 + k, nn - 1)];
#pragma unroll
                    for (int k = 0; k < NE; ++k) x[k] = ld4(B + (int64_t)j[k] * ldb + q * 4);
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        take_gt(m.x, id.x, x[k].x, j[k]);
                        take_gt(m.y, id.y, x[k].y, j[k]);
                        take_gt(m.z, id.z, x[k].z, j[k]);
                        take_gt(m.w, id.w, x[k].w, j[k]);
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
            if (A) {
                const float4 a = ld4(A + (int64_t)row * lda + q * 4);
                m.x = a.x + m.x, m.y = a.y + m.y, m.z = a.z + m.z, m.w = a.w + m.w;
            }
            *reinterpret_cast<float4*>(yrow + q * 4) = m;
            if (grow) *reinterpret_cast<int4*>(grow + q * 4) = id;
        }
    }
}

__global__ __launch_bounds__(256) void gather_max_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                const float* __restrict__ B, int64_t ldb,
                                                                const float* __restrict__ A, int64_t lda, float* __restrict__ Y,
                                                                int64_t ldy, int* __restrict__ arg, int64_t ldg, int n_rows,
                                                                int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* yrow = Y + (int64_t)row * ldy;
    int* grow = arg ? arg + (int64_t)row * ldg : nullptr;
    for (int c = 0; c < C; ++c) {
        float m = 0.f;
        int id = -1;
        if (e1 > e0) {
            id = col[e0];
            m = B[(int64_t)id * ldb + c];
            for (int e = e0 + 1; e < e1; ++e) {
                const int j = col[e];
                take_gt(m, id, B[(int64_t)j * ldb + c], j);
            }
            if (A) m = A[(int64_t)row * lda + c] + m;
        }
        yrow[c] = m;
        if (grow) grow[c] = id;
    }
}

// ------------------------------------------------------------------------------------------------ backward
__global__ __launch_bounds__(256) void gather_max_bwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ dG, int64_t lddg,
                                                             const int* __restrict__ arg, int64_t ldg, float* __restrict__ dA,
                                                             int64_t ldda, float* __restrict__ dB, int64_t lddb, int n_rows, int C,
                                                             int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        float* arow = dA + (int64_t)row * ldda;
        float* brow = dB + (int64_t)row * lddb;
        if (nn == 0) {
            for (int q = sl; q < W; q += 8) {
                *reinterpret_cast<float4*>(arow + q * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(brow + q * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            continue;
        }
        for (int q = sl; q < W; q += 8) {
            *reinterpret_cast<float4*>(arow + q * 4) = ld4(dG + (int64_t)row * lddg + q * 4);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    int64_t j[NE];
                    int4 w[NE];
                    float4 x[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) j[k] = col[rbase + min(b0 + k, nn - 1)];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        w[k] = ld4i(arg + j[k] * ldg + q * 4);
                        x[k] = ld4(dG + j[k] * lddg + q * 4);
                    }
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int me = b0 + k < nn ? row : -2;            // (a re-read last entry adds nothing; arg >= -1)
                        acc.x += w[k].x == me ? x[k].x : 0.f;
                        acc.y += w[k].y == me ? x[k].y : 0.f;
                        acc.z += w[k].z == me ? x[k].z : 0.f;
                        acc.w += w[k].w == me ? x[k].w : 0.f;
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
            *reinterpret_cast<float4*>(brow + q * 4) = acc;
        }
    }
}

__global__ __launch_bounds__(256) void gather_max_bwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const float* __restrict__ dG, int64_t lddg,
                                                                    const int* __restrict__ arg, int64_t ldg,
                                                                    float* __restrict__ dA, int64_t ldda, float* __restrict__ dB,
                                                                    int64_t lddb, int n_rows, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int c = 0; c < C; ++c) {
        float acc = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int64_t j = col[e];
            acc += arg[j * ldg + c] == row ? dG[j * lddg + c] : 0.f;
        }
        dA[(int64_t)row * ldda + c] = e1 > e0 ? dG[(int64_t)row * lddg + c] : 0.f;
        dB[(int64_t)row * lddb + c] = acc;
    }
}

}  // namespace

extern "C" int ddmp_gather_max_f32(const ddmp_graph* g, const float* B, int64_t ldb, const float* A, int64_t lda, int C, float* Y,
                                   int64_t ldy, int32_t* arg, int64_t ldarg, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g, false) && B && Y && C >= 1 && ldb >= C && ldy >= C && (!A || lda >= C) && (!arg || ldarg >= C) && Y != B &&
            Y != A);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && ldb % 4 == 0 && ldy % 4 == 0 && al16(B) && al16(Y) && (!A || (lda % 4 == 0 && al16(A))) && (!arg
                     || (ldarg % 4 == 0 && al16(arg)));
    return launch_rows((hipStream_t)stream, (int)g->n_rows, vec, gather_max_kernel, gather_max_scalar_kernel, g->rowptr, g->col, B,
                       ldb, A, lda, Y, ldy, arg, ldarg, (int)g->n_rows, C);
}

extern "C" int ddmp_gather_max_bwd_f32(const ddmp_graph* g, const float* dG, int64_t lddg, const int32_t* arg, int64_t ldarg, int C,
                                       float* dA, int64_t ldda, float* dB, int64_t lddb, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g, false) && dG && arg && dA && dB && C >= 1 && lddg >= C && ldarg >= C && ldda >= C && lddb >= C && dA != dG &&
            dB != dG && dA != dB);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddg % 4 == 0 && ldarg % 4 == 0 && ldda % 4 == 0 && lddb % 4 == 0 && al16(dG) && al16(arg) &&
                     al16(dA) && al16(dB);
    return launch_rows((hipStream_t)stream, (int)g->n_rows, vec, gather_max_bwd_kernel, gather_max_bwd_scalar_kernel, g->rowptr,
                       g->col, dG, lddg, arg, ldarg, dA, ldda, dB, lddb, (int)g->n_rows, C);
}

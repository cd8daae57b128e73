// Graph attention (GATConv): scores, fused edge-softmax + gather, and the two backward launches.
//
//   z_e = leaky_relu(s_src[col e, h] + s_dst[row e, h]),  alpha_e = a_e exp(z_e - max) / sum_row a_e exp(z_e - max),
//   Y[i,h,:] = sum_{e in row i} alpha_e Hf[col e, h, :]
//
// over the COALESCED CSR of a valued graph left at all-ones values: a_e is the multiplicity of the entry, so the a_e exp(..) terms
// are the softmax over the multiset of edges.  On the row-gather layout with head passes (row_gather.h); its own part:
//   * the per-(row, head) reductions (max, denominator, delta, ds_dst, ds_src, the dot products) are strided over the head's lanes;
//     a shorter row's re-read last entry enters with factor 0;
//   * a row longer than one batch accumulates through its own output row (same lane, same address, program order): the
//     1200-entry hub row is exact like any other.
// No LDS, no barrier.
#include "colsum_final.h"

namespace {

constexpr int kDR = 256;           // rows per partial of the attention-vector gradient

__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.f ? x : slope * x; }

// ------------------------------------------------------------------------------------------------ scores
__global__ __launch_bounds__(256) void gat_scores_kernel(const float* __restrict__ Hf, int64_t ldh, int n_rows, int heads, int C,
                                                         const float* __restrict__ att_src, const float* __restrict__ att_dst,
                                                         float* __restrict__ s_src, float* __restrict__ s_dst, int lw,
                                                         int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROWS {
        const float* hrow = Hf + (int64_t)row * ldh;
        FOR_HEAD_PASSES(heads) {
            float as = 0.f, ad = 0.f;
            for (int q = q0; q < W; q += lw) {
                const float4 x = ld4(hrow + hh * C + q * 4);
                as = dot4(x, ld4(att_src + hh * C + q * 4), as);
                ad = dot4(x, ld4(att_dst + hh * C + q * 4), ad);
            }
            as = red_sum(as, lw);
            ad = red_sum(ad, lw);
            if (hv && q0 == 0) {
                s_src[(int64_t)row * heads + h] = as;
                s_dst[(int64_t)row * heads + h] = ad;
            }
        }
    }
}

__global__ __launch_bounds__(256) void gat_scores_scalar_kernel(const float* __restrict__ Hf, int64_t ldh, int n_rows, int heads,
                                                                int C, const float* __restrict__ att_src,
                                                                const float* __restrict__ att_dst, float* __restrict__ s_src,
                                                                float* __restrict__ s_dst) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const float* hrow = Hf + (int64_t)row * ldh;
    for (int h = 0; h < heads; ++h) {
        float as = 0.f, ad = 0.f;
        for (int c = 0; c < C; ++c) {
            const float x = hrow[h * C + c];
            as = fmaf(x, att_src[h * C + c], as);
            ad = fmaf(x, att_dst[h * C + c], ad);
        }
        s_src[(int64_t)row * heads + h] = as;
        s_dst[(int64_t)row * heads + h] = ad;
    }
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void gat_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                      const float* __restrict__ mult, const float* __restrict__ Hf, int64_t ldh,
                                                      const float* __restrict__ s_src, const float* __restrict__ s_dst, float slope,
                                                      const float* __restrict__ bias, float* alpha, float* Y, int64_t ldy, int n_rows,
                                                      int heads, int C, int lw, int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    FOR_CHUNK_ROW_ENTRIES {
        float* yrow = Y + (int64_t)row * ldy;
        FOR_HEAD_PASSES(heads) {
            const float sd = s_dst[(int64_t)row * heads + hh];
            // softmax of the row's entries for head hh: the head's lw lanes take the entries lw apart
            float m = -INFINITY;
            for (int e = q0; e < nn; e += lw) m = fmaxf(m, leaky(s_src[(int64_t)col[rbase + e] * heads + hh] + sd, slope));
            m = red_max(m, lw);
            float den = 0.f;
            for (int e = q0; e < nn; e += lw)
                den += mult[rbase + e] * expf(leaky(s_src[(int64_t)col[rbase + e] * heads + hh] + sd, slope) - m);
            den = red_sum(den, lw);
            const float inv = 1.f / den;                          // (nn > 0: den >= the largest entry's multiplicity >= 1)
            for (int e = q0; e < nn; e += lw) {
                const float z = leaky(s_src[(int64_t)col[rbase + e] * heads + hh] + sd, slope);
                if (hv) alpha[(int64_t)(rbase + e) * heads + h] = mult[rbase + e] * expf(z - m) * inv;
            }
            // the gather reads the factors its sibling lanes wrote: same wave, same CU's L1 -- a workgroup-scope fence
            __threadfence_block();
            gather_pass<false>(col, nullptr, alpha, Hf, ldh, yrow, rbase, nn, heads, C, hh, hv, q0, lw, [&](int q) {
                return bias ? ld4(bias + hh * C + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            });
        }
    }
}

__global__ __launch_bounds__(256) void gat_fwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ mult, const float* __restrict__ Hf,
                                                             int64_t ldh, const float* __restrict__ s_src,
                                                             const float* __restrict__ s_dst, float slope,
                                                             const float* __restrict__ bias, float* alpha, float* __restrict__ Y,
                                                             int64_t ldy, int n_rows, int heads, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* yrow = Y + (int64_t)row * ldy;
    for (int h = 0; h < heads; ++h) {
        const float sd = s_dst[(int64_t)row * heads + h];
        float m = -INFINITY;
        for (int e = e0; e < e1; ++e) m = fmaxf(m, leaky(s_src[(int64_t)col[e] * heads + h] + sd, slope));
        float den = 0.f;
        for (int e = e0; e < e1; ++e) den += mult[e] * expf(leaky(s_src[(int64_t)col[e] * heads + h] + sd, slope) - m);
        const float inv = 1.f / den;
        for (int e = e0; e < e1; ++e)
            alpha[(int64_t)e * heads + h] = mult[e] * expf(leaky(s_src[(int64_t)col[e] * heads + h] + sd, slope) - m) * inv;
        for (int c = 0; c < C; ++c) {
            float acc = bias ? bias[h * C + c] : 0.f;
            for (int e = e0; e < e1; ++e) acc = fmaf(alpha[(int64_t)e * heads + h], Hf[(int64_t)col[e] * ldh + h * C + c], acc);
            yrow[h * C + c] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, edge side
__global__ __launch_bounds__(256) void gat_bwd_edge_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const float* __restrict__ dOut, int64_t lddo,
                                                           const float* __restrict__ Hf, int64_t ldh,
                                                           const float* __restrict__ s_src, const float* __restrict__ s_dst,
                                                           float slope, const float* __restrict__ alpha, float* ds,
                                                           float* __restrict__ ds_dst, int n_rows, int heads, int C, int lw,
                                                           int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        const float* grow = dOut + (int64_t)row * lddo;
        FOR_HEAD_PASSES(heads) {
            // dalpha_e for every entry (parked in ds) and delta = sum_e alpha_e dalpha_e, entries in ascending order
            float delta = 0.f;
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    const float* xp[NE];
                    float acc[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int e = rbase + min(b0 + k, nn - 1);
                        xp[k] = Hf + (int64_t)col[e] * ldh + hh * C;
                        acc[k] = 0.f;
                    }
                    for (int q = q0; q < W; q += lw) {
                        const float4 y = ld4(grow + hh * C + q * 4);
                        float4 x[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = ld4(xp[k] + q * 4);
#pragma unroll
                        for (int k = 0; k < NE; ++k) acc[k] = dot4(y, x[k], acc[k]);
                    }
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const float t = red_sum(acc[k], lw);
                        const bool ok = b0 + k < nn;
                        const int64_t e = rbase + min(b0 + k, nn - 1);
                        const float al = alpha[e * heads + hh];
                        delta = fmaf(ok ? al : 0.f, t, delta);
                        // lane (entry mod lw) of the head parks it: the lane that takes this entry in the sweep below
                        if (ok && hv && q0 == (k & (lw - 1))) ds[e * heads + h] = t;
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
            // ds_e = alpha_e (dalpha_e - delta) leaky'(z_e), and its row sum
            const float sd = s_dst[(int64_t)row * heads + hh];
            float part = 0.f;
            for (int e = q0; hv && e < nn; e += lw) {
                const int64_t ee = rbase + e;
                const float z0 = s_src[(int64_t)col[ee] * heads + h] + sd;
                const float v = alpha[ee * heads + h] * (ds[ee * heads + h] - delta) * (z0 > 0.f ? 1.f : slope);
                ds[ee * heads + h] = v;
                part += v;
            }
            part = red_sum(part, lw);
            if (hv && q0 == 0) ds_dst[(int64_t)row * heads + h] = part;
        }
    }
}

__global__ __launch_bounds__(256) void gat_bwd_edge_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                  const float* __restrict__ dOut, int64_t lddo,
                                                                  const float* __restrict__ Hf, int64_t ldh,
                                                                  const float* __restrict__ s_src, const float* __restrict__ s_dst,
                                                                  float slope, const float* __restrict__ alpha, float* ds,
                                                                  float* __restrict__ ds_dst, int n_rows, int heads, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    const float* grow = dOut + (int64_t)row * lddo;
    for (int h = 0; h < heads; ++h) {
        float delta = 0.f;
        for (int e = e0; e < e1; ++e) {
            const float* x = Hf + (int64_t)col[e] * ldh + h * C;
            float t = 0.f;
            for (int c = 0; c < C; ++c) t = fmaf(grow[h * C + c], x[c], t);
            ds[(int64_t)e * heads + h] = t;
            delta = fmaf(alpha[(int64_t)e * heads + h], t, delta);
        }
        const float sd = s_dst[(int64_t)row * heads + h];
        float part = 0.f;
        for (int e = e0; e < e1; ++e) {
            const float z0 = s_src[(int64_t)col[e] * heads + h] + sd;
            const float v = alpha[(int64_t)e * heads + h] * (ds[(int64_t)e * heads + h] - delta) * (z0 > 0.f ? 1.f : slope);
            ds[(int64_t)e * heads + h] = v;
            part += v;
        }
        ds_dst[(int64_t)row * heads + h] = part;
    }
}

// ------------------------------------------------------------------------------------------------ backward, node side
__global__ __launch_bounds__(256) void gat_bwd_node_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const int* __restrict__ mirror, const float* __restrict__ dOut,
                                                           int64_t lddo, const float* __restrict__ alpha, const float* __restrict__ ds,
                                                           const float* __restrict__ ds_dst, const float* __restrict__ att_src,
                                                           const float* __restrict__ att_dst, float* dHf, int64_t lddh,
                                                           float* __restrict__ ds_src, int n_rows, int heads, int C, int lw,
                                                           int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    FOR_CHUNK_ROW_ENTRIES {
        float* orow = dHf + (int64_t)row * lddh;
        FOR_HEAD_PASSES(heads) {
            float p = 0.f;
            for (int e = q0; e < nn; e += lw) p += ds[(int64_t)mirror[rbase + e] * heads + hh];
            p = red_sum(p, lw);
            const float dd = ds_dst[(int64_t)row * heads + hh];
            if (hv && q0 == 0) ds_src[(int64_t)row * heads + h] = p;
            gather_pass<true>(col, mirror, alpha, dOut, lddo, orow, rbase, nn, heads, C, hh, hv, q0, lw, [&](int q) {
                const float4 a = ld4(att_src + hh * C + q * 4), b = ld4(att_dst + hh * C + q * 4);
                return make_float4(fmaf(p, a.x, dd * b.x), fmaf(p, a.y, dd * b.y), fmaf(p, a.z, dd * b.z), fmaf(p, a.w, dd * b.w));
            });
        }
    }
}

__global__ __launch_bounds__(256) void gat_bwd_node_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                  const int* __restrict__ mirror, const float* __restrict__ dOut,
                                                                  int64_t lddo, const float* __restrict__ alpha,
                                                                  const float* __restrict__ ds, const float* __restrict__ ds_dst,
                                                                  const float* __restrict__ att_src, const float* __restrict__ att_dst,
                                                                  float* __restrict__ dHf, int64_t lddh, float* __restrict__ ds_src,
                                                                  int n_rows, int heads, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* orow = dHf + (int64_t)row * lddh;
    for (int h = 0; h < heads; ++h) {
        float p = 0.f;
        for (int e = e0; e < e1; ++e) p += ds[(int64_t)mirror[e] * heads + h];
        const float dd = ds_dst[(int64_t)row * heads + h];
        ds_src[(int64_t)row * heads + h] = p;
        for (int c = 0; c < C; ++c) {
            float acc = fmaf(p, att_src[h * C + c], dd * att_dst[h * C + c]);
            for (int e = e0; e < e1; ++e)
                acc = fmaf(alpha[(int64_t)mirror[e] * heads + h], dOut[(int64_t)col[e] * lddo + h * C + c], acc);
            orow[h * C + c] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ attention-vector gradient
// stage 1: partial[chunk][0 | 1][col] = sum over the chunk's kDR rows (ascending) of ds_{src | dst}[r, col / C] Hf[r, col]
__global__ __launch_bounds__(256) void gat_datt_partial_kernel(const float* __restrict__ Hf, int64_t ldh, int64_t n_rows, int heads,
                                                               int C, const float* __restrict__ ds_src,
                                                               const float* __restrict__ ds_dst, float* __restrict__ partial) {
    const int HC = heads * C;
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= HC) return;
    const int h = c / C;
    const int64_t ra = (int64_t)blockIdx.x * kDR, rb = ra + kDR < n_rows ? ra + kDR : n_rows;
    float ps = 0.f, pd = 0.f;
    for (int64_t r = ra; r < rb; ++r) {
        const float x = Hf[r * ldh + c];
        ps = fmaf(ds_src[r * heads + h], x, ps);
        pd = fmaf(ds_dst[r * heads + h], x, pd);
    }
    partial[((int64_t)blockIdx.x * 2 + 0) * HC + c] = ps;
    partial[((int64_t)blockIdx.x * 2 + 1) * HC + c] = pd;
}

inline bool gat_dims_ok(int heads, int C) { return heads > 0 && C > 0 && (int64_t)heads * C < (1 << 24); }

}  // namespace

extern "C" int ddmp_gat_scores_f32(const float* Hf, int64_t ldh, int64_t n_rows, int heads, int C, const float* att_src,
                                   const float* att_dst, float* s_src, float* s_dst, ddmp_stream stream) {
    ARG_TRY(Hf && att_src && att_dst && s_src && s_dst && n_rows >= 0 && n_rows < (int64_t)INT32_MAX && gat_dims_ok(heads, C) &&
            ldh >= (int64_t)heads * C);
    if (n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && ldh % 4 == 0 && al16(Hf) && al16(att_src) && al16(att_dst);
    return launch_head_rows((hipStream_t)stream, (int)n_rows, vec, lanes_per_head(C), gat_scores_kernel, gat_scores_scalar_kernel, Hf,
                            ldh, (int)n_rows, heads, C, att_src, att_dst, s_src, s_dst);
}

extern "C" int ddmp_gat_fwd_f32(const ddmp_graph* g, const float* Hf, int64_t ldh, int heads, int C, const float* s_src,
                                const float* s_dst, float slope, const float* bias, float* alpha, float* Y, int64_t ldy,
                                ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && Hf && s_src && s_dst && alpha && Y && gat_dims_ok(heads, C) && ldh >= (int64_t)heads * C &&
            ldy >= (int64_t)heads * C && Y != Hf);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && ldh % 4 == 0 && ldy % 4 == 0 && al16(Hf) && al16(Y) && (!bias || al16(bias));
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), gat_fwd_kernel, gat_fwd_scalar_kernel,
                            g->rowptr, g->col, g->a, Hf, ldh, s_src, s_dst, slope, bias, alpha, Y, ldy, (int)g->n_rows, heads, C);
}

extern "C" int ddmp_gat_bwd_edge_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Hf, int64_t ldh, int heads,
                                     int C, const float* s_src, const float* s_dst, float slope, const float* alpha, float* ds,
                                     float* ds_dst, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && dOut && Hf && s_src && s_dst && alpha && ds && ds_dst && gat_dims_ok(heads, C) &&
            lddo >= (int64_t)heads * C && ldh >= (int64_t)heads * C && ds != alpha);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddo % 4 == 0 && ldh % 4 == 0 && al16(dOut) && al16(Hf);
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), gat_bwd_edge_kernel,
                            gat_bwd_edge_scalar_kernel, g->rowptr, g->col, dOut, lddo, Hf, ldh, s_src, s_dst, slope, alpha, ds, ds_dst,
                            (int)g->n_rows, heads, C);
}

extern "C" int ddmp_gat_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, int heads, int C, const float* alpha,
                                     const float* ds, const float* ds_dst, const float* att_src, const float* att_dst, float* dHf,
                                     int64_t lddh, float* ds_src, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && dOut && alpha && ds && ds_dst && att_src && att_dst && dHf && ds_src && gat_dims_ok(heads, C) &&
            lddo >= (int64_t)heads * C && lddh >= (int64_t)heads * C && dHf != dOut);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddo % 4 == 0 && lddh % 4 == 0 && al16(dOut) && al16(dHf) && al16(att_src) && al16(att_dst);
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), gat_bwd_node_kernel,
                            gat_bwd_node_scalar_kernel, g->rowptr, g->col, g->mirror, dOut, lddo, alpha, ds, ds_dst, att_src, att_dst,
                            dHf, lddh, ds_src, (int)g->n_rows, heads, C);
}

extern "C" size_t ddmp_gat_datt_workspace_bytes(int64_t n_rows, int heads, int C) {
    if (n_rows <= 0 || heads <= 0 || C <= 0) return 0;
    return (size_t)cdiv(n_rows, kDR) * 2 * (size_t)heads * (size_t)C * sizeof(float);
}

extern "C" int ddmp_gat_datt_f32(const float* Hf, int64_t ldh, int64_t n_rows, int heads, int C, const float* ds_src,
                                 const float* ds_dst, float* datt_src, float* datt_dst, void* workspace, size_t workspace_bytes,
                                 ddmp_stream stream) {
    ARG_TRY(Hf && ds_src && ds_dst && datt_src && datt_dst && n_rows > 0 && n_rows < (int64_t)INT32_MAX && gat_dims_ok(heads, C) &&
            ldh >= (int64_t)heads * C);
    if (!workspace || workspace_bytes < ddmp_gat_datt_workspace_bytes(n_rows, heads, C)) return DDMP_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int HC = heads * C;
    const int n_chunks = (int)cdiv(n_rows, kDR);
    float* partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(gat_datt_partial_kernel, dim3(n_chunks, (unsigned)cdiv(HC, 256)), dim3(256), 0, st, Hf, ldh, n_rows, heads, C,
                       ds_src, ds_dst, partial);
    LAUNCH_TRY();
    return launch_colsum_final(st, partial, n_chunks, 2 * HC, datt_src, datt_dst, HC);
}

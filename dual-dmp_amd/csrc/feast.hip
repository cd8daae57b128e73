// Feature-steered convolution (FeaStConv): fused head softmax + gather, and the two backward launches.
//
//   q_e[h] = softmax over HEADS of (P[col e, h] - P[row e, h] + c[h]),  beta_e[h] = a_e q_e[h] / deg_i,  deg_i = sum_{row i} a_e,
//   Y[i,:] = sum_{e in row i} sum_h beta_e[h] Hf[col e, h, :]  (+ bias)
//
// over the COALESCED CSR of a valued graph left at all-ones values (a_e = the multiplicity of the entry), the graph of gat.hip, on
// the row-gather layout with head passes (row_gather.h).  The difference from graph attention: the softmax runs over the heads of
// ONE entry, and the heads are summed into one output row of width C.  With W = C / 4 float4 per head:
//   * W in {1, 2, 4}: the 8 / W heads of a pass sit side by side; in the forward each lane sums its heads and the 8 / W partial rows
//     are combined by a fixed xor tree;
//   * any other W: one head after the other.
// The factors beta (forward) and the dot products g (edge-side backward) are formed with the row's ENTRIES spread over the 8 lanes
// (each lane takes all heads of its entry: the head softmax needs no shuffle), written to their per-entry arrays and read back by
// the sibling lanes of the same wave after a workgroup-scope fence, as gat.hip's alpha is.  A shorter row's re-read last entry
// enters with factor 0.  An output float4 is accumulated in registers over ALL entries and heads of its row before it is stored:
// the 1200-entry hub row is exact like any other.  No LDS, no barrier in the gather kernels.  The three gather loops live in
// gather_mix.h, shared with gmm.hip.
#include "colsum_final.h"
#include "gather_mix.h"

namespace {

constexpr int kDR = 1024;          // rows per partial of the offset gradient

// beta_e[:] of one entry: the head softmax (exp arguments <= 0) times scale = a_e / deg_i
__device__ __forceinline__ void head_softmax(const float* __restrict__ pc, const float* __restrict__ pr, const float* __restrict__ cv,
                                             int heads, float scale, float* out) {
    float m = -INFINITY;
    for (int h = 0; h < heads; ++h) m = fmaxf(m, pc[h] - pr[h] + cv[h]);
    float s = 0.f;
    for (int h = 0; h < heads; ++h) s += expf(pc[h] - pr[h] + cv[h] - m);
    const float f = scale / s;                                    // (s >= 1: the largest head contributes exp(0))
    for (int h = 0; h < heads; ++h) out[h] = expf(pc[h] - pr[h] + cv[h] - m) * f;
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void feast_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const float* __restrict__ mult, const float* __restrict__ Hf, int64_t ldh,
                                                        const float* __restrict__ P, int64_t ldp, const float* __restrict__ cvec,
                                                        const float* __restrict__ bias, float* beta, float* __restrict__ Y,
                                                        int64_t ldy, int n_rows, int heads, int C, int lw, int chunks_per_xcd,
                                                        int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        float* yrow = Y + (int64_t)row * ldy;
        if (nn == 0) {                                            // a row without entries: the bias alone
            for (int q = sl; q < W; q += 8)
                *reinterpret_cast<float4*>(yrow + q * 4) = bias ? ld4(bias + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        // deg_i from the multiplicities, then beta of the row's entries: the 8 lanes take the entries 8 apart, all heads each
        float deg = 0.f;
        for (int e = sl; e < nn; e += 8) deg += mult[rbase + e];
        deg = red_sum(deg, 8);
        const float* prow = P + (int64_t)row * ldp;
        for (int e = sl; e < nn; e += 8) {
            const int64_t ee = rbase + e;
            head_softmax(P + (int64_t)col[ee] * ldp, prow, cvec, heads, mult[ee] / deg, beta + ee * heads);
        }
        // the gather reads the factors its sibling lanes wrote: same wave, same CU's L1 -- a workgroup-scope fence
        __threadfence_block();
        for (int q = q0; q < W; q += lw) {                        // (lw < 8: exactly one trip, all 8 lanes together)
            float4 acc = mix_gather_row(col, Hf, ldh, beta, heads, C, lw, hp, sub, rbase, nn, q);
            if (bias) {
                const float4 b = ld4(bias + q * 4);
                acc.x += b.x, acc.y += b.y, acc.z += b.z, acc.w += b.w;
            }
            if (sub == 0) *reinterpret_cast<float4*>(yrow + q * 4) = acc;
        }
    }
}

__global__ __launch_bounds__(256) void feast_fwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               const float* __restrict__ mult, const float* __restrict__ Hf,
                                                               int64_t ldh, const float* __restrict__ P, int64_t ldp,
                                                               const float* __restrict__ cvec, const float* __restrict__ bias,
                                                               float* beta, float* __restrict__ Y, int64_t ldy, int n_rows,
                                                               int heads, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* yrow = Y + (int64_t)row * ldy;
    float deg = 0.f;
    for (int e = e0; e < e1; ++e) deg += mult[e];
    const float* prow = P + (int64_t)row * ldp;
    for (int e = e0; e < e1; ++e) head_softmax(P + (int64_t)col[e] * ldp, prow, cvec, heads, mult[e] / deg, beta + (int64_t)e * heads);
    for (int c = 0; c < C; ++c) {
        float acc = 0.f;
        for (int e = e0; e < e1; ++e) {
            const float* x = Hf + (int64_t)col[e] * ldh + c;
            for (int h = 0; h < heads; ++h) acc = fmaf(beta[(int64_t)e * heads + h], x[h * C], acc);
        }
        yrow[c] = bias ? acc + bias[c] : acc;
    }
}

// ------------------------------------------------------------------------------------------------ backward, edge side
// dz_e[h] = beta_e[h] (g_e[h] - delta_e), delta_e = sum_h (beta_e[h] / m_e) g_e[h], m_e = sum_h beta_e[h]; rs[i,h] = sum_row dz_e[h].
// beta / m is q_e: with one head it is exactly 1, delta_e exactly g_e and dz exactly 0.
__device__ __forceinline__ float entry_delta(const float* bp, const float* gp, int heads) {
    float m = 0.f;
    for (int h = 0; h < heads; ++h) m += bp[h];
    float delta = 0.f;
    for (int h = 0; h < heads; ++h) delta = fmaf(bp[h] / m, gp[h], delta);
    return delta;
}

__global__ __launch_bounds__(256) void feast_bwd_edge_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ dOut, int64_t lddo,
                                                             const float* __restrict__ Hf, int64_t ldh,
                                                             const float* __restrict__ beta, float* dz, float* rs, int n_rows,
                                                             int heads, int C, int lw, int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    FOR_CHUNK_ROW_ENTRIES {
        const float* grow = dOut + (int64_t)row * lddo;
        float* rrow = rs + (int64_t)row * heads;
        if (nn == 0) {
            for (int h = sl; h < heads; h += 8) rrow[h] = 0.f;
            continue;
        }
        // g_e[h] = dOut[i,:] . Hf[col e, h, :] for every (entry, head), parked in dz
        mix_edge_dots(col, grow, Hf, ldh, dz, heads, C, lw, hp, sub, q0, rbase, nn);
        // the sweep below reads what the sibling lanes parked: same wave, same CU's L1 -- a workgroup-scope fence
        __threadfence_block();
        // one entry per lane, all heads: dz in place; its row sums by a fixed xor tree per 8 entries, accumulated through rs[i,:]
        // (same lane, same address, program order)
#pragma unroll 1
        for (int b0 = 0; b0 < nn; b0 += 8) {
            const bool ok = b0 + sl < nn;
            const int64_t ee = rbase + min(b0 + sl, nn - 1);
            const float* bp = beta + ee * heads;
            float* gp = dz + ee * heads;
            const float delta = entry_delta(bp, gp, heads);
            for (int h = 0; h < heads; ++h) {
                const float v = ok ? bp[h] * (gp[h] - delta) : 0.f;
                if (ok) gp[h] = v;
                const float s = red_sum(v, 8);
                if (sl == 0) rrow[h] = b0 == 0 ? s : rrow[h] + s;
            }
        }
    }
}

__global__ __launch_bounds__(256) void feast_bwd_edge_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const float* __restrict__ dOut, int64_t lddo,
                                                                    const float* __restrict__ Hf, int64_t ldh,
                                                                    const float* __restrict__ beta, float* dz, float* rs,
                                                                    int n_rows, int heads, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    const float* grow = dOut + (int64_t)row * lddo;
    float* rrow = rs + (int64_t)row * heads;
    for (int h = 0; h < heads; ++h) rrow[h] = 0.f;
    for (int e = e0; e < e1; ++e) {
        const float* bp = beta + (int64_t)e * heads;
        float* gp = dz + (int64_t)e * heads;
        for (int h = 0; h < heads; ++h) {
            const float* x = Hf + (int64_t)col[e] * ldh + h * C;
            float t = 0.f;
            for (int c = 0; c < C; ++c) t = fmaf(grow[c], x[c], t);
            gp[h] = t;
        }
        const float delta = entry_delta(bp, gp, heads);
        for (int h = 0; h < heads; ++h) {
            const float v = bp[h] * (gp[h] - delta);
            gp[h] = v;
            rrow[h] += v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, node side
__global__ __launch_bounds__(256) void feast_bwd_node_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const int* __restrict__ mirror, const float* __restrict__ dOut,
                                                             int64_t lddo, const float* __restrict__ beta,
                                                             const float* __restrict__ dz, const float* __restrict__ rs,
                                                             float* __restrict__ dHf, int64_t lddh, float* __restrict__ dP,
                                                             int64_t lddp, int n_rows, int heads, int C, int lw, int chunks_per_xcd,
                                                             int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        float* orow = dHf + (int64_t)row * lddh;
        FOR_HEAD_PASSES(heads) {
            // dP[j,h] = sum_{e'} dz[mirror e', h] - rs[j,h]: the head's lw lanes take the entries lw apart
            float p = 0.f;
            for (int e = q0; e < nn; e += lw) p += dz[(int64_t)mirror[rbase + e] * heads + hh];
            p = red_sum(p, lw);
            if (hv && q0 == 0) dP[(int64_t)row * lddp + h] = p - rs[(int64_t)row * heads + h];
            // dHf[j,h,:] = sum_{e'} beta[mirror e', h] dOut[col e', :]
            for (int q = q0; q < W; q += lw) {
                const float4 acc = mix_node_gather(col, mirror, dOut, lddo, beta, heads, hh, rbase, nn, q);
                if (hv) *reinterpret_cast<float4*>(orow + hh * C + q * 4) = acc;
            }
        }
    }
}

__global__ __launch_bounds__(256) void feast_bwd_node_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const int* __restrict__ mirror, const float* __restrict__ dOut,
                                                                    int64_t lddo, const float* __restrict__ beta,
                                                                    const float* __restrict__ dz, const float* __restrict__ rs,
                                                                    float* __restrict__ dHf, int64_t lddh, float* __restrict__ dP,
                                                                    int64_t lddp, int n_rows, int heads, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* orow = dHf + (int64_t)row * lddh;
    for (int h = 0; h < heads; ++h) {
        float p = 0.f;
        for (int e = e0; e < e1; ++e) p += dz[(int64_t)mirror[e] * heads + h];
        dP[(int64_t)row * lddp + h] = p - rs[(int64_t)row * heads + h];
        for (int c = 0; c < C; ++c) {
            float acc = 0.f;
            for (int e = e0; e < e1; ++e) acc = fmaf(beta[(int64_t)mirror[e] * heads + h], dOut[(int64_t)col[e] * lddo + c], acc);
            orow[h * C + c] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ offset gradient dc = colsum(rs)
// stage 1: partial[chunk][h] = sum over the chunk's kDR rows of rs[r, h].  The chunk is a flat run of kDR * heads floats; the
// first S = (256 / heads) * heads threads walk it S apart, so a thread's head never changes; thread h then adds the S / heads
// thread sums of its head in ascending thread order.
__global__ __launch_bounds__(256) void feast_dc_partial_kernel(const float* __restrict__ rs, int64_t n_rows, int heads,
                                                               float* __restrict__ partial) {
    __shared__ float sm[256];
    const int S = (256 / heads) * heads;
    const int64_t ra = (int64_t)blockIdx.x * kDR, rb = ra + kDR < n_rows ? ra + kDR : n_rows;
    const int64_t f0 = ra * heads, f1 = rb * heads;
    float t = 0.f;
    if ((int)threadIdx.x < S)
        for (int64_t f = f0 + threadIdx.x; f < f1; f += S) t += rs[f];
    sm[threadIdx.x] = t;
    __syncthreads();
    if ((int)threadIdx.x < heads) {
        float s = 0.f;
        for (int k = threadIdx.x; k < S; k += heads) s += sm[k];
        partial[(int64_t)blockIdx.x * heads + threadIdx.x] = s;
    }
}

}  // namespace

extern "C" int ddmp_feast_fwd_f32(const ddmp_graph* g, const float* Hf, int64_t ldh, const float* P, int64_t ldp, int heads, int C,
                                  const float* c, const float* bias, float* beta, float* Y, int64_t ldy, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && Hf && P && c && beta && Y && feast_dims_ok(heads, C) && ldh >= (int64_t)heads * C && ldp >= heads &&
            ldy >= C && Y != Hf && Y != P);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && ldh % 4 == 0 && ldy % 4 == 0 && al16(Hf) && al16(Y) && (!bias || al16(bias));
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), feast_fwd_kernel, feast_fwd_scalar_kernel,
                            g->rowptr, g->col, g->a, Hf, ldh, P, ldp, c, bias, beta, Y, ldy, (int)g->n_rows, heads, C);
}

extern "C" int ddmp_feast_bwd_edge_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Hf, int64_t ldh, int heads,
                                       int C, const float* beta, float* dz, float* rs, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && dOut && Hf && beta && dz && rs && feast_dims_ok(heads, C) && lddo >= C &&
            ldh >= (int64_t)heads * C && dz != beta);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddo % 4 == 0 && ldh % 4 == 0 && al16(dOut) && al16(Hf);
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), feast_bwd_edge_kernel,
                            feast_bwd_edge_scalar_kernel, g->rowptr, g->col, dOut, lddo, Hf, ldh, beta, dz, rs, (int)g->n_rows,
                            heads, C);
}

extern "C" int ddmp_feast_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, int heads, int C, const float* beta,
                                       const float* dz, const float* rs, float* dHf, int64_t lddh, float* dP, int64_t lddp,
                                       ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && dOut && beta && dz && rs && dHf && dP && feast_dims_ok(heads, C) && lddo >= C &&
            lddh >= (int64_t)heads * C && lddp >= heads && dHf != dOut && dP != rs);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddo % 4 == 0 && lddh % 4 == 0 && al16(dOut) && al16(dHf);
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), feast_bwd_node_kernel,
                            feast_bwd_node_scalar_kernel, g->rowptr, g->col, g->mirror, dOut, lddo, beta, dz, rs, dHf, lddh, dP,
                            lddp, (int)g->n_rows, heads, C);
}

extern "C" size_t ddmp_feast_dc_workspace_bytes(int64_t n_rows, int heads) {
    if (n_rows <= 0 || heads <= 0) return 0;
    return (size_t)cdiv(n_rows, kDR) * (size_t)heads * sizeof(float);
}

extern "C" int ddmp_feast_dc_f32(const float* rs, int64_t n_rows, int heads, float* dc, void* workspace, size_t workspace_bytes,
                                 ddmp_stream stream) {
    ARG_TRY(rs && dc && n_rows > 0 && n_rows < (int64_t)INT32_MAX && heads > 0 && heads <= kMaxHeads);
    if (!workspace || workspace_bytes < ddmp_feast_dc_workspace_bytes(n_rows, heads)) return DDMP_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int n_chunks = (int)cdiv(n_rows, kDR);
    float* partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(feast_dc_partial_kernel, dim3(n_chunks), dim3(256), 0, st, rs, n_rows, heads, partial);
    LAUNCH_TRY();
    return launch_colsum_final(st, partial, n_chunks, heads, dc, nullptr, heads);
}

// Dynamic graph attention (GATv2Conv): the score of an edge is a C-wide reduction over a per-edge quantity,
//
//   u_e[h,c] = Xl[col e, h, c] + Xr[row e, h, c],  z_e[h] = sum_c att[h,c] leaky_relu(u_e[h,c]),
//   alpha_e = a_e exp(z_e - max) / sum_row a_e exp(z_e - max),  Y[i,h,:] = sum_{e in row i} alpha_e Xl[col e, h, :]
//
// over the COALESCED CSR of the attention graph (a_e: the multiplicity of the entry, as in gat.hip).  On the row-gather layout
// with head passes (row_gather.h); its own part:
//   * every launch sweeps a row's entries TWICE in batches of kEB: once for the per-entry scalars (z_e, dalpha_e), which are parked
//     in the per-entry output array by the lane (entry mod lw) of the head -- the lane that takes the entry in the strided
//     softmax sweep -- and once for the feature-wide sums.  The second read of a neighbour row follows the first within one
//     (row, head) pass;
//   * the q loop (a head's float4 slabs) runs INSIDE a batch with one float4 per entry in flight, whatever the head's width: a
//     lane never holds more than kEB gathered float4 (two per entry in the node-side backward);
//   * a row longer than one batch accumulates through its own output rows (same lane, same address, program order);
//   * u_e is formed by ONE float32 addition everywhere (forward, both backward launches), so the branch of the leaky relu is the
//     same in all three.
// No LDS, no barrier, no atomics.
#include "colsum_final.h"

namespace {

constexpr int kDR = 256;           // rows per partial of the attention-vector gradient

__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.f ? x : slope * x; }
__device__ __forceinline__ float dleaky(float x, float slope) { return x > 0.f ? 1.f : slope; }
// acc + sum over the float4's channels of a leaky_relu(x + r)
__device__ __forceinline__ float score4(float4 a, float4 x, float4 r, float slope, float acc) {
    acc = fmaf(a.x, leaky(x.x + r.x, slope), acc);
    acc = fmaf(a.y, leaky(x.y + r.y, slope), acc);
    acc = fmaf(a.z, leaky(x.z + r.z, slope), acc);
    return fmaf(a.w, leaky(x.w + r.w, slope), acc);
}
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void gatv2_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const float* __restrict__ mult, const float* __restrict__ Xl, int64_t ldl,
                                                        const float* __restrict__ Xr, int64_t ldr, const float* __restrict__ att,
                                                        float slope, const float* __restrict__ bias, float* alpha, float* Y,
                                                        int64_t ldy, int n_rows, int heads, int C, int lw, int chunks_per_xcd,
                                                        int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        float* yrow = Y + (int64_t)row * ldy;
        FOR_HEAD_PASSES(heads) {
            const float* rh = Xr + (int64_t)row * ldr + hh * C;
            const float* ah = att + hh * C;
            // z_e for every entry (parked in alpha) and the row's maximum; every lane of the head holds the same sums
            float m = -INFINITY;
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    const float* xp[NE];
                    float acc[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int e = rbase + min(b0 + k, nn - 1);
                        xp[k] = Xl + (int64_t)col[e] * ldl + hh * C;
                        acc[k] = 0.f;
                    }
                    for (int q = q0; q < W; q += lw) {
                        const float4 r = ld4(rh + q * 4), a = ld4(ah + q * 4);
                        float4 x[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = ld4(xp[k] + q * 4);
#pragma unroll
                        for (int k = 0; k < NE; ++k) acc[k] = score4(a, x[k], r, slope, acc[k]);
                    }
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const float t = red_sum(acc[k], lw);
                        const bool ok = b0 + k < nn;
                        m = ok ? fmaxf(m, t) : m;
                        if (ok && hv && q0 == (k & (lw - 1))) alpha[(int64_t)(rbase + b0 + k) * heads + h] = t;
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
            // the softmax: the head's lw lanes take the entries lw apart -- each lane the entries it parked itself
            float den = 0.f;
            for (int e = q0; hv && e < nn; e += lw) den += mult[rbase + e] * expf(alpha[(int64_t)(rbase + e) * heads + h] - m);
            den = red_sum(den, lw);
            const float inv = 1.f / den;                          // (nn > 0: den >= the largest entry's multiplicity >= 1)
            for (int e = q0; hv && e < nn; e += lw) {
                const int64_t ee = rbase + e;
                alpha[ee * heads + h] = mult[ee] * expf(alpha[ee * heads + h] - m) * inv;
            }
            // the gather reads the factors its sibling lanes wrote: same wave, same CU's L1 -- a workgroup-scope fence
            __threadfence_block();
            gather_pass<false>(col, nullptr, alpha, Xl, ldl, yrow, rbase, nn, heads, C, hh, hv, q0, lw, [&](int q) {
                return bias ? ld4(bias + hh * C + q * 4) : zero4();
            });
        }
    }
}

__global__ __launch_bounds__(256) void gatv2_fwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               const float* __restrict__ mult, const float* __restrict__ Xl,
                                                               int64_t ldl, const float* __restrict__ Xr, int64_t ldr,
                                                               const float* __restrict__ att, float slope,
                                                               const float* __restrict__ bias, float* alpha, float* __restrict__ Y,
                                                               int64_t ldy, int n_rows, int heads, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* yrow = Y + (int64_t)row * ldy;
    for (int h = 0; h < heads; ++h) {
        const float* rh = Xr + (int64_t)row * ldr + h * C;
        float m = -INFINITY;
        for (int e = e0; e < e1; ++e) {
            const float* x = Xl + (int64_t)col[e] * ldl + h * C;
            float z = 0.f;
            for (int c = 0; c < C; ++c) z = fmaf(att[h * C + c], leaky(x[c] + rh[c], slope), z);
            alpha[(int64_t)e * heads + h] = z;
            m = fmaxf(m, z);
        }
        float den = 0.f;
        for (int e = e0; e < e1; ++e) den += mult[e] * expf(alpha[(int64_t)e * heads + h] - m);
        const float inv = 1.f / den;
        for (int e = e0; e < e1; ++e) alpha[(int64_t)e * heads + h] = mult[e] * expf(alpha[(int64_t)e * heads + h] - m) * inv;
        for (int c = 0; c < C; ++c) {
            float acc = bias ? bias[h * C + c] : 0.f;
            for (int e = e0; e < e1; ++e) acc = fmaf(alpha[(int64_t)e * heads + h], Xl[(int64_t)col[e] * ldl + h * C + c], acc);
            yrow[h * C + c] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, edge side
// dXr[i,h,:] = sum_{e in row i} dz_e att[h,:] leaky'(u_e[h,:]) and, `part` non-null, part[i,h,:] = sum_{e in row i} dz_e
// leaky(u_e[h,:]): the row's share of the attention-vector gradient.
__global__ __launch_bounds__(256) void gatv2_bwd_edge_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ dOut, int64_t lddo,
                                                             const float* __restrict__ Xl, int64_t ldl,
                                                             const float* __restrict__ Xr, int64_t ldr,
                                                             const float* __restrict__ att, float slope,
                                                             const float* __restrict__ alpha, float* dz, float* dXr, int64_t lddr,
                                                             float* part, int64_t ldp, int n_rows, int heads, int C, int lw,
                                                             int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        FOR_HEAD_PASSES(heads) {
            const float* gh = dOut + (int64_t)row * lddo + hh * C;
            const float* rh = Xr + (int64_t)row * ldr + hh * C;
            const float* ah = att + hh * C;
            float* xo = dXr + (int64_t)row * lddr + hh * C;
            float* po = part ? part + (int64_t)row * ldp + hh * C : nullptr;
            if (nn == 0) {
                for (int q = q0; hv && q < W; q += lw) {
                    *reinterpret_cast<float4*>(xo + q * 4) = zero4();
                    if (po) *reinterpret_cast<float4*>(po + q * 4) = zero4();
                }
                continue;
            }
            // dalpha_e for every entry (parked in dz) and delta = sum_e alpha_e dalpha_e, entries in ascending order
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
                        xp[k] = Xl + (int64_t)col[e] * ldl + hh * C;
                        acc[k] = 0.f;
                    }
                    for (int q = q0; q < W; q += lw) {
                        const float4 y = ld4(gh + q * 4);
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
                        if (ok && hv && q0 == (k & (lw - 1))) dz[e * heads + h] = t;
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
            // dz_e = alpha_e (dalpha_e - delta): each lane the entries it parked itself
            for (int e = q0; hv && e < nn; e += lw) {
                const int64_t ee = rbase + e;
                dz[ee * heads + h] = alpha[ee * heads + h] * (dz[ee * heads + h] - delta);
            }
            // the second sweep reads the dz its sibling lanes wrote
            __threadfence_block();
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    const float* xp[NE];
                    float f[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int64_t e = rbase + min(b0 + k, nn - 1);
                        xp[k] = Xl + (int64_t)col[e] * ldl + hh * C;
                        const float v = dz[e * heads + hh];
                        f[k] = b0 + k < nn ? v : 0.f;
                    }
                    for (int q = q0; q < W; q += lw) {
                        const float4 r = ld4(rh + q * 4), a = ld4(ah + q * 4);
                        float4 x[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = ld4(xp[k] + q * 4);
                        float4 s = zero4();
                        float4 p = (po && b0 != 0) ? ld4(po + q * 4) : zero4();
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            const float ux = x[k].x + r.x, uy = x[k].y + r.y, uz = x[k].z + r.z, uw = x[k].w + r.w;
                            s.x = fmaf(f[k], dleaky(ux, slope), s.x);
                            s.y = fmaf(f[k], dleaky(uy, slope), s.y);
                            s.z = fmaf(f[k], dleaky(uz, slope), s.z);
                            s.w = fmaf(f[k], dleaky(uw, slope), s.w);
                            p.x = fmaf(f[k], leaky(ux, slope), p.x);
                            p.y = fmaf(f[k], leaky(uy, slope), p.y);
                            p.z = fmaf(f[k], leaky(uz, slope), p.z);
                            p.w = fmaf(f[k], leaky(uw, slope), p.w);
                        }
                        float4 o = b0 == 0 ? zero4() : ld4(xo + q * 4);
                        o.x = fmaf(a.x, s.x, o.x);
                        o.y = fmaf(a.y, s.y, o.y);
                        o.z = fmaf(a.z, s.z, o.z);
                        o.w = fmaf(a.w, s.w, o.w);
                        if (hv) {
                            *reinterpret_cast<float4*>(xo + q * 4) = o;
                            if (po) *reinterpret_cast<float4*>(po + q * 4) = p;
                        }
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
        }
    }
}

__global__ __launch_bounds__(256) void gatv2_bwd_edge_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const float* __restrict__ dOut, int64_t lddo,
                                                                    const float* __restrict__ Xl, int64_t ldl,
                                                                    const float* __restrict__ Xr, int64_t ldr,
                                                                    const float* __restrict__ att, float slope,
                                                                    const float* __restrict__ alpha, float* dz,
                                                                    float* __restrict__ dXr, int64_t lddr, float* __restrict__ part,
                                                                    int64_t ldp, int n_rows, int heads, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int h = 0; h < heads; ++h) {
        const float* gh = dOut + (int64_t)row * lddo + h * C;
        const float* rh = Xr + (int64_t)row * ldr + h * C;
        float delta = 0.f;
        for (int e = e0; e < e1; ++e) {
            const float* x = Xl + (int64_t)col[e] * ldl + h * C;
            float t = 0.f;
            for (int c = 0; c < C; ++c) t = fmaf(gh[c], x[c], t);
            dz[(int64_t)e * heads + h] = t;
            delta = fmaf(alpha[(int64_t)e * heads + h], t, delta);
        }
        for (int e = e0; e < e1; ++e) dz[(int64_t)e * heads + h] = alpha[(int64_t)e * heads + h] * (dz[(int64_t)e * heads + h] - delta);
        for (int c = 0; c < C; ++c) {
            float s = 0.f, p = 0.f;
            for (int e = e0; e < e1; ++e) {
                const float u = Xl[(int64_t)col[e] * ldl + h * C + c] + rh[c];
                const float v = dz[(int64_t)e * heads + h];
                s = fmaf(v, dleaky(u, slope), s);
                p = fmaf(v, leaky(u, slope), p);
            }
            dXr[(int64_t)row * lddr + h * C + c] = att[h * C + c] * s;
            if (part) part[(int64_t)row * ldp + h * C + c] = p;
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, node side
// dXl[j,h,:] = sum_{e' in row j} alpha[mirror e'] dOut[col e', h, :] + att[h,:] sum_{e'} dz[mirror e'] leaky'(Xl[j,h,:] + Xr[col e', h, :])
__global__ __launch_bounds__(256) void gatv2_bwd_node_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const int* __restrict__ mirror, const float* __restrict__ dOut,
                                                             int64_t lddo, const float* __restrict__ Xl, int64_t ldl,
                                                             const float* __restrict__ Xr, int64_t ldr,
                                                             const float* __restrict__ att, float slope,
                                                             const float* __restrict__ alpha, const float* __restrict__ dz,
                                                             float* dXl, int64_t lddl, int n_rows, int heads, int C, int lw,
                                                             int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        FOR_HEAD_PASSES(heads) {
            const float* lh = Xl + (int64_t)row * ldl + hh * C;
            const float* ah = att + hh * C;
            float* orow = dXl + (int64_t)row * lddl + hh * C;
            if (nn == 0) {
                for (int q = q0; hv && q < W; q += lw) *reinterpret_cast<float4*>(orow + q * 4) = zero4();
                continue;
            }
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    const float* dp[NE];
                    const float* rp[NE];
                    float fa[NE], fz[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int e = rbase + min(b0 + k, nn - 1);
                        const int64_t c = col[e], mm = mirror[e];
                        dp[k] = dOut + c * lddo + hh * C;
                        rp[k] = Xr + c * ldr + hh * C;
                        const float va = alpha[mm * heads + hh], vz = dz[mm * heads + hh];
                        const bool ok = b0 + k < nn;
                        fa[k] = ok ? va : 0.f;
                        fz[k] = ok ? vz : 0.f;
                    }
                    for (int q = q0; q < W; q += lw) {
                        float* op = orow + q * 4;
                        const float4 xl = ld4(lh + q * 4), a = ld4(ah + q * 4);
                        float4 acc = b0 == 0 ? zero4() : ld4(op);
                        float4 d[NE], r[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            d[k] = ld4(dp[k] + q * 4);
                            r[k] = ld4(rp[k] + q * 4);
                        }
                        float4 s = zero4();
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            fma4(acc, fa[k], d[k]);
                            s.x = fmaf(fz[k], dleaky(xl.x + r[k].x, slope), s.x);
                            s.y = fmaf(fz[k], dleaky(xl.y + r[k].y, slope), s.y);
                            s.z = fmaf(fz[k], dleaky(xl.z + r[k].z, slope), s.z);
                            s.w = fmaf(fz[k], dleaky(xl.w + r[k].w, slope), s.w);
                        }
                        acc.x = fmaf(a.x, s.x, acc.x);
                        acc.y = fmaf(a.y, s.y, acc.y);
                        acc.z = fmaf(a.z, s.z, acc.z);
                        acc.w = fmaf(a.w, s.w, acc.w);
                        if (hv) *reinterpret_cast<float4*>(op) = acc;
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
        }
    }
}

__global__ __launch_bounds__(256) void gatv2_bwd_node_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const int* __restrict__ mirror, const float* __restrict__ dOut,
                                                                    int64_t lddo, const float* __restrict__ Xl, int64_t ldl,
                                                                    const float* __restrict__ Xr, int64_t ldr,
                                                                    const float* __restrict__ att, float slope,
                                                                    const float* __restrict__ alpha, const float* __restrict__ dz,
                                                                    float* __restrict__ dXl, int64_t lddl, int n_rows, int heads,
                                                                    int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int h = 0; h < heads; ++h)
        for (int c = 0; c < C; ++c) {
            const float xl = Xl[(int64_t)row * ldl + h * C + c];
            float acc = 0.f, s = 0.f;
            for (int e = e0; e < e1; ++e) {
                const int64_t j = col[e], mm = mirror[e];
                acc = fmaf(alpha[mm * heads + h], dOut[j * lddo + h * C + c], acc);
                s = fmaf(dz[mm * heads + h], dleaky(xl + Xr[j * ldr + h * C + c], slope), s);
            }
            dXl[(int64_t)row * lddl + h * C + c] = fmaf(att[h * C + c], s, acc);
        }
}

// ------------------------------------------------------------------------------------------------ attention-vector gradient
// stage 1: partial[chunk][col] = sum over the chunk's kDR rows (ascending) of part[r, col]
__global__ __launch_bounds__(256) void gatv2_datt_partial_kernel(const float* __restrict__ part, int64_t ldp, int64_t n_rows, int HC,
                                                                 float* __restrict__ partial) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= HC) return;
    const int64_t ra = (int64_t)blockIdx.x * kDR, rb = ra + kDR < n_rows ? ra + kDR : n_rows;
    float p = 0.f;
    for (int64_t r = ra; r < rb; ++r) p += part[r * ldp + c];
    partial[(int64_t)blockIdx.x * HC + c] = p;
}

inline bool gatv2_dims_ok(int heads, int C) { return heads > 0 && C > 0 && (int64_t)heads * C < (1 << 24); }
inline bool ld_ok(int64_t ld, int heads, int C) { return ld >= (int64_t)heads * C; }

}  // namespace

extern "C" int ddmp_gatv2_fwd_f32(const ddmp_graph* g, const float* Xl, int64_t ldl, const float* Xr, int64_t ldr, int heads, int C,
                                  const float* att, float slope, const float* bias, float* alpha, float* Y, int64_t ldy,
                                  ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && Xl && Xr && att && alpha && Y && gatv2_dims_ok(heads, C) && ld_ok(ldl, heads, C) &&
            ld_ok(ldr, heads, C) && ld_ok(ldy, heads, C) && Y != Xl && Y != Xr);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && ldl % 4 == 0 && ldr % 4 == 0 && ldy % 4 == 0 && al16(Xl) && al16(Xr) && al16(att) && al16(Y) &&
                     (!bias || al16(bias));
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), gatv2_fwd_kernel, gatv2_fwd_scalar_kernel,
                            g->rowptr, g->col, g->a, Xl, ldl, Xr, ldr, att, slope, bias, alpha, Y, ldy, (int)g->n_rows, heads, C);
}

extern "C" int ddmp_gatv2_bwd_edge_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Xl, int64_t ldl,
                                       const float* Xr, int64_t ldr, int heads, int C, const float* att, float slope,
                                       const float* alpha, float* dz, float* dXr, int64_t lddr, float* part, int64_t ldp,
                                       ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && dOut && Xl && Xr && att && alpha && dz && dXr && gatv2_dims_ok(heads, C) && ld_ok(lddo, heads, C) &&
            ld_ok(ldl, heads, C) && ld_ok(ldr, heads, C) && ld_ok(lddr, heads, C) && (!part || ld_ok(ldp, heads, C)) && dz != alpha &&
            dXr != dOut && dXr != Xl && dXr != Xr && part != dXr && part != dOut && part != Xl && part != Xr);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddo % 4 == 0 && ldl % 4 == 0 && ldr % 4 == 0 && lddr % 4 == 0 && al16(dOut) && al16(Xl) &&
                     al16(Xr) && al16(att) && al16(dXr) && (!part || (ldp % 4 == 0 && al16(part)));
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), gatv2_bwd_edge_kernel,
                            gatv2_bwd_edge_scalar_kernel, g->rowptr, g->col, dOut, lddo, Xl, ldl, Xr, ldr, att, slope, alpha, dz, dXr,
                            lddr, part, ldp, (int)g->n_rows, heads, C);
}

extern "C" int ddmp_gatv2_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Xl, int64_t ldl,
                                       const float* Xr, int64_t ldr, int heads, int C, const float* att, float slope,
                                       const float* alpha, const float* dz, float* dXl, int64_t lddl, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && dOut && Xl && Xr && att && alpha && dz && dXl && gatv2_dims_ok(heads, C) && ld_ok(lddo, heads, C) &&
            ld_ok(ldl, heads, C) && ld_ok(ldr, heads, C) && ld_ok(lddl, heads, C) && dXl != dOut && dXl != Xl && dXl != Xr);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddo % 4 == 0 && ldl % 4 == 0 && ldr % 4 == 0 && lddl % 4 == 0 && al16(dOut) && al16(Xl) &&
                     al16(Xr) && al16(att) && al16(dXl);
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), gatv2_bwd_node_kernel,
                            gatv2_bwd_node_scalar_kernel, g->rowptr, g->col, g->mirror, dOut, lddo, Xl, ldl, Xr, ldr, att, slope,
                            alpha, dz, dXl, lddl, (int)g->n_rows, heads, C);
}

extern "C" size_t ddmp_gatv2_datt_workspace_bytes(int64_t n_rows, int heads, int C) {
    if (n_rows <= 0 || heads <= 0 || C <= 0) return 0;
    return (size_t)cdiv(n_rows, kDR) * (size_t)heads * (size_t)C * sizeof(float);
}

extern "C" int ddmp_gatv2_datt_f32(const float* part, int64_t ldp, int64_t n_rows, int heads, int C, float* datt, void* workspace,
                                   size_t workspace_bytes, ddmp_stream stream) {
    ARG_TRY(part && datt && n_rows > 0 && n_rows < (int64_t)INT32_MAX && gatv2_dims_ok(heads, C) && ld_ok(ldp, heads, C));
    if (!workspace || workspace_bytes < ddmp_gatv2_datt_workspace_bytes(n_rows, heads, C)) return DDMP_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int HC = heads * C;
    const int n_chunks = (int)cdiv(n_rows, kDR);
    float* partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(gatv2_datt_partial_kernel, dim3(n_chunks, (unsigned)cdiv(HC, 256)), dim3(256), 0, st, part, ldp, n_rows, HC,
                       partial);
    LAUNCH_TRY();
    return launch_colsum_final(st, partial, n_chunks, HC, datt, nullptr, HC);
}

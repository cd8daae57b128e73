// Graph transformer (TransformerConv): scaled dot-product attention over the edges,
//
//   z_e[h] = scale * Q[row e, h, :] . K[col e, h, :],  alpha_e = a_e exp(z_e - max) / sum_row a_e exp(z_e - max),
//   Y[i,h,:] = skip[i,h,:] + sum_{e in row i} alpha_e V[col e, h, :]
//
// over the COALESCED CSR of the attention graph (a_e: the multiplicity of the entry, as in gat.hip).  The stream that is scored
// (K) is not the stream that is gathered (V).  On the row-gather layout with head passes (row_gather.h), in gatv2.hip's two-sweep
// shape:
//   * every launch of the row side sweeps a row's entries TWICE in batches of kEB: once for the per-entry scalars (z_e, dalpha_e),
//     which are parked in the per-entry output array by the lane (entry mod lw) of the head -- the lane that takes the entry in
//     the strided softmax sweep -- and once for the feature-wide sums (V in the forward, K in the edge-side backward);
//   * the q loop (a head's float4 slabs) runs INSIDE a batch with one float4 per entry in flight, whatever the head's width (two
//     per entry in the node-side backward, whose two neighbour streams Q and dOut are in flight together);
//   * a row longer than one batch accumulates through its own output rows (same lane, same address, program order).
// No LDS, no barrier, no atomics.
#include "row_gather.h"

namespace {

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void tconv_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        const float* __restrict__ mult, const float* __restrict__ Q, int64_t ldq,
                                                        const float* __restrict__ K, int64_t ldk, const float* __restrict__ V,
                                                        int64_t ldv, float scale, const float* __restrict__ skip, int64_t lds,
                                                        float* alpha, float* Y, int64_t ldy, int n_rows, int heads, int C, int lw,
                                                        int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        float* yrow = Y + (int64_t)row * ldy;
        const float* srow = skip ? skip + (int64_t)row * lds : nullptr;
        FOR_HEAD_PASSES(heads) {
            const float* qh = Q + (int64_t)row * ldq + hh * C;
            // z_e for every entry (parked in alpha) and the row's maximum; every lane of the head holds the same sums
            float m = -INFINITY;
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    const float* kp[NE];
                    float acc[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int e = rbase + min(b0 + k, nn - 1);
                        kp[k] = K + (int64_t)col[e] * ldk + hh * C;
                        acc[k] = 0.f;
                    }
                    for (int q = q0; q < W; q += lw) {
                        const float4 r = ld4(qh + q * 4);
                        float4 x[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = ld4(kp[k] + q * 4);
#pragma unroll
                        for (int k = 0; k < NE; ++k) acc[k] = dot4(r, x[k], acc[k]);
                    }
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const float t = scale * red_sum(acc[k], lw);
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
            gather_pass<false>(col, nullptr, alpha, V, ldv, yrow, rbase, nn, heads, C, hh, hv, q0, lw, [&](int q) {
                return srow ? ld4(srow + hh * C + q * 4) : zero4();
            });
        }
    }
}

__global__ __launch_bounds__(256) void tconv_fwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               const float* __restrict__ mult, const float* __restrict__ Q,
                                                               int64_t ldq, const float* __restrict__ K, int64_t ldk,
                                                               const float* __restrict__ V, int64_t ldv, float scale,
                                                               const float* __restrict__ skip, int64_t lds, float* alpha,
                                                               float* __restrict__ Y, int64_t ldy, int n_rows, int heads, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* yrow = Y + (int64_t)row * ldy;
    for (int h = 0; h < heads; ++h) {
        const float* qh = Q + (int64_t)row * ldq + h * C;
        float m = -INFINITY;
        for (int e = e0; e < e1; ++e) {
            const float* x = K + (int64_t)col[e] * ldk + h * C;
            float z = 0.f;
            for (int c = 0; c < C; ++c) z = fmaf(qh[c], x[c], z);
            z *= scale;
            alpha[(int64_t)e * heads + h] = z;
            m = fmaxf(m, z);
        }
        float den = 0.f;
        for (int e = e0; e < e1; ++e) den += mult[e] * expf(alpha[(int64_t)e * heads + h] - m);
        const float inv = 1.f / den;
        for (int e = e0; e < e1; ++e) alpha[(int64_t)e * heads + h] = mult[e] * expf(alpha[(int64_t)e * heads + h] - m) * inv;
        for (int c = 0; c < C; ++c) {
            float acc = skip ? skip[(int64_t)row * lds + h * C + c] : 0.f;
            for (int e = e0; e < e1; ++e) acc = fmaf(alpha[(int64_t)e * heads + h], V[(int64_t)col[e] * ldv + h * C + c], acc);
            yrow[h * C + c] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, edge side
// dz_e = alpha_e (dOut[i,h,:] . V[col e, h, :] - delta), delta = sum_{e in row i} alpha_e dalpha_e;  dQ[i,h,:] = scale sum_e dz_e
// K[col e, h, :]
__global__ __launch_bounds__(256) void tconv_bwd_edge_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ dOut, int64_t lddo,
                                                             const float* __restrict__ K, int64_t ldk, const float* __restrict__ V,
                                                             int64_t ldv, float scale, const float* __restrict__ alpha, float* dz,
                                                             float* dQ, int64_t lddq, int n_rows, int heads, int C, int lw,
                                                             int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        FOR_HEAD_PASSES(heads) {
            const float* gh = dOut + (int64_t)row * lddo + hh * C;
            float* xo = dQ + (int64_t)row * lddq + hh * C;
            if (nn == 0) {
                for (int q = q0; hv && q < W; q += lw) *reinterpret_cast<float4*>(xo + q * 4) = zero4();
                continue;
            }
            // dalpha_e for every entry (parked in dz) and delta = sum_e alpha_e dalpha_e, entries in ascending order
            float delta = 0.f;
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    const float* vp[NE];
                    float acc[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int e = rbase + min(b0 + k, nn - 1);
                        vp[k] = V + (int64_t)col[e] * ldv + hh * C;
                        acc[k] = 0.f;
                    }
                    for (int q = q0; q < W; q += lw) {
                        const float4 y = ld4(gh + q * 4);
                        float4 x[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = ld4(vp[k] + q * 4);
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
                    const float* kp[NE];
                    float f[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int64_t e = rbase + min(b0 + k, nn - 1);
                        kp[k] = K + (int64_t)col[e] * ldk + hh * C;
                        const float v = scale * dz[e * heads + hh];
                        f[k] = b0 + k < nn ? v : 0.f;
                    }
                    for (int q = q0; q < W; q += lw) {
                        float4 o = b0 == 0 ? zero4() : ld4(xo + q * 4);
                        float4 x[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = ld4(kp[k] + q * 4);
#pragma unroll
                        for (int k = 0; k < NE; ++k) fma4(o, f[k], x[k]);
                        if (hv) *reinterpret_cast<float4*>(xo + q * 4) = o;
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
        }
    }
}

__global__ __launch_bounds__(256) void tconv_bwd_edge_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const float* __restrict__ dOut, int64_t lddo,
                                                                    const float* __restrict__ K, int64_t ldk,
                                                                    const float* __restrict__ V, int64_t ldv, float scale,
                                                                    const float* __restrict__ alpha, float* dz,
                                                                    float* __restrict__ dQ, int64_t lddq, int n_rows, int heads,
                                                                    int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int h = 0; h < heads; ++h) {
        const float* gh = dOut + (int64_t)row * lddo + h * C;
        float delta = 0.f;
        for (int e = e0; e < e1; ++e) {
            const float* x = V + (int64_t)col[e] * ldv + h * C;
            float t = 0.f;
            for (int c = 0; c < C; ++c) t = fmaf(gh[c], x[c], t);
            dz[(int64_t)e * heads + h] = t;
            delta = fmaf(alpha[(int64_t)e * heads + h], t, delta);
        }
        for (int e = e0; e < e1; ++e) dz[(int64_t)e * heads + h] = alpha[(int64_t)e * heads + h] * (dz[(int64_t)e * heads + h] - delta);
        for (int c = 0; c < C; ++c) {
            float s = 0.f;
            for (int e = e0; e < e1; ++e) s = fmaf(scale * dz[(int64_t)e * heads + h], K[(int64_t)col[e] * ldk + h * C + c], s);
            dQ[(int64_t)row * lddq + h * C + c] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, node side
// dK[j,h,:] = scale sum_{e' in row j} dz[mirror e'] Q[col e', h, :],  dV[j,h,:] = sum_{e'} alpha[mirror e'] dOut[col e', h, :] and
// (dS non-null) the skip block's gradient dS[j,:] = dOut[j,:] copied into its columns of the same row buffer.
__global__ __launch_bounds__(256) void tconv_bwd_node_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const int* __restrict__ mirror, const float* __restrict__ dOut,
                                                             int64_t lddo, const float* __restrict__ Q, int64_t ldq, float scale,
                                                             const float* __restrict__ alpha, const float* __restrict__ dz,
                                                             float* dK, int64_t lddk, float* dV, int64_t lddv, float* dS,
                                                             int64_t ldds, int n_rows, int heads, int C, int lw, int chunks_per_xcd,
                                                             int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        if (dS)
            for (int q = sl; q < heads * W; q += 8)
                *reinterpret_cast<float4*>(dS + (int64_t)row * ldds + q * 4) = ld4(dOut + (int64_t)row * lddo + q * 4);
        FOR_HEAD_PASSES(heads) {
            float* ko = dK + (int64_t)row * lddk + hh * C;
            float* vo = dV + (int64_t)row * lddv + hh * C;
            if (nn == 0) {
                for (int q = q0; hv && q < W; q += lw) {
                    *reinterpret_cast<float4*>(ko + q * 4) = zero4();
                    *reinterpret_cast<float4*>(vo + q * 4) = zero4();
                }
                continue;
            }
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    const float* dp[NE];
                    const float* qp[NE];
                    float fa[NE], fz[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int e = rbase + min(b0 + k, nn - 1);
                        const int64_t c = col[e], mm = mirror[e];
                        dp[k] = dOut + c * lddo + hh * C;
                        qp[k] = Q + c * ldq + hh * C;
                        const float va = alpha[mm * heads + hh], vz = scale * dz[mm * heads + hh];
                        const bool ok = b0 + k < nn;
                        fa[k] = ok ? va : 0.f;
                        fz[k] = ok ? vz : 0.f;
                    }
                    for (int q = q0; q < W; q += lw) {
                        float4 ak = b0 == 0 ? zero4() : ld4(ko + q * 4);
                        float4 av = b0 == 0 ? zero4() : ld4(vo + q * 4);
                        float4 d[NE], r[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            d[k] = ld4(dp[k] + q * 4);
                            r[k] = ld4(qp[k] + q * 4);
                        }
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            fma4(av, fa[k], d[k]);
                            fma4(ak, fz[k], r[k]);
                        }
                        if (hv) {
                            *reinterpret_cast<float4*>(ko + q * 4) = ak;
                            *reinterpret_cast<float4*>(vo + q * 4) = av;
                        }
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
        }
    }
}

__global__ __launch_bounds__(256) void tconv_bwd_node_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const int* __restrict__ mirror, const float* __restrict__ dOut,
                                                                    int64_t lddo, const float* __restrict__ Q, int64_t ldq,
                                                                    float scale, const float* __restrict__ alpha,
                                                                    const float* __restrict__ dz, float* __restrict__ dK,
                                                                    int64_t lddk, float* __restrict__ dV, int64_t lddv,
                                                                    float* __restrict__ dS, int64_t ldds, int n_rows, int heads,
                                                                    int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    if (dS)
        for (int c = 0; c < heads * C; ++c) dS[(int64_t)row * ldds + c] = dOut[(int64_t)row * lddo + c];
    for (int h = 0; h < heads; ++h)
        for (int c = 0; c < C; ++c) {
            float ak = 0.f, av = 0.f;
            for (int e = e0; e < e1; ++e) {
                const int64_t j = col[e], mm = mirror[e];
                av = fmaf(alpha[mm * heads + h], dOut[j * lddo + h * C + c], av);
                ak = fmaf(scale * dz[mm * heads + h], Q[j * ldq + h * C + c], ak);
            }
            dK[(int64_t)row * lddk + h * C + c] = ak;
            dV[(int64_t)row * lddv + h * C + c] = av;
        }
}

inline bool tconv_dims_ok(int heads, int C) { return heads > 0 && C > 0 && (int64_t)heads * C < (1 << 24); }
inline bool ld_ok(int64_t ld, int heads, int C) { return ld >= (int64_t)heads * C; }
inline bool vec_ok(const float* p, int64_t ld) { return al16(p) && ld % 4 == 0; }

}  // namespace

extern "C" int ddmp_tconv_fwd_f32(const ddmp_graph* g, const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V,
                                  int64_t ldv, int heads, int C, float scale, const float* skip, int64_t lds, float* alpha, float* Y,
                                  int64_t ldy, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && Q && K && V && alpha && Y && tconv_dims_ok(heads, C) && ld_ok(ldq, heads, C) && ld_ok(ldk, heads, C) &&
            ld_ok(ldv, heads, C) && ld_ok(ldy, heads, C) && (!skip || ld_ok(lds, heads, C)) && Y != Q && Y != K && Y != V && Y != skip);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(Q, ldq) && vec_ok(K, ldk) && vec_ok(V, ldv) && vec_ok(Y, ldy) && (!skip || vec_ok(skip, lds));
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), tconv_fwd_kernel, tconv_fwd_scalar_kernel,
                            g->rowptr, g->col, g->a, Q, ldq, K, ldk, V, ldv, scale, skip, lds, alpha, Y, ldy, (int)g->n_rows, heads, C);
}

extern "C" int ddmp_tconv_bwd_edge_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* K, int64_t ldk,
                                       const float* V, int64_t ldv, int heads, int C, float scale, const float* alpha, float* dz,
                                       float* dQ, int64_t lddq, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && dOut && K && V && alpha && dz && dQ && tconv_dims_ok(heads, C) && ld_ok(lddo, heads, C) &&
            ld_ok(ldk, heads, C) && ld_ok(ldv, heads, C) && ld_ok(lddq, heads, C) && dz != alpha && dQ != dOut && dQ != K && dQ != V);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(dOut, lddo) && vec_ok(K, ldk) && vec_ok(V, ldv) && vec_ok(dQ, lddq);
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), tconv_bwd_edge_kernel,
                            tconv_bwd_edge_scalar_kernel, g->rowptr, g->col, dOut, lddo, K, ldk, V, ldv, scale, alpha, dz, dQ, lddq,
                            (int)g->n_rows, heads, C);
}

extern "C" int ddmp_tconv_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Q, int64_t ldq, int heads,
                                       int C, float scale, const float* alpha, const float* dz, float* dK, int64_t lddk, float* dV,
                                       int64_t lddv, float* dS, int64_t ldds, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && dOut && Q && alpha && dz && dK && dV && tconv_dims_ok(heads, C) && ld_ok(lddo, heads, C) &&
            ld_ok(ldq, heads, C) && ld_ok(lddk, heads, C) && ld_ok(lddv, heads, C) && (!dS || ld_ok(ldds, heads, C)) && dK != dV &&
            dK != dOut && dK != Q && dV != dOut && dV != Q && dS != dOut && dS != Q && dS != dK && dS != dV);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(dOut, lddo) && vec_ok(Q, ldq) && vec_ok(dK, lddk) && vec_ok(dV, lddv) &&
                     (!dS || vec_ok(dS, ldds));
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), tconv_bwd_node_kernel,
                            tconv_bwd_node_scalar_kernel, g->rowptr, g->col, g->mirror, dOut, lddo, Q, ldq, scale, alpha, dz, dK, lddk,
                            dV, lddv, dS, ldds, (int)g->n_rows, heads, C);
}

// Gaussian-mixture convolution (MoNet's GMMConv): fused per-edge Gaussians + gather, and the two backward launches.
//
//   gamma_t[k] = exp(-1/2 sum_d (a_t[d] - mu[k,d])^2 / (EPS + sigma[k,d]^2))      for an input edge t with pseudo-coordinates a_t,
//   w_e[k]     = (1 / deg_i) sum_{t in edges of e} gamma_t[k],                     deg_i = sum_{row i} a_e (the multiplicities),
//   Y[i,:]     = sum_{e in row i} sum_k w_e[k] Hf[col e, k, :]  (+ R[i,:]) (+ bias)
//
// over the COALESCED CSR of a valued graph built WITHOUT loop handling (flags 0) and left at all-ones values; an entry's input
// edges come from its ee_ptr / ee_idx span, in input order -- exact for duplicate edges whose pseudo-coordinates differ.
// On the row-gather layout with head passes (row_gather.h) and the gather loops of gather_mix.h, shared with feast.hip: the
// per-entry factors are formed with the row's entries spread over the 8 lanes, written to their [entries, K] array and read back by
// the sibling lanes behind a workgroup-scope fence.  mu, 1 / (EPS + sigma^2) and sigma are staged once per workgroup in LDS (K * dim
// <= 128 floats each; one barrier before the first row).
#include "gather_mix.h"

namespace {

constexpr int kMaxKD = 128;        // K * dim: the [n, 2 K dim] partials go through the 256-column reduction of feast.hip
constexpr float kEps = 1e-15f;

// mu, inv = 1 / (EPS + sigma^2) and sigma of every (k, d) -> LDS, once per workgroup (not per edge)
#define GMM_TABLES                                                                                 \
    __shared__ float s_mu[kMaxKD], s_inv[kMaxKD], s_sg[kMaxKD];                                    \
    for (int p = threadIdx.x; p < K * dim; p += blockDim.x) {                                      \
        const float sg = sigma[p];                                                                 \
        s_mu[p] = mu[p];                                                                           \
        s_sg[p] = sg;                                                                              \
        s_inv[p] = 1.0f / (kEps + sg * sg);                                                        \
    }                                                                                              \
    __syncthreads();

// gamma_t[k] of one input edge (a: its dim pseudo-coordinates; mk / ik: row k of the LDS tables).  The exp argument is <= 0.
__device__ __forceinline__ float gauss(const float* __restrict__ a, const float* mk, const float* ik, int dim) {
    float s = 0.f;
    for (int d = 0; d < dim; ++d) {
        const float df = a[d] - mk[d];
        s = fmaf(df * df, ik[d], s);
    }
    return expf(-0.5f * s);
}

// w_e[:] of one entry: its input edges in input order, divided by deg_i
__device__ __forceinline__ void entry_weights(const int* __restrict__ ee_ptr, const int* __restrict__ ee_idx,
                                              const float* __restrict__ attr, const float* s_mu, const float* s_inv, int K, int dim,
                                              int64_t e, float deg, float* out) {
    const int t0 = ee_ptr[e], t1 = ee_ptr[e + 1];
    for (int k = 0; k < K; ++k) {
        float acc = 0.f;
        for (int t = t0; t < t1; ++t) acc += gauss(attr + (int64_t)ee_idx[t] * dim, s_mu + k * dim, s_inv + k * dim, dim);
        out[k] = acc / deg;
    }
}

// The dmu / dsigma terms of one entry for component k and the coordinates d0 .. d0 + 3: its input edges in input order.
//   c_t = gamma_t[k] G / deg,  u = c_t (a_t[d] - mu[k,d]) inv[k,d]  (the dmu term),  u (a_t[d] - mu[k,d]) sigma[k,d] inv[k,d]  (dsigma)
__device__ __forceinline__ void entry_param_terms(const int* __restrict__ ee_idx, const float* __restrict__ attr, const float* mk,
                                                  const float* ik, const float* sk, int dim, int d0, int t0, int t1, float gs,
                                                  float (&pm)[4], float (&ps)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) pm[j] = ps[j] = 0.f;
    for (int t = t0; t < t1; ++t) {
        const float* a = attr + (int64_t)ee_idx[t] * dim;
        const float c = gauss(a, mk, ik, dim) * gs;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (d0 + j < dim) {
                const float df = a[d0 + j] - mk[d0 + j];
                const float u = c * df * ik[d0 + j];
                pm[j] += u;
                ps[j] += u * df * (sk[d0 + j] * ik[d0 + j]);
            }
        }
    }
}

// dattr[t, :] = - sum_k c_t[k] (a_t[d] - mu[k,d]) inv[k,d] of every input edge of one entry (gp: the entry's G[:], K values)
__device__ __forceinline__ void entry_dattr(const int* __restrict__ ee_idx, const float* __restrict__ attr, const float* s_mu,
                                            const float* s_inv, int K, int dim, int t0, int t1, const float* gp, float deg,
                                            float* __restrict__ dattr) {
    for (int t = t0; t < t1; ++t) {
        const int64_t ed = ee_idx[t];
        const float* a = attr + ed * dim;
        for (int d0 = 0; d0 < dim; d0 += 4) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < K; ++k) {
                const float* mk = s_mu + k * dim;
                const float* ik = s_inv + k * dim;
                const float c = gauss(a, mk, ik, dim) * (gp[k] / deg);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d0 + j < dim) acc[j] -= c * (a[d0 + j] - mk[d0 + j]) * ik[d0 + j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (d0 + j < dim) dattr[ed * dim + d0 + j] = acc[j];
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void gmm_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                      const float* __restrict__ mult, const int* __restrict__ ee_ptr,
                                                      const int* __restrict__ ee_idx, const float* __restrict__ Hf, int64_t ldh,
                                                      const float* __restrict__ attr, int dim, const float* __restrict__ mu,
                                                      const float* __restrict__ sigma, const float* __restrict__ R, int64_t ldr,
                                                      const float* __restrict__ bias, float* w, float* __restrict__ Y, int64_t ldy,
                                                      int n_rows, int K, int C, int lw, int chunks_per_xcd, int n_chunks) {
    GMM_TABLES
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        float* yrow = Y + (int64_t)row * ldy;
        const float* rrow = R ? R + (int64_t)row * ldr : nullptr;
        if (nn == 0) {                                            // a row without entries: its own root block and the bias
            for (int q = sl; q < W; q += 8) {
                float4 acc = rrow ? ld4(rrow + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                if (bias) {
                    const float4 b = ld4(bias + q * 4);
                    acc.x += b.x, acc.y += b.y, acc.z += b.z, acc.w += b.w;
                }
                *reinterpret_cast<float4*>(yrow + q * 4) = acc;
            }
            continue;
        }
        // deg_i from the multiplicities, then w of the row's entries: the 8 lanes take the entries 8 apart, all components each
        float deg = 0.f;
        for (int e = sl; e < nn; e += 8) deg += mult[rbase + e];
        deg = red_sum(deg, 8);
        for (int e = sl; e < nn; e += 8) {
            const int64_t ee = rbase + e;
            entry_weights(ee_ptr, ee_idx, attr, s_mu, s_inv, K, dim, ee, deg, w + ee * K);
        }
        // the gather reads the factors its sibling lanes wrote: same wave, same CU's L1 -- a workgroup-scope fence
        __threadfence_block();
        for (int q = q0; q < W; q += lw) {                        // (lw < 8: exactly one trip, all 8 lanes together)
            float4 acc = mix_gather_row(col, Hf, ldh, w, K, C, lw, hp, sub, rbase, nn, q);
            if (rrow) {
                const float4 r = ld4(rrow + q * 4);
                acc.x += r.x, acc.y += r.y, acc.z += r.z, acc.w += r.w;
            }
            if (bias) {
                const float4 b = ld4(bias + q * 4);
                acc.x += b.x, acc.y += b.y, acc.z += b.z, acc.w += b.w;
            }
            if (sub == 0) *reinterpret_cast<float4*>(yrow + q * 4) = acc;
        }
    }
}

__global__ __launch_bounds__(256) void gmm_fwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ mult, const int* __restrict__ ee_ptr,
                                                             const int* __restrict__ ee_idx, const float* __restrict__ Hf,
                                                             int64_t ldh, const float* __restrict__ attr, int dim,
                                                             const float* __restrict__ mu, const float* __restrict__ sigma,
                                                             const float* __restrict__ R, int64_t ldr,
                                                             const float* __restrict__ bias, float* w, float* __restrict__ Y,
                                                             int64_t ldy, int n_rows, int K, int C) {
    GMM_TABLES
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* yrow = Y + (int64_t)row * ldy;
    float deg = 0.f;
    for (int e = e0; e < e1; ++e) deg += mult[e];
    for (int e = e0; e < e1; ++e) entry_weights(ee_ptr, ee_idx, attr, s_mu, s_inv, K, dim, e, deg, w + (int64_t)e * K);
    for (int c = 0; c < C; ++c) {
        float acc = 0.f;
        for (int e = e0; e < e1; ++e) {
            const float* x = Hf + (int64_t)col[e] * ldh + c;
            for (int k = 0; k < K; ++k) acc = fmaf(w[(int64_t)e * K + k], x[k * C], acc);
        }
        if (R) acc += R[(int64_t)row * ldr + c];
        yrow[c] = bias ? acc + bias[c] : acc;
    }
}

// ------------------------------------------------------------------------------------------------ backward, edge side
// G_e[k] = dOut[i,:] . Hf[col e, k, :] parked in ge; then per row the sums of the dmu and dsigma terms over its entries and their
// input edges -> parts[i, 0 .. K dim) (dmu) and parts[i, K dim .. 2 K dim) (dsigma): an entry's edges in input order, the row's
// entries by a fixed xor tree per 8 in CSR order, accumulated through parts[i,:] (same lane, same address, program order).
__global__ __launch_bounds__(256) void gmm_bwd_edge_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const float* __restrict__ mult, const int* __restrict__ ee_ptr,
                                                           const int* __restrict__ ee_idx, const float* __restrict__ dOut,
                                                           int64_t lddo, const float* __restrict__ Hf, int64_t ldh,
                                                           const float* __restrict__ attr, int dim, const float* __restrict__ mu,
                                                           const float* __restrict__ sigma, float* ge, float* parts,
                                                           float* __restrict__ dattr, int n_rows, int K, int C, int lw,
                                                           int chunks_per_xcd, int n_chunks) {
    GMM_TABLES
    HEAD_CHUNK_PROLOGUE
    const int KD = K * dim;
    FOR_CHUNK_ROW_ENTRIES {
        const float* grow = dOut + (int64_t)row * lddo;
        float* prow = parts + (int64_t)row * (2 * KD);
        if (nn == 0) {
            for (int p = sl; p < 2 * KD; p += 8) prow[p] = 0.f;
            continue;
        }
        float deg = 0.f;
        for (int e = sl; e < nn; e += 8) deg += mult[rbase + e];
        deg = red_sum(deg, 8);
        mix_edge_dots(col, grow, Hf, ldh, ge, K, C, lw, hp, sub, q0, rbase, nn);
        // the sweep below reads what the sibling lanes parked: same wave, same CU's L1 -- a workgroup-scope fence
        __threadfence_block();
        // one entry per lane
#pragma unroll 1
        for (int b0 = 0; b0 < nn; b0 += 8) {
            const bool ok = b0 + sl < nn;
            const int64_t ee = rbase + min(b0 + sl, nn - 1);
            const int t0 = ee_ptr[ee], t1 = ok ? ee_ptr[ee + 1] : t0;
            const float* gp = ge + ee * K;
            for (int k = 0; k < K; ++k) {
                const float gs = gp[k] / deg;
                for (int d0 = 0; d0 < dim; d0 += 4) {
                    float pm[4], ps[4];
                    entry_param_terms(ee_idx, attr, s_mu + k * dim, s_inv + k * dim, s_sg + k * dim, dim, d0, t0, t1, gs, pm, ps);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (d0 + j < dim) {                       // (row-group uniform: every lane of the 8 takes part in the tree)
                            const float sm = red_sum(pm[j], 8), ss = red_sum(ps[j], 8);
                            const int p = k * dim + d0 + j;
                            if (sl == 0) {
                                prow[p] = b0 == 0 ? sm : prow[p] + sm;
                                prow[KD + p] = b0 == 0 ? ss : prow[KD + p] + ss;
                            }
                        }
                    }
                }
            }
            if (dattr && ok) entry_dattr(ee_idx, attr, s_mu, s_inv, K, dim, t0, t1, gp, deg, dattr);
        }
    }
}

__global__ __launch_bounds__(256) void gmm_bwd_edge_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                  const float* __restrict__ mult, const int* __restrict__ ee_ptr,
                                                                  const int* __restrict__ ee_idx, const float* __restrict__ dOut,
                                                                  int64_t lddo, const float* __restrict__ Hf, int64_t ldh,
                                                                  const float* __restrict__ attr, int dim,
                                                                  const float* __restrict__ mu, const float* __restrict__ sigma,
                                                                  float* ge, float* parts, float* __restrict__ dattr, int n_rows,
                                                                  int K, int C) {
    GMM_TABLES
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int KD = K * dim;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    const float* grow = dOut + (int64_t)row * lddo;
    float* prow = parts + (int64_t)row * (2 * KD);
    for (int p = 0; p < 2 * KD; ++p) prow[p] = 0.f;
    float deg = 0.f;
    for (int e = e0; e < e1; ++e) deg += mult[e];
    for (int e = e0; e < e1; ++e) {
        float* gp = ge + (int64_t)e * K;
        const int t0 = ee_ptr[e], t1 = ee_ptr[e + 1];
        for (int k = 0; k < K; ++k) {
            const float* x = Hf + (int64_t)col[e] * ldh + k * C;
            float t = 0.f;
            for (int c = 0; c < C; ++c) t = fmaf(grow[c], x[c], t);
            gp[k] = t;
            const float gs = t / deg;
            for (int d0 = 0; d0 < dim; d0 += 4) {
                float pm[4], ps[4];
                entry_param_terms(ee_idx, attr, s_mu + k * dim, s_inv + k * dim, s_sg + k * dim, dim, d0, t0, t1, gs, pm, ps);
                for (int j = 0; j < 4 && d0 + j < dim; ++j) {
                    prow[k * dim + d0 + j] += pm[j];
                    prow[KD + k * dim + d0 + j] += ps[j];
                }
            }
        }
        if (dattr) entry_dattr(ee_idx, attr, s_mu, s_inv, K, dim, t0, t1, gp, deg, dattr);
    }
}

// ------------------------------------------------------------------------------------------------ backward, node side
// dHf[j,k,:] = sum_{e' in row j} w[mirror e', k] dOut[col e', :] written completely, and (dR non-null) the root block's gradient
// dR[j,:] = dOut[j,:] copied into its columns of the same row buffer.
__global__ __launch_bounds__(256) void gmm_bwd_node_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const int* __restrict__ mirror, const float* __restrict__ dOut,
                                                           int64_t lddo, const float* __restrict__ w, float* __restrict__ dHf,
                                                           int64_t lddh, float* __restrict__ dR, int64_t lddr, int n_rows, int K,
                                                           int C, int lw, int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        float* orow = dHf + (int64_t)row * lddh;
        if (dR)
            for (int q = sl; q < W; q += 8)
                *reinterpret_cast<float4*>(dR + (int64_t)row * lddr + q * 4) = ld4(dOut + (int64_t)row * lddo + q * 4);
        FOR_HEAD_PASSES(K) {
            for (int q = q0; q < W; q += lw) {
                const float4 acc = mix_node_gather(col, mirror, dOut, lddo, w, K, hh, rbase, nn, q);
                if (hv) *reinterpret_cast<float4*>(orow + hh * C + q * 4) = acc;
            }
        }
    }
}

__global__ __launch_bounds__(256) void gmm_bwd_node_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                  const int* __restrict__ mirror, const float* __restrict__ dOut,
                                                                  int64_t lddo, const float* __restrict__ w,
                                                                  float* __restrict__ dHf, int64_t lddh, float* __restrict__ dR,
                                                                  int64_t lddr, int n_rows, int K, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* orow = dHf + (int64_t)row * lddh;
    if (dR)
        for (int c = 0; c < C; ++c) dR[(int64_t)row * lddr + c] = dOut[(int64_t)row * lddo + c];
    for (int k = 0; k < K; ++k) {
        for (int c = 0; c < C; ++c) {
            float acc = 0.f;
            for (int e = e0; e < e1; ++e) acc = fmaf(w[(int64_t)mirror[e] * K + k], dOut[(int64_t)col[e] * lddo + c], acc);
            orow[k * C + c] = acc;
        }
    }
}

// the attention graph WITHOUT loop handling: every input edge belongs to exactly one entry and every entry has input edges
inline bool gmm_graph_ok(const ddmp_graph* g) {
    return attn_graph_ok(g) && g->valued == DDMP_GV_VALUED && g->ee_ptr && g->ee_idx;
}
inline bool gmm_dims_ok(int K, int dim, int C) { return dim > 0 && K > 0 && (int64_t)K * dim <= kMaxKD && feast_dims_ok(K, C); }

}  // namespace

extern "C" int ddmp_gmm_fwd_f32(const ddmp_graph* g, const float* Hf, int64_t ldh, const float* attr, int dim, const float* mu,
                                const float* sigma, int K, int C, const float* R, int64_t ldr, const float* bias, float* w, float* Y,
                                int64_t ldy, ddmp_stream stream) {
    ARG_TRY(gmm_graph_ok(g) && Hf && attr && mu && sigma && w && Y && gmm_dims_ok(K, dim, C) && ldh >= (int64_t)K * C && ldy >= C &&
            (!R || ldr >= C) && Y != Hf && Y != R);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && ldh % 4 == 0 && ldy % 4 == 0 && al16(Hf) && al16(Y) && (!bias || al16(bias)) && (!R || (al16(R)
                     && ldr % 4 == 0));
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), gmm_fwd_kernel, gmm_fwd_scalar_kernel,
                            g->rowptr, g->col, g->a, g->ee_ptr, g->ee_idx, Hf, ldh, attr, dim, mu, sigma, R, ldr, bias, w, Y, ldy,
                            (int)g->n_rows, K, C);
}

extern "C" int ddmp_gmm_bwd_edge_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Hf, int64_t ldh,
                                     const float* attr, int dim, const float* mu, const float* sigma, int K, int C, float* ge,
                                     float* parts, float* dattr, ddmp_stream stream) {
    ARG_TRY(gmm_graph_ok(g) && dOut && Hf && attr && mu && sigma && ge && parts && gmm_dims_ok(K, dim, C) && lddo >= C &&
            ldh >= (int64_t)K * C && dattr != attr);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddo % 4 == 0 && ldh % 4 == 0 && al16(dOut) && al16(Hf);
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), gmm_bwd_edge_kernel,
                            gmm_bwd_edge_scalar_kernel, g->rowptr, g->col, g->a, g->ee_ptr, g->ee_idx, dOut, lddo, Hf, ldh, attr,
                            dim, mu, sigma, ge, parts, dattr, (int)g->n_rows, K, C);
}

extern "C" int ddmp_gmm_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, int K, int C, const float* w, float* dHf,
                                     int64_t lddh, float* dR, int64_t lddr, ddmp_stream stream) {
    ARG_TRY(gmm_graph_ok(g) && dOut && w && dHf && feast_dims_ok(K, C) && lddo >= C && lddh >= (int64_t)K * C && (!dR || lddr >= C) &&
            dHf != dOut && dR != dOut);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddo % 4 == 0 && lddh % 4 == 0 && al16(dOut) && al16(dHf) && (!dR || (al16(dR) && lddr % 4 ==
                     0));
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), gmm_bwd_node_kernel,
                            gmm_bwd_node_scalar_kernel, g->rowptr, g->col, g->mirror, dOut, lddo, w, dHf, lddh, dR, lddr,
                            (int)g->n_rows, K, C);
}

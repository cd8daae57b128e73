// B-spline convolution (SplineCNN's SplineConv, degree 1): every input edge t: j -> i with pseudo-coordinates
// a_t in [0,1]^dim selects S = 2^dim of the K = prod(kernel_size) weight blocks of Hf[j] = x_j . weight, viewed [K, C]:
//
//   v_d = a_t[d] (kernel_size[d] - open[d]),  f_d = v_d - floor(v_d),
//   b_{t,s} = prod_d (s_d ? f_d : 1 - f_d),   k_{t,s} = sum_d ((floor(v_d) + s_d) mod kernel_size[d]) stride[d],   s in [0, S)
//   Y[i,:]  = (1 / n_i) sum_{t -> i} sum_s b_{t,s} Hf[j_t, k_{t,s}, :]  (+ R[i,:]) (+ bias),   n_i = the input edges into i (mean) or 1
//
// over the COALESCED CSR of a valued graph built WITHOUT loop handling (flags 0); an entry's input edges come from its ee_ptr /
// ee_idx span, in input order -- exact for duplicate edges whose pseudo-coordinates differ.  Only the S selected C-wide blocks of
// a neighbour's row are touched, never its K blocks.  Nothing is stored per edge: both launches evaluate the basis from attr.
// On the row-gather layout of row_gather.h, a selected block playing the part of a head:
//   * forward: the lanes of a head pass hold hp = 8 / lw different s, summed by the fixed xor tree at the end of the row;
//   * backward, node side: row j owns dHf[j, :, :], zeroes it and adds b_{t,s} dY[i,:] / n_i into block k_{t,s} for every edge
//     j -> i (found through the mirror map) -- a read-modify-write of the row's own memory by ONE lane per address (two s may
//     select the same block when a kernel_size is 1, so the lanes of a pass divide the BLOCKS: lane group `sub` owns the blocks
//     k = sub mod hp), in program order: no atomics, bitwise reproducible;
//   * the per-entry metadata (col, the edge span, 1 / n_i, the first edge's pseudo-coordinates) is fetched by the 8 lanes of the
//     row group for 8 entries at once -- one chain of dependent loads per batch instead of one per entry -- and handed round by
//     shuffles; further edges of an entry (duplicates) are read directly.
// kernel_size, its strides and kernel_size - open are kernel arguments (SplineTab), dim is a template parameter: the basis is
// straight-line code on registers.  Block indices are a true non-negative modulo clamped into [0, kernel_size[d]): memory-safe for
// every attr value, NaN and Inf included.  Every row * stride product is int64.
#include "row_gather.h"

namespace {

constexpr int kMaxDim = 5;         // S = 2^dim <= 32

struct SplineTab {
    int ks[kMaxDim];               // kernel_size[d]
    int st[kMaxDim];               // prod_{d' < d} kernel_size[d']: the first coordinate varies fastest
    float m[kMaxDim];              // kernel_size[d] - open[d]
};

// floor(v_d) mod kernel_size[d] in [0, kernel_size[d]) and the fraction f_d of one edge (a: its DIM pseudo-coordinates)
template <int DIM>
struct Basis {
    int i0[DIM];
    float fr[DIM];
    __device__ __forceinline__ void prep(const float (&a)[DIM], const SplineTab& tab) {
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            const float v = a[d] * tab.m[d];
            const float fl = floorf(v);
            fr[d] = v - fl;
            int i = fabsf(fl) < 1e9f ? (int)fl : 0;              // (NaN / Inf / huge: any block, but one of this row)
            i %= tab.ks[d];
            if (i < 0) i += tab.ks[d];
            i0[d] = min(max(i, 0), tab.ks[d] - 1);
        }
    }
    // b_{t,s} and the block index k_{t,s} < K
    __device__ __forceinline__ void eval(int s, const SplineTab& tab, float& b, int& k) const {
        b = 1.f;
        k = 0;
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
            const bool up = (s >> d) & 1;
            b *= up ? fr[d] : 1.f - fr[d];
            int i = i0[d] + (up ? 1 : 0);
            if (i >= tab.ks[d]) i = 0;                           // (i0 + 1 == kernel_size wraps: the closed spline's seam, and the
            k += i * tab.st[d];                                  //  open spline's a == 1 with weight 0)
        }
    }
};

template <int DIM>
__device__ __forceinline__ void load_attr(const float* __restrict__ attr, int64_t t, float (&a)[DIM]) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) a[d] = attr[t * DIM + d];
}

// The metadata of up to 8 entries of a row, one entry per lane of the row group (entry b0 + sl; a lane past the row's end repeats
// the last entry with an EMPTY edge span): the neighbour, the span of input edges, and the first edge's pseudo-coordinates.
template <int DIM>
struct EntryMeta {
    int c, t0, t1;
    float inv;                     // backward only: 1 / n_{col e} (mean) or 1
    float a[DIM];
    __device__ __forceinline__ EntryMeta from(int base, int k) const {
        EntryMeta r;
        r.c = __shfl(c, base + k, 64);
        r.t0 = __shfl(t0, base + k, 64);
        r.t1 = __shfl(t1, base + k, 64);
        r.inv = __shfl(inv, base + k, 64);
#pragma unroll
        for (int d = 0; d < DIM; ++d) r.a[d] = __shfl(a[d], base + k, 64);
        return r;
    }
};

// ------------------------------------------------------------------------------------------------ forward
template <int DIM>
__global__ __launch_bounds__(256) void spline_fwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                         const int* __restrict__ ee_ptr, const int* __restrict__ ee_idx,
                                                         const float* __restrict__ Hf, int64_t ldh, const float* __restrict__ attr,
                                                         SplineTab tab, const float* __restrict__ R, int64_t ldr,
                                                         const float* __restrict__ bias, int mean, float* __restrict__ Y, int64_t ldy,
                                                         int n_rows, int C, int lw, int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    constexpr int S = 1 << DIM;
    const int W = C >> 2;
    const int gbase = lane & ~7;
    FOR_CHUNK_ROW_ENTRIES {
        float* yrow = Y + (int64_t)row * ldy;
        const float* rrow = R ? R + (int64_t)row * ldr : nullptr;
        const int n_in = nn > 0 ? ee_ptr[rbase + nn] - ee_ptr[rbase] : 0;
        const float scale = (mean && n_in > 0) ? 1.0f / (float)n_in : 1.0f;
#pragma unroll 1
        for (int qb = 0; qb < W; qb += lw) {                      // (lw < 8: exactly one trip, all 8 lanes together)
            const bool qv = qb + q0 < W;
            const int q = qv ? qb + q0 : W - 1;                   // (a lane past a ragged end re-reads the last slab, stores nothing)
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                EntryMeta<DIM> mine;
                {
                    const bool ok = b0 + sl < nn;
                    const int e = rbase + min(b0 + sl, nn - 1);
                    mine.c = col[e];
                    mine.t0 = ee_ptr[e];
                    mine.t1 = ok ? ee_ptr[e + 1] : mine.t0;
                    mine.inv = 1.f;
                    load_attr<DIM>(attr, ee_idx[mine.t0], mine.a);
                }
                const int cnt = min(kEB, nn - b0);
#pragma unroll 1
                for (int k = 0; k < cnt; ++k) {
                    const EntryMeta<DIM> en = mine.from(gbase, k);
                    const float* xrow = Hf + (int64_t)en.c * ldh + q * 4;
#pragma unroll 1
                    for (int t = en.t0; t < en.t1; ++t) {
                        Basis<DIM> bs;
                        if (t == en.t0) {
                            bs.prep(en.a, tab);
                        } else {
                            float a[DIM];
                            load_attr<DIM>(attr, ee_idx[t], a);
                            bs.prep(a, tab);
                        }
#pragma unroll 4
                        for (int sg = 0; sg < S; sg += hp) {
                            const int s = sg + sub;
                            const bool sv = s < S;
                            float b;
                            int kb;
                            bs.eval(sv ? s : S - 1, tab, b, kb);
                            const float4 x = ld4(xrow + kb * C);
                            fma4(acc, sv ? b : 0.f, x);
                        }
                    }
                }
            }
            if (lw < 8) {                                         // the 8 / lw selected blocks of this pass -> one row
                acc.x = red_heads(acc.x, lw);
                acc.y = red_heads(acc.y, lw);
                acc.z = red_heads(acc.z, lw);
                acc.w = red_heads(acc.w, lw);
            }
            acc.x *= scale, acc.y *= scale, acc.z *= scale, acc.w *= scale;
            if (rrow) {
                const float4 r = ld4(rrow + q * 4);
                acc.x += r.x, acc.y += r.y, acc.z += r.z, acc.w += r.w;
            }
            if (bias) {
                const float4 b = ld4(bias + q * 4);
                acc.x += b.x, acc.y += b.y, acc.z += b.z, acc.w += b.w;
            }
            if (qv && sub == 0) *reinterpret_cast<float4*>(yrow + q * 4) = acc;
        }
    }
}

// one thread per row: any width, any alignment.  Y[row,:] is the accumulator (same thread, same address, program order).
template <int DIM>
__global__ __launch_bounds__(256) void spline_fwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                const int* __restrict__ ee_ptr, const int* __restrict__ ee_idx,
                                                                const float* __restrict__ Hf, int64_t ldh,
                                                                const float* __restrict__ attr, SplineTab tab,
                                                                const float* __restrict__ R, int64_t ldr,
                                                                const float* __restrict__ bias, int mean, float* Y, int64_t ldy,
                                                                int n_rows, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    constexpr int S = 1 << DIM;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* yrow = Y + (int64_t)row * ldy;
    for (int c = 0; c < C; ++c) yrow[c] = 0.f;
    const int n_in = ee_ptr[e1] - ee_ptr[e0];
    const float scale = (mean && n_in > 0) ? 1.0f / (float)n_in : 1.0f;
    for (int e = e0; e < e1; ++e) {
        const float* xrow = Hf + (int64_t)col[e] * ldh;
        for (int t = ee_ptr[e]; t < ee_ptr[e + 1]; ++t) {
            float a[DIM];
            load_attr<DIM>(attr, ee_idx[t], a);
            Basis<DIM> bs;
            bs.prep(a, tab);
            for (int s = 0; s < S; ++s) {
                float b;
                int kb;
                bs.eval(s, tab, b, kb);
                const float* x = xrow + (int64_t)kb * C;
                for (int c = 0; c < C; ++c) yrow[c] = fmaf(b, x[c], yrow[c]);
            }
        }
    }
    for (int c = 0; c < C; ++c) {
        float acc = yrow[c] * scale;
        if (R) acc += R[(int64_t)row * ldr + c];
        yrow[c] = bias ? acc + bias[c] : acc;
    }
}

// ------------------------------------------------------------------------------------------------ backward, node side
// dHf[j,k,:] = sum_{t: j -> i} [sum_{s: k_{t,s} = k} b_{t,s}] dOut[i,:] / n_i, written completely (blocks no edge selects are zero),
// and (dR non-null) the root block's gradient dR[j,:] = dOut[j,:] copied into its columns of the same row buffer.  Row j's own
// entries e' enumerate the targets i = col e' (the structure is symmetric); the edges j -> i are the span of the mirrored entry.
template <int DIM>
__global__ __launch_bounds__(256) void spline_bwd_node_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              const int* __restrict__ mirror, const int* __restrict__ ee_ptr,
                                                              const int* __restrict__ ee_idx, const float* __restrict__ dOut,
                                                              int64_t lddo, const float* __restrict__ attr, SplineTab tab, int mean,
                                                              float* dHf, int64_t lddh, float* __restrict__ dR, int64_t lddr,
                                                              int n_rows, int K, int C, int lw, int chunks_per_xcd, int n_chunks) {
    HEAD_CHUNK_PROLOGUE
    constexpr int S = 1 << DIM;
    const int W = C >> 2;
    const int gbase = lane & ~7;
    bool distinct = true;
#pragma unroll
    for (int d = 0; d < DIM; ++d) distinct = distinct && tab.ks[d] >= 2;
    FOR_CHUNK_ROW_ENTRIES {
        float* orow = dHf + (int64_t)row * lddh;
        if (dR)
            for (int q = sl; q < W; q += 8)
                *reinterpret_cast<float4*>(dR + (int64_t)row * lddr + q * 4) = ld4(dOut + (int64_t)row * lddo + q * 4);
#pragma unroll 1
        for (int qb = 0; qb < W; qb += lw) {                      // (lw < 8: exactly one trip, all 8 lanes together)
            const bool qv = qb + q0 < W;
            const int q = qv ? qb + q0 : W - 1;
            // this lane's addresses: column slab q of the blocks k = sub mod hp
            if (qv)
                for (int k = sub; k < K; k += hp)
                    *reinterpret_cast<float4*>(orow + (int64_t)k * C + q * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                EntryMeta<DIM> mine;
                {
                    const bool ok = b0 + sl < nn;
                    const int e = rbase + min(b0 + sl, nn - 1);
                    const int i = col[e], me = mirror[e];
                    mine.c = i;
                    mine.t0 = ee_ptr[me];
                    mine.t1 = ok ? ee_ptr[me + 1] : mine.t0;
                    const int n_in = ee_ptr[rowptr[i + 1]] - ee_ptr[rowptr[i]];
                    mine.inv = (mean && n_in > 0) ? 1.0f / (float)n_in : 1.0f;
                    load_attr<DIM>(attr, ee_idx[mine.t0], mine.a);
                }
                const int cnt = min(kEB, nn - b0);
#pragma unroll 1
                for (int k = 0; k < cnt; ++k) {
                    const EntryMeta<DIM> en = mine.from(gbase, k);
                    float4 g = ld4(dOut + (int64_t)en.c * lddo + q * 4);
                    g.x *= en.inv, g.y *= en.inv, g.z *= en.inv, g.w *= en.inv;
#pragma unroll 1
                    for (int t = en.t0; t < en.t1; ++t) {
                        Basis<DIM> bs;
                        if (t == en.t0) {
                            bs.prep(en.a, tab);
                        } else {
                            float a[DIM];
                            load_attr<DIM>(attr, ee_idx[t], a);
                            bs.prep(a, tab);
                        }
                        if (distinct) {
                            // every kernel_size >= 2: the S blocks of one edge are S different blocks, so their loads go out
                            // together, 8 at a time (unconditional: a lane that does not own a block reads it and stores nothing)
                            constexpr int SB = S < 8 ? S : 8;
#pragma unroll 1
                            for (int s0 = 0; s0 < S; s0 += SB) {
                                float b[SB];
                                float* op[SB];
                                bool on[SB];
                                float4 v[SB];
#pragma unroll
                                for (int u = 0; u < SB; ++u) {
                                    int kb;
                                    bs.eval(s0 + u, tab, b[u], kb);
                                    on[u] = qv && (kb & (hp - 1)) == sub;
                                    op[u] = orow + (int64_t)kb * C + q * 4;
                                }
#pragma unroll
                                for (int u = 0; u < SB; ++u) v[u] = ld4(op[u]);
#pragma unroll
                                for (int u = 0; u < SB; ++u) {
                                    fma4(v[u], b[u], g);
                                    if (on[u]) *reinterpret_cast<float4*>(op[u]) = v[u];
                                }
                            }
                        } else {
#pragma unroll 1
                            for (int s = 0; s < S; ++s) {         // (in order: two s select the same block where a kernel_size is 1)
                                float b;
                                int kb;
                                bs.eval(s, tab, b, kb);
                                if (qv && (kb & (hp - 1)) == sub) {
                                    float* op = orow + (int64_t)kb * C + q * 4;
                                    float4 acc = ld4(op);
                                    fma4(acc, b, g);
                                    *reinterpret_cast<float4*>(op) = acc;
                                }
                            }
                        }
                    }
                }
            }
        }
    }
}

template <int DIM>
__global__ __launch_bounds__(256) void spline_bwd_node_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                     const int* __restrict__ mirror, const int* __restrict__ ee_ptr,
                                                                     const int* __restrict__ ee_idx, const float* __restrict__ dOut,
                                                                     int64_t lddo, const float* __restrict__ attr, SplineTab tab,
                                                                     int mean, float* dHf, int64_t lddh, float* __restrict__ dR,
                                                                     int64_t lddr, int n_rows, int K, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    constexpr int S = 1 << DIM;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* orow = dHf + (int64_t)row * lddh;
    if (dR)
        for (int c = 0; c < C; ++c) dR[(int64_t)row * lddr + c] = dOut[(int64_t)row * lddo + c];
    for (int64_t p = 0; p < (int64_t)K * C; ++p) orow[p] = 0.f;
    for (int e = e0; e < e1; ++e) {
        const int i = col[e], me = mirror[e];
        const float* grow = dOut + (int64_t)i * lddo;
        const int n_in = ee_ptr[rowptr[i + 1]] - ee_ptr[rowptr[i]];
        const float inv = (mean && n_in > 0) ? 1.0f / (float)n_in : 1.0f;
        for (int t = ee_ptr[me]; t < ee_ptr[me + 1]; ++t) {
            float a[DIM];
            load_attr<DIM>(attr, ee_idx[t], a);
            Basis<DIM> bs;
            bs.prep(a, tab);
            for (int s = 0; s < S; ++s) {
                float b;
                int kb;
                bs.eval(s, tab, b, kb);
                float* o = orow + (int64_t)kb * C;
                for (int c = 0; c < C; ++c) o[c] = fmaf(b, grow[c] * inv, o[c]);
            }
        }
    }
}

// the attention graph WITHOUT loop handling: every input edge belongs to exactly one entry and every entry has input edges
inline bool spline_graph_ok(const ddmp_graph* g) {
    return attn_graph_ok(g) && g->valued == DDMP_GV_VALUED && g->ee_ptr && g->ee_idx;
}

// kernel_size / is_open (host arrays of dim ints) -> the kernel-argument table and K; false: dim or a size out of range
inline bool spline_tab(int dim, const int32_t* kernel_size, const int32_t* is_open, int C, SplineTab& tab, int& K) {
    if (dim < 1 || dim > kMaxDim || !kernel_size || !is_open || C < 1) return false;
    int64_t k = 1;
    for (int d = 0; d < kMaxDim; ++d) {
        const int ks = d < dim ? kernel_size[d] : 1;
        if (ks < 1) return false;
        tab.ks[d] = ks;
        tab.st[d] = (int)k;
        tab.m[d] = d < dim ? (float)(ks - (is_open[d] ? 1 : 0)) : 0.f;
        k *= ks;
        if (k * C >= (1 << 24)) return false;
    }
    K = (int)k;
    return true;
}

inline bool vec_ok(const float* p, int64_t ld) { return al16(p) && ld % 4 == 0; }

#define SPLINE_DIM_SWITCH(dim, launch)                                                             \
    switch (dim) {                                                                                 \
        case 1: launch(1); break;                                                                  \
        case 2: launch(2); break;                                                                  \
        case 3: launch(3); break;                                                                  \
        case 4: launch(4); break;                                                                  \
        default: launch(5); break;                                                                 \
    }

}  // namespace

extern "C" int ddmp_spline_fwd_f32(const ddmp_graph* g, const float* Hf, int64_t ldh, const float* attr, int dim,
                                   const int32_t* kernel_size, const int32_t* is_open, int C, const float* R, int64_t ldr,
                                   const float* bias, int mean, float* Y, int64_t ldy, ddmp_stream stream) {
    SplineTab tab;
    int K = 0;
    ARG_TRY(spline_graph_ok(g) && Hf && attr && Y && spline_tab(dim, kernel_size, is_open, C, tab, K) && ldh >= (int64_t)K * C &&
            ldy >= C && (!R || ldr >= C) && Y != Hf && Y != R && Y != attr && Y != bias);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(Hf, ldh) && vec_ok(Y, ldy) && al16(bias) && (!R || vec_ok(R, ldr));
#define LAUNCH(D)                                                                                                                \
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), spline_fwd_kernel<D>,                   \
                            spline_fwd_scalar_kernel<D>, g->rowptr, g->col, g->ee_ptr, g->ee_idx, Hf, ldh, attr, tab, R, ldr, bias, \
                            mean, Y, ldy, (int)g->n_rows, C)
    SPLINE_DIM_SWITCH(dim, LAUNCH)
#undef LAUNCH
}

extern "C" int ddmp_spline_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* attr, int dim,
                                        const int32_t* kernel_size, const int32_t* is_open, int C, int mean, float* dHf,
                                        int64_t lddh, float* dR, int64_t lddr, ddmp_stream stream) {
    SplineTab tab;
    int K = 0;
    ARG_TRY(spline_graph_ok(g) && dOut && attr && dHf && spline_tab(dim, kernel_size, is_open, C, tab, K) && lddo >= C &&
            lddh >= (int64_t)K * C && (!dR || lddr >= C) && dHf != dOut && dR != dOut && dHf != attr && dR != attr && dR != dHf);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(dOut, lddo) && vec_ok(dHf, lddh) && (!dR || vec_ok(dR, lddr));
#define LAUNCH(D)                                                                                                                \
    return launch_head_rows((hipStream_t)stream, (int)g->n_rows, vec, lanes_per_head(C), spline_bwd_node_kernel<D>,              \
                            spline_bwd_node_scalar_kernel<D>, g->rowptr, g->col, g->mirror, g->ee_ptr, g->ee_idx, dOut, lddo, attr, \
                            tab, mean, dHf, lddh, dR, lddr, (int)g->n_rows, K, C)
    SPLINE_DIM_SWITCH(dim, LAUNCH)
#undef LAUNCH
}

// Crystal graph convolution (CGConv): TWO per-channel gates on every input edge t: j -> i, each a learned function
// of the edge's attributes a_t [dim],
//
//   F_t = Af[i,:] + Bf[j,:] + Ef a_t,   S_t = As[i,:] + Bs[j,:] + Es a_t,
//   Y[i,:] = init_i + w_i sum_{t -> i} sigmoid(F_t) (.) softplus(S_t),   init_i = root[i,:],   w_i = 1 (add) | 1 / n_in(i) (mean)
//
// over the COALESCED CSR of the attention graph built without loop handling.  dim > 0: an entry's input edges come from its ee_ptr /
// ee_idx span, in input order -- exact for duplicate edges whose attributes differ.  dim == 0: no attributes, an entry counts with
// its multiplicity and the ee tables are not touched.  Nothing is stored per edge: the backward launches RECOMPUTE both gates from
// the rows the forward read.  On the row-gather layout without heads (row_gather.h), as rgate.hip:
//   * the three launches are ONE sweep (cgate_kernel) over two of the row's own blocks (R1, R2) and two gathered blocks (X1, X2):
//       forward    R = Af, As   X = Bf, Bs                 Y   += m f s
//       row side   R = Af, As   X = Bf, Bs   g = m dOut[i]   dAf += dF = g s f (1 - f),  dAs += dS = g f sigmoid(S),
//                                                           P[i] += [dF (x) a_t | dS (x) a_t]
//       node side  R = Bf, Bs   X = Af, As   g = m dOut[i]   dBf += dF,  dBs += dS          (i = col e', gathered: a third stream)
//     with m = w_i (x the multiplicity when dim == 0) of the edge's TARGET.  The node side walks row j's own entries e', which
//     enumerate the targets i = col e' that j feeds -- the structure is symmetric -- and takes the edges j -> i (or their count)
//     from the mirrored entry;
//   * the per-entry metadata (col, the edge span, m, the first edge's attributes) is fetched by the 8 lanes of the row group for
//     up to 8 entries at once -- one chain of dependent loads per batch -- and handed round by shuffles, as spline.hip does;
//     further edges of an entry (duplicates) are read directly;
//   * Ef, Es are passed TRANSPOSED [dim, C]: a lane's four channels of one attribute coordinate are one float4, and the 2 dim
//     float4 of a column slab stay in registers over the batch;
//   * the loads of a batch are unconditional: a shorter row re-reads its last entry, masked by m = 0 (dim == 0) or an empty edge
//     span (dim > 0); the entries per batch (8, 4 or 2) follow the register budget of the mode and dim;
//   * a row longer than one batch accumulates through its own output rows (same lane, same address, program order).
// No LDS, no barrier, no atomics, every sum in a fixed order.  dim is a template parameter in [0, kMaxDim].
#include "row_gather.h"

namespace {

constexpr int kMaxDim = 8;         // CG_MAX_DIM of ops.py

enum { kFwd = 0, kRow = 1, kNode = 2 };

struct CgArgs {
    const int* rowptr;
    const int* col;
    const int* mirror;
    const float* mult;
    const int* ee_ptr;             // dim > 0 only
    const int* ee_idx;
    const float* attr;             // [input edges, dim]
    const float* R1;               // the row's own blocks: Af, As (kFwd, kRow) | Bf, Bs (kNode)
    int64_t ldr1;
    const float* R2;
    int64_t ldr2;
    const float* X1;               // the gathered blocks: Bf, Bs (kFwd, kRow) | Af, As (kNode)
    int64_t ldx1;
    const float* X2;
    int64_t ldx2;
    const float* G;                // kFwd: root (nullable) | dOut: the row's own (kRow), gathered (kNode)
    int64_t ldg;
    const float* Ef;               // [dim, C]
    const float* Es;
    float* O1;                     // Y | dAf | dBf
    int64_t ldo1;
    float* O2;                     // - | dAs | dBs
    int64_t ldo2;
    float* P;                      // kRow, nullable: [n, 2, dim, C]
    float* dS;                     // kNode, nullable: dS[row,:] = dOut[row,:]
    int64_t ldds;
    int mean, n_rows, C;
};

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 scale4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// 1 / (1 + exp(-x)), rgate.hip's: finite for every finite x, the hardware exponent's rounding leaves |x| 2^-24 relative
__device__ __forceinline__ float sigmoidf(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

// softplus(x) = max(x, 0) + log1p(u), u = exp(-|x|) in [0, 1], and (kGrad) its derivative sigmoid(x) from the same u.
// log1p(u) = 2 atanh(z), z = u / (2 + u) <= 1/3, as the odd series 2 z (1 + t/3 + ... + t^7/15), t = z^2 <= 1/9 (the first
// dropped term is below 1.4e-9 of the sum): relative accuracy down to u = 0, where log(1 + u) would return 0.  No branch; u
// underflows to 0 for |x| > 87.3 and the result is max(x, 0); no NaN and no Inf for any finite x.
template <bool kGrad>
__device__ __forceinline__ float softplusf(float x, float& dsp) {
    const float u = __expf(-fabsf(x));
    const float z = u * __builtin_amdgcn_rcpf(2.f + u);
    const float t = z * z;
    float p = 1.f / 15.f;
    p = fmaf(p, t, 1.f / 13.f);
    p = fmaf(p, t, 1.f / 11.f);
    p = fmaf(p, t, 1.f / 9.f);
    p = fmaf(p, t, 1.f / 7.f);
    p = fmaf(p, t, 1.f / 5.f);
    p = fmaf(p, t, 1.f / 3.f);
    p = fmaf(p, t, 1.f);
    if (kGrad) dsp = (x >= 0.f ? 1.f : u) * __builtin_amdgcn_rcpf(1.f + u);
    return fmaxf(x, 0.f) + 2.f * z * p;
}

// one channel of one edge with gate arguments F, S.  kFwd: o1 += g f s (g = m).  Backward (g = m dOut): dF = g s f (1 - f),
// dS = g f sigmoid(S); o1 += dF, o2 += dS.
template <int kMode>
__device__ __forceinline__ void edge1(float F, float S, float g, float& o1, float& o2, float& dF, float& dS) {
    const float f = sigmoidf(F);
    float dsp = 0.f;
    const float s = softplusf<kMode != kFwd>(S, dsp);
    if (kMode == kFwd) {
        o1 = fmaf(g * f, s, o1);
    } else {
        dF = g * s * (f * (1.f - f));
        dS = g * f * dsp;
        o1 += dF;
        o2 += dS;
    }
}
template <int kMode>
__device__ __forceinline__ void edge4(float4 F, float4 S, float4 g, float4& o1, float4& o2, float4& dF, float4& dS) {
    edge1<kMode>(F.x, S.x, g.x, o1.x, o2.x, dF.x, dS.x);
    edge1<kMode>(F.y, S.y, g.y, o1.y, o2.y, dF.y, dS.y);
    edge1<kMode>(F.z, S.z, g.z, o1.z, o2.z, dF.z, dS.z);
    edge1<kMode>(F.w, S.w, g.w, o1.w, o2.w, dF.w, dS.w);
}

template <int DIM>
__device__ __forceinline__ void load_attr(const float* __restrict__ attr, int64_t t, float* a) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) a[d] = attr[t * DIM + d];
}

// w_i: 1 (add), or 1 / n_in(i) (mean): the input edges into i -- the width of row i's edge span (dim > 0), or the sum of its
// entries' multiplicities (dim == 0: integers in float32, exact below 2^24).  1 for a row without edges.
template <int DIM>
__device__ __forceinline__ float row_weight(const CgArgs& p, int i) {
    if (!p.mean) return 1.f;
    const int e0 = p.rowptr[i], e1 = p.rowptr[i + 1];
    float n = 0.f;
    if (DIM > 0) {
        n = (float)(p.ee_ptr[e1] - p.ee_ptr[e0]);
    } else {
        for (int e = e0; e < e1; ++e) n += p.mult[e];
    }
    return n > 0.f ? 1.0f / n : 1.0f;
}

// The metadata of up to 8 entries of a row, one entry per lane of the row group (entry b0 + sl; a lane past the batch or the row's
// end repeats the row's last entry, masked: m = 0 when DIM == 0, an EMPTY edge span otherwise).
template <int DIM>
struct EntryMeta {
    int c, t0, t1;                 // the neighbour; DIM > 0: the span of input edges
    float m;                       // w of the edge's target (x the multiplicity when DIM == 0)
    float a[DIM > 0 ? DIM : 1];    // DIM > 0: the first edge's attributes
};

// Run `batch` with the entry count of this batch as a compile-time constant <= EB: the longest row's count among the wave's active
// rows (wave-uniform, from ballots) -- ROW_BATCH_SWITCH for a batch of EB entries.
template <int N, int EB, class Batch>
__device__ __forceinline__ void batch_dispatch(int ne_w, Batch& batch) {
    if constexpr (N >= EB) {
        batch(std::integral_constant<int, EB>());
    } else {
        if (ne_w <= N)
            batch(std::integral_constant<int, N>());
        else
            batch_dispatch<N + 1, EB>(ne_w, batch);
    }
}
template <int EB, class Batch>
__device__ __forceinline__ void batch_switch(int b0, int nn, Batch& batch) {
    int ne_w = 0;
#pragma unroll
    for (int k = 0; k < EB; ++k) ne_w += __any(b0 + k < nn) ? 1 : 0;
    batch_dispatch<1, EB>(ne_w, batch);
}

// entries per batch: the gathered float4 in flight (2 per entry, 3 on the node side) next to the 2 DIM float4 of Ef / Es and, on
// the row side, the 2 DIM float4 of the partials -- chosen so that no instantiation needs scratch and all but the row side at
// dim 6 .. 8 (258 .. 308 registers, the surplus in AGPRs: one wave per SIMD) stay below 256 registers
constexpr int entries_per_batch(int mode, int dim) {
    return mode == kFwd ? (dim <= 4 ? 8 : 4) : mode == kRow ? (dim <= 2 ? 8 : dim <= 4 ? 4 : 2) : (dim <= 4 ? 4 : 2);
}

template <int kMode, int DIM, int EB>
__global__ __launch_bounds__(256) void cgate_kernel(const CgArgs p, int chunks_per_xcd, int n_chunks) {
    static_assert(EB >= 1 && EB <= 8, "one entry per lane of the row group");
    const int n_rows = p.n_rows;
    const int* __restrict__ rowptr = p.rowptr;
    ROW_CHUNK_PROLOGUE
    constexpr int D1 = DIM > 0 ? DIM : 1;
    const int C = p.C, W = C >> 2;
    const int gbase = lane & ~7;
    const bool parts = kMode == kRow && DIM > 0 && p.P != nullptr;
    FOR_CHUNK_ROW_ENTRIES {
        const float* r1 = p.R1 + (int64_t)row * p.ldr1;
        const float* r2 = p.R2 + (int64_t)row * p.ldr2;
        const float* grow = (kMode != kNode && p.G) ? p.G + (int64_t)row * p.ldg : nullptr;   // the root | the row's dOut
        float* o1 = p.O1 + (int64_t)row * p.ldo1;
        float* o2 = kMode != kFwd ? p.O2 + (int64_t)row * p.ldo2 : nullptr;
        float* prow = parts ? p.P + (int64_t)row * (2 * DIM) * C : nullptr;
        if (kMode == kNode && p.dS)
            for (int q = sl; q < W; q += 8) st4(p.dS + (int64_t)row * p.ldds + q * 4, ld4(p.G + (int64_t)row * p.ldg + q * 4));
        // what the sums start from: the forward's root block, zeros in the backward
        auto init = [&](int q) { return (kMode == kFwd && grow) ? ld4(grow + q * 4) : zero4(); };
        if (nn == 0) {
            for (int q = sl; q < W; q += 8) {
                st4(o1 + q * 4, init(q));
                if (kMode != kFwd) st4(o2 + q * 4, zero4());
                if (parts)
                    for (int d = 0; d < 2 * DIM; ++d) st4(prow + d * C + q * 4, zero4());
            }
            continue;
        }
        const float wrow = kMode == kNode ? 1.f : row_weight<DIM>(p, row);
#pragma unroll 1
        for (int b0 = 0; b0 < nn; b0 += EB) {
            EntryMeta<DIM> mine;
            {
                const bool ok = sl < EB && b0 + sl < nn;
                const int e = rbase + min(b0 + sl, nn - 1);
                const int c = p.col[e];
                const int se = kMode == kNode ? p.mirror[e] : e;   // the entry of the edges c -> row | row -> c
                mine.c = c;
                mine.t0 = mine.t1 = 0;
                mine.a[0] = 0.f;
                float m = kMode == kNode ? row_weight<DIM>(p, c) : wrow;
                if (DIM == 0) {
                    m = ok ? m * p.mult[se] : 0.f;
                } else {
                    mine.t0 = p.ee_ptr[se];
                    mine.t1 = ok ? p.ee_ptr[se + 1] : mine.t0;
                    load_attr<DIM>(p.attr, p.ee_idx[mine.t0], mine.a);
                }
                mine.m = m;
            }
            auto batch = [&](auto ne_tag) {
                constexpr int NE = decltype(ne_tag)::value;
#pragma unroll 1
                for (int qb = 0; qb < W; qb += 8) {               // (the 8 lanes stay together: they hand the metadata round)
                    const bool qv = qb + sl < W;
                    const int q = qv ? qb + sl : W - 1;           // (a lane past a ragged end re-reads the last slab, stores nothing)
                    const float4 a1 = ld4(r1 + q * 4), a2 = ld4(r2 + q * 4);
                    const float4 gown = kMode == kRow ? ld4(grow + q * 4) : zero4();
                    float4 ef[D1], es[D1], pf[D1], ps[D1];
#pragma unroll
                    for (int d = 0; d < D1; ++d) {
                        ef[d] = DIM > 0 ? ld4(p.Ef + d * C + q * 4) : zero4();
                        es[d] = DIM > 0 ? ld4(p.Es + d * C + q * 4) : zero4();
                        pf[d] = (parts && b0 > 0) ? ld4(prow + d * C + q * 4) : zero4();
                        ps[d] = (parts && b0 > 0) ? ld4(prow + (DIM + d) * C + q * 4) : zero4();
                    }
                    float4 acc1 = b0 == 0 ? init(q) : ld4(o1 + q * 4);
                    float4 acc2 = (kMode == kFwd || b0 == 0) ? zero4() : ld4(o2 + q * 4);
                    float4 x1[NE], x2[NE], x3[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int64_t c = __shfl(mine.c, gbase + k, 64);
                        x1[k] = ld4(p.X1 + c * p.ldx1 + q * 4);
                        x2[k] = ld4(p.X2 + c * p.ldx2 + q * 4);
                        x3[k] = kMode == kNode ? ld4(p.G + c * p.ldg + q * 4) : zero4();
                    }
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const float m = __shfl(mine.m, gbase + k, 64);
                        const float4 g = kMode == kFwd ? make_float4(m, m, m, m) : scale4(kMode == kRow ? gown : x3[k], m);
                        const float4 F0 = add4(a1, x1[k]), S0 = add4(a2, x2[k]);
                        float4 dF = zero4(), dS = zero4();
                        if (DIM == 0) {
                            edge4<kMode>(F0, S0, g, acc1, acc2, dF, dS);
                        } else {
                            const int t0 = __shfl(mine.t0, gbase + k, 64), t1 = __shfl(mine.t1, gbase + k, 64);
                            float a[D1];
#pragma unroll
                            for (int d = 0; d < D1; ++d) a[d] = __shfl(mine.a[d], gbase + k, 64);
#pragma unroll 1
                            for (int t = t0; t < t1; ++t) {
                                if (t != t0) load_attr<DIM>(p.attr, p.ee_idx[t], a);
                                float4 F = F0, S = S0;
#pragma unroll
                                for (int d = 0; d < D1; ++d) {
                                    fma4(F, a[d], ef[d]);
                                    fma4(S, a[d], es[d]);
                                }
                                edge4<kMode>(F, S, g, acc1, acc2, dF, dS);
                                if (kMode == kRow) {
#pragma unroll
                                    for (int d = 0; d < D1; ++d) {
                                        fma4(pf[d], a[d], dF);
                                        fma4(ps[d], a[d], dS);
                                    }
                                }
                            }
                        }
                    }
                    if (qv) {
                        st4(o1 + q * 4, acc1);
                        if (kMode != kFwd) st4(o2 + q * 4, acc2);
                        if (parts) {
#pragma unroll
                            for (int d = 0; d < D1; ++d) {
                                st4(prow + d * C + q * 4, pf[d]);
                                st4(prow + (DIM + d) * C + q * 4, ps[d]);
                            }
                        }
                    }
                }
            };
            batch_switch<EB>(b0, nn, batch);
        }
    }
}

// one thread per row: any width, any alignment
template <int kMode, int DIM>
__global__ __launch_bounds__(256) void cgate_scalar_kernel(const CgArgs p) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= p.n_rows) return;
    constexpr int D1 = DIM > 0 ? DIM : 1;
    const int C = p.C;
    const int e0 = p.rowptr[row], e1 = p.rowptr[row + 1];
    const bool parts = kMode == kRow && DIM > 0 && p.P != nullptr;
    const float wrow = kMode == kNode ? 1.f : row_weight<DIM>(p, row);
    for (int c = 0; c < C; ++c) {
        if (kMode == kNode && p.dS) p.dS[(int64_t)row * p.ldds + c] = p.G[(int64_t)row * p.ldg + c];
        const float a1 = p.R1[(int64_t)row * p.ldr1 + c], a2 = p.R2[(int64_t)row * p.ldr2 + c];
        const float gown = kMode == kRow ? p.G[(int64_t)row * p.ldg + c] : 0.f;
        float acc1 = (kMode == kFwd && p.G) ? p.G[(int64_t)row * p.ldg + c] : 0.f, acc2 = 0.f;
        float pf[D1], ps[D1];
        for (int d = 0; d < D1; ++d) pf[d] = ps[d] = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int64_t j = p.col[e];
            const int se = kMode == kNode ? p.mirror[e] : e;
            float m = kMode == kNode ? row_weight<DIM>(p, (int)j) : wrow;
            if (DIM == 0) m *= p.mult[se];
            const float g = kMode == kFwd ? m : m * (kMode == kRow ? gown : p.G[j * p.ldg + c]);
            const float F0 = a1 + p.X1[j * p.ldx1 + c], S0 = a2 + p.X2[j * p.ldx2 + c];
            float dF = 0.f, dS = 0.f;
            if (DIM == 0) {
                edge1<kMode>(F0, S0, g, acc1, acc2, dF, dS);
            } else {
                for (int t = p.ee_ptr[se]; t < p.ee_ptr[se + 1]; ++t) {
                    float a[D1];
                    load_attr<DIM>(p.attr, p.ee_idx[t], a);
                    float F = F0, S = S0;
                    for (int d = 0; d < D1; ++d) {
                        F = fmaf(a[d], p.Ef[d * C + c], F);
                        S = fmaf(a[d], p.Es[d * C + c], S);
                    }
                    edge1<kMode>(F, S, g, acc1, acc2, dF, dS);
                    if (kMode == kRow)
                        for (int d = 0; d < D1; ++d) {
                            pf[d] = fmaf(a[d], dF, pf[d]);
                            ps[d] = fmaf(a[d], dS, ps[d]);
                        }
                }
            }
        }
        p.O1[(int64_t)row * p.ldo1 + c] = acc1;
        if (kMode != kFwd) p.O2[(int64_t)row * p.ldo2 + c] = acc2;
        if (parts)
            for (int d = 0; d < DIM; ++d) {
                p.P[((int64_t)row * 2 * DIM + d) * C + c] = pf[d];
                p.P[((int64_t)row * 2 * DIM + DIM + d) * C + c] = ps[d];
            }
    }
}

inline bool cgate_dims_ok(int C, int dim) { return C > 0 && C < (1 << 20) && dim >= 0 && dim <= kMaxDim; }

// dim == 0: the attention graph and no attributes; dim > 0: the graph WITHOUT loop handling (every input edge belongs to exactly
// one entry and every entry has input edges) with its ee tables, the attributes and both edge weights
inline bool cgate_graph_ok(const ddmp_graph* g, int dim, const float* attr, const float* Ef, const float* Es) {
    if (!attn_graph_ok(g)) return false;
    if (dim == 0) return !attr && !Ef && !Es;
    return g->valued == DDMP_GV_VALUED && g->ee_ptr && g->ee_idx && attr && Ef && Es;
}

template <int kMode, int DIM>
int cgate_launch_dim(const ddmp_graph* g, const CgArgs& a, bool vec, ddmp_stream stream) {
    return launch_rows((hipStream_t)stream, (int)g->n_rows, vec, cgate_kernel<kMode, DIM, entries_per_batch(kMode, DIM)>,
                       cgate_scalar_kernel<kMode, DIM>, a);
}

template <int kMode>
int cgate_launch(const ddmp_graph* g, CgArgs a, int dim, ddmp_stream stream) {
    if (g->n_rows == 0) return DDMP_OK;
    a.rowptr = g->rowptr, a.col = g->col, a.mirror = g->mirror, a.mult = g->a;
    a.ee_ptr = dim > 0 ? g->ee_ptr : nullptr, a.ee_idx = dim > 0 ? g->ee_idx : nullptr;
    a.n_rows = (int)g->n_rows;
    const bool vec = a.C % 4 == 0 && vec_ok(a.R1, a.ldr1) && vec_ok(a.R2, a.ldr2) && vec_ok(a.X1, a.ldx1) && vec_ok(a.X2, a.ldx2) &&
                     (!a.G || vec_ok(a.G, a.ldg)) && al16(a.Ef) && al16(a.Es) && vec_ok(a.O1, a.ldo1) &&
                     (!a.O2 || vec_ok(a.O2, a.ldo2)) && al16(a.P) && (!a.dS || vec_ok(a.dS, a.ldds));
    switch (dim) {
        case 0: return cgate_launch_dim<kMode, 0>(g, a, vec, stream);
        case 1: return cgate_launch_dim<kMode, 1>(g, a, vec, stream);
        case 2: return cgate_launch_dim<kMode, 2>(g, a, vec, stream);
        case 3: return cgate_launch_dim<kMode, 3>(g, a, vec, stream);
        case 4: return cgate_launch_dim<kMode, 4>(g, a, vec, stream);
        case 5: return cgate_launch_dim<kMode, 5>(g, a, vec, stream);
        case 6: return cgate_launch_dim<kMode, 6>(g, a, vec, stream);
        case 7: return cgate_launch_dim<kMode, 7>(g, a, vec, stream);
        default: return cgate_launch_dim<kMode, 8>(g, a, vec, stream);
    }
}

}  // namespace

extern "C" int ddmp_cgate_fwd_f32(const ddmp_graph* g, const float* Af, int64_t ldaf, const float* As, int64_t ldas, const float* Bf,
                                  int64_t ldbf, const float* Bs, int64_t ldbs, int C, const float* attr, int dim, const float* EfT,
                                  const float* EsT, const float* root, int64_t ldr, int mean, float* Y, int64_t ldy,
                                  ddmp_stream stream) {
    ARG_TRY(cgate_dims_ok(C, dim) && cgate_graph_ok(g, dim, attr, EfT, EsT) && Af && As && Bf && Bs && Y && ldaf >= C && ldas >= C &&
            ldbf >= C && ldbs >= C && ldy >= C && (!root || ldr >= C));
    const float* ins[8] = {Af, As, Bf, Bs, attr, EfT, EsT, root};
    for (int i = 0; i < 8; ++i) ARG_TRY(Y != ins[i]);
    CgArgs a = {};
    a.attr = attr, a.R1 = Af, a.ldr1 = ldaf, a.R2 = As, a.ldr2 = ldas, a.X1 = Bf, a.ldx1 = ldbf, a.X2 = Bs, a.ldx2 = ldbs;
    a.G = root, a.ldg = ldr, a.Ef = EfT, a.Es = EsT, a.O1 = Y, a.ldo1 = ldy, a.mean = mean, a.C = C;
    return cgate_launch<kFwd>(g, a, dim, stream);
}

extern "C" int ddmp_cgate_bwd_row_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Af, int64_t ldaf,
                                      const float* As, int64_t ldas, const float* Bf, int64_t ldbf, const float* Bs, int64_t ldbs,
                                      int C, const float* attr, int dim, const float* EfT, const float* EsT, int mean, float* dAf,
                                      int64_t lddaf, float* dAs, int64_t lddas, float* P, ddmp_stream stream) {
    ARG_TRY(cgate_dims_ok(C, dim) && cgate_graph_ok(g, dim, attr, EfT, EsT) && dOut && Af && As && Bf && Bs && dAf && dAs &&
            lddo >= C && ldaf >= C && ldas >= C && ldbf >= C && ldbs >= C && lddaf >= C && lddas >= C && (dim > 0 || !P));
    const float* ins[8] = {dOut, Af, As, Bf, Bs, attr, EfT, EsT};
    float* outs[3] = {dAf, dAs, P};
    for (int o = 0; o < 3; ++o) {
        if (!outs[o]) continue;
        for (int i = 0; i < 8; ++i) ARG_TRY(outs[o] != ins[i]);
        for (int q = 0; q < o; ++q) ARG_TRY(outs[o] != outs[q]);
    }
    CgArgs a = {};
    a.attr = attr, a.R1 = Af, a.ldr1 = ldaf, a.R2 = As, a.ldr2 = ldas, a.X1 = Bf, a.ldx1 = ldbf, a.X2 = Bs, a.ldx2 = ldbs;
    a.G = dOut, a.ldg = lddo, a.Ef = EfT, a.Es = EsT, a.O1 = dAf, a.ldo1 = lddaf, a.O2 = dAs, a.ldo2 = lddas, a.P = P;
    a.mean = mean, a.C = C;
    return cgate_launch<kRow>(g, a, dim, stream);
}

extern "C" int ddmp_cgate_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Af, int64_t ldaf,
                                       const float* As, int64_t ldas, const float* Bf, int64_t ldbf, const float* Bs, int64_t ldbs,
                                       int C, const float* attr, int dim, const float* EfT, const float* EsT, int mean, float* dBf,
                                       int64_t lddbf, float* dBs, int64_t lddbs, float* dS, int64_t ldds, ddmp_stream stream) {
    ARG_TRY(cgate_dims_ok(C, dim) && cgate_graph_ok(g, dim, attr, EfT, EsT) && dOut && Af && As && Bf && Bs && dBf && dBs &&
            lddo >= C && ldaf >= C && ldas >= C && ldbf >= C && ldbs >= C && lddbf >= C && lddbs >= C && (!dS || ldds >= C));
    const float* ins[8] = {dOut, Af, As, Bf, Bs, attr, EfT, EsT};
    float* outs[3] = {dBf, dBs, dS};
    for (int o = 0; o < 3; ++o) {
        if (!outs[o]) continue;
        for (int i = 0; i < 8; ++i) ARG_TRY(outs[o] != ins[i]);
        for (int q = 0; q < o; ++q) ARG_TRY(outs[o] != outs[q]);
    }
    CgArgs a = {};
    a.attr = attr, a.R1 = Bf, a.ldr1 = ldbf, a.R2 = Bs, a.ldr2 = ldbs, a.X1 = Af, a.ldx1 = ldaf, a.X2 = As, a.ldx2 = ldas;
    a.G = dOut, a.ldg = lddo, a.Ef = EfT, a.Es = EsT, a.O1 = dBf, a.ldo1 = lddbf, a.O2 = dBs, a.ldo2 = lddbs, a.dS = dS, a.ldds = ldds;
    a.mean = mean, a.C = C;
    return cgate_launch<kNode>(g, a, dim, stream);
}

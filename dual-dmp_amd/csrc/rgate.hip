// Residual gated graph convolution (ResGatedGraphConv): a PER-CHANNEL sigmoid gate on every edge,
//
//   Y[i,:] = init_i + sum_{e in row i} a_e sigma(K[i,:] + Q[col e,:]) (.) V[col e,:],   init_i = skip[i,:] + bias
//
// over the COALESCED CSR of the attention graph (a_e: the multiplicity of the entry, as in gat.hip).  The edge weight is as wide
// as the features, so nothing is parked per entry: the backward launches RECOMPUTE the gate from the rows the forward read.  On
// the row-gather layout without heads (row_gather.h):
//   * the three launches are ONE sweep (rgate_kernel) over two of the row's own blocks (A, B) and two gathered blocks (G1, G2),
//     with g = sigma(A[row] + G1[col e]) in all three:
//       forward    A = K,  B = the init,  G1 = Q,  G2 = V      Y  += a g G2
//       row side   A = K,  B = dOut,      G1 = Q,  G2 = V      dK += a g (1 - g) B G2
//       node side  A = Q,  B = V,         G1 = K,  G2 = dOut   dV += a g G2,  dQ += a g (1 - g) B G2,   a = mult[mirror e]
//     (the node side walks row j's own entries e', which enumerate the targets i = col e' that j feeds -- the structure is
//     symmetric -- and takes the multiplicity of the edge j -> i from the mirrored entry);
//   * the q loop (the row's float4 slabs, 8 lanes at a time) runs INSIDE a batch of kEB entries with two float4 per entry in
//     flight: the budget of tconv_bwd_node_kernel;
//   * the loads of a batch are unconditional: a shorter row re-reads its last entry and masks it with a zero factor;
//   * a row longer than one batch accumulates through its own output rows (same lane, same address, program order).
// No LDS, no barrier, no atomics, every sum in a fixed order.
#include "row_gather.h"

namespace {

enum { kFwd = 0, kRow = 1, kNode = 2 };

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// 1 / (1 + exp(-x)): exp overflows to +inf for x < -88.7 and the reciprocal of +inf is 0, exp underflows to 0 for large x and the
// gate is 1 -- no NaN and no Inf for any finite x.  The hardware exp2 / reciprocal: the exponent's rounding leaves a relative
// error of |x| 2^-24 in exp(-x), which is below 1e-6 wherever the gate is not saturated.
__device__ __forceinline__ float sigmoidf(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }

// one channel of one entry: t1 = f g x2 (forward, dV), t2 = t1 (1 - g) b (dK, dQ)
template <int kMode>
__device__ __forceinline__ void gate1(float a, float b, float x1, float x2, float f, float& o1, float& o2) {
    const float g = sigmoidf(a + x1);
    const float t = f * g * x2;
    if (kMode == kFwd) {
        o1 += t;
    } else {
        o1 = fmaf(t * (1.f - g), b, o1);
        if (kMode == kNode) o2 += t;
    }
}
template <int kMode>
__device__ __forceinline__ void gate4(float4 a, float4 b, float4 x1, float4 x2, float f, float4& o1, float4& o2) {
    gate1<kMode>(a.x, b.x, x1.x, x2.x, f, o1.x, o2.x);
    gate1<kMode>(a.y, b.y, x1.y, x2.y, f, o1.y, o2.y);
    gate1<kMode>(a.z, b.z, x1.z, x2.z, f, o1.z, o2.z);
    gate1<kMode>(a.w, b.w, x1.w, x2.w, f, o1.w, o2.w);
}

// A, B: the row's own blocks (kFwd: B = the skip block, nullable, and `bias` [C], nullable); G1, G2: the gathered blocks;
// O1 (and kNode: O2) the accumulated outputs, written completely; kNode, dS non-null: dS[row,:] = G2[row,:] (= dOut).
template <int kMode>
__global__ __launch_bounds__(256) void rgate_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                    const int* __restrict__ mirror, const float* __restrict__ mult,
                                                    const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                    int64_t ldb, const float* __restrict__ bias, const float* __restrict__ G1,
                                                    int64_t ld1, const float* __restrict__ G2, int64_t ld2, float* O1, int64_t ldo1,
                                                    float* O2, int64_t ldo2, float* dS, int64_t ldds, int n_rows, int C,
                                                    int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        const float* arow = A + (int64_t)row * lda;
        const float* brow = B ? B + (int64_t)row * ldb : nullptr;
        float* o1 = O1 + (int64_t)row * ldo1;
        float* o2 = kMode == kNode ? O2 + (int64_t)row * ldo2 : nullptr;
        // what the sums start from: the forward's skip + bias, zeros in the backward
        auto init = [&](int q) {
            if (kMode != kFwd) return zero4();
            const float4 s = brow ? ld4(brow + q * 4) : zero4();
            const float4 b = bias ? ld4(bias + q * 4) : zero4();
            return make_float4(s.x + b.x, s.y + b.y, s.z + b.z, s.w + b.w);
        };
        if (kMode == kNode && dS)
            for (int q = sl; q < W; q += 8)
                *reinterpret_cast<float4*>(dS + (int64_t)row * ldds + q * 4) = ld4(G2 + (int64_t)row * ld2 + q * 4);
        if (nn == 0) {
            for (int q = sl; q < W; q += 8) {
                *reinterpret_cast<float4*>(o1 + q * 4) = init(q);
                if (kMode == kNode) *reinterpret_cast<float4*>(o2 + q * 4) = zero4();
            }
            continue;
        }
#pragma unroll 1
        for (int b0 = 0; b0 < nn; b0 += kEB) {
            auto batch = [&](auto ne_tag) {
                constexpr int NE = decltype(ne_tag)::value;
                const float* p1[NE];
                const float* p2[NE];
                float f[NE];
#pragma unroll
                for (int k = 0; k < NE; ++k) {
                    const int e = rbase + min(b0 + k, nn - 1);
                    const int64_t c = col[e];
                    p1[k] = G1 + c * ld1;
                    p2[k] = G2 + c * ld2;
                    const float v = mult[kMode == kNode ? mirror[e] : e];
                    f[k] = b0 + k < nn ? v : 0.f;
                }
                for (int q = sl; q < W; q += 8) {
                    const float4 a = ld4(arow + q * 4);
                    const float4 b = kMode == kFwd ? zero4() : ld4(brow + q * 4);
                    float4 acc1 = b0 == 0 ? init(q) : ld4(o1 + q * 4);
                    float4 acc2 = (kMode != kNode || b0 == 0) ? zero4() : ld4(o2 + q * 4);
                    float4 x1[NE], x2[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        x1[k] = ld4(p1[k] + q * 4);
                        x2[k] = ld4(p2[k] + q * 4);
                    }
#pragma unroll
                    for (int k = 0; k < NE; ++k) gate4<kMode>(a, b, x1[k], x2[k], f[k], acc1, acc2);
                    *reinterpret_cast<float4*>(o1 + q * 4) = acc1;
                    if (kMode == kNode) *reinterpret_cast<float4*>(o2 + q * 4) = acc2;
                }
            };
            ROW_BATCH_SWITCH(b0, nn, batch)
        }
    }
}

// one thread per row: any width, any alignment
template <int kMode>
__global__ __launch_bounds__(256) void rgate_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const int* __restrict__ mirror, const float* __restrict__ mult,
                                                           const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                           int64_t ldb, const float* __restrict__ bias,
                                                           const float* __restrict__ G1, int64_t ld1, const float* __restrict__ G2,
                                                           int64_t ld2, float* __restrict__ O1, int64_t ldo1,
                                                           float* __restrict__ O2, int64_t ldo2, float* __restrict__ dS,
                                                           int64_t ldds, int n_rows, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int c = 0; c < C; ++c) {
        if (kMode == kNode && dS) dS[(int64_t)row * ldds + c] = G2[(int64_t)row * ld2 + c];
        const float a = A[(int64_t)row * lda + c];
        float b = 0.f, acc1 = 0.f, acc2 = 0.f;
        if (kMode == kFwd)
            acc1 = (B ? B[(int64_t)row * ldb + c] : 0.f) + (bias ? bias[c] : 0.f);
        else
            b = B[(int64_t)row * ldb + c];
        for (int e = e0; e < e1; ++e) {
            const int64_t j = col[e];
            gate1<kMode>(a, b, G1[j * ld1 + c], G2[j * ld2 + c], mult[kMode == kNode ? mirror[e] : e], acc1, acc2);
        }
        O1[(int64_t)row * ldo1 + c] = acc1;
        if (kMode == kNode) O2[(int64_t)row * ldo2 + c] = acc2;
    }
}

inline bool rgate_dims_ok(int C) { return C > 0 && C < (1 << 24); }
inline bool vec_ok(const float* p, int64_t ld) { return al16(p) && ld % 4 == 0; }

template <int kMode>
int rgate_launch(const ddmp_graph* g, const float* A, int64_t lda, const float* B, int64_t ldb, const float* bias, const float* G1,
                 int64_t ld1, const float* G2, int64_t ld2, float* O1, int64_t ldo1, float* O2, int64_t ldo2, float* dS,
                 int64_t ldds, int C, ddmp_stream stream) {
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(A, lda) && (!B || vec_ok(B, ldb)) && al16(bias) && vec_ok(G1, ld1) && vec_ok(G2, ld2) &&
                     vec_ok(O1, ldo1) && (!O2 || vec_ok(O2, ldo2)) && (!dS || vec_ok(dS, ldds));
    return launch_rows((hipStream_t)stream, (int)g->n_rows, vec, rgate_kernel<kMode>, rgate_scalar_kernel<kMode>, g->rowptr, g->col,
                       g->mirror, g->a, A, lda, B, ldb, bias, G1, ld1, G2, ld2, O1, ldo1, O2, ldo2, dS, ldds, (int)g->n_rows, C);
}

}  // namespace

extern "C" int ddmp_rgate_fwd_f32(const ddmp_graph* g, const float* K, int64_t ldk, const float* Q, int64_t ldq, const float* V,
                                  int64_t ldv, int C, const float* skip, int64_t lds, const float* bias, float* Y, int64_t ldy,
                                  ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && K && Q && V && Y && rgate_dims_ok(C) && ldk >= C && ldq >= C && ldv >= C && ldy >= C &&
            (!skip || lds >= C) && Y != K && Y != Q && Y != V && Y != skip && Y != bias);
    return rgate_launch<kFwd>(g, K, ldk, skip, lds, bias, Q, ldq, V, ldv, Y, ldy, nullptr, 0, nullptr, 0, C, stream);
}

extern "C" int ddmp_rgate_bwd_row_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* K, int64_t ldk,
                                      const float* Q, int64_t ldq, const float* V, int64_t ldv, int C, float* dK, int64_t lddk,
                                      ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && dOut && K && Q && V && dK && rgate_dims_ok(C) && lddo >= C && ldk >= C && ldq >= C && ldv >= C &&
            lddk >= C && dK != dOut && dK != K && dK != Q && dK != V);
    return rgate_launch<kRow>(g, K, ldk, dOut, lddo, nullptr, Q, ldq, V, ldv, dK, lddk, nullptr, 0, nullptr, 0, C, stream);
}

extern "C" int ddmp_rgate_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* K, int64_t ldk,
                                       const float* Q, int64_t ldq, const float* V, int64_t ldv, int C, float* dQ, int64_t lddq,
                                       float* dV, int64_t lddv, float* dS, int64_t ldds, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && dOut && K && Q && V && dQ && dV && rgate_dims_ok(C) && lddo >= C && ldk >= C && ldq >= C &&
            ldv >= C && lddq >= C && lddv >= C && (!dS || ldds >= C));
    const float* ins[4] = {dOut, K, Q, V};
    float* outs[3] = {dQ, dV, dS};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 4; ++i) ARG_TRY(outs[o] != ins[i]);
        for (int p = 0; p < o; ++p) ARG_TRY(outs[o] != outs[p]);
    }
    return rgate_launch<kNode>(g, Q, ldq, V, ldv, nullptr, K, ldk, dOut, lddo, dQ, lddq, dV, lddv, dS, ldds, C, stream);
}

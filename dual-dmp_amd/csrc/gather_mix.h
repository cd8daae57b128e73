// Mixing `heads` gathered blocks by per-entry factors, on the row-gather layout of row_gather.h: the three gather loops shared by
// feast.hip (factors = the head softmax beta) and gmm.hip (factors = the Gaussian-mixture weights w) -- forward, the dot products
// of the edge-side backward, the node-side backward -- parameterised on the [entries, heads] array the factors are read from.
#pragma once
#include "row_gather.h"

namespace {

constexpr int kMaxHeads = 256;     // (one thread per head in the column-sum reduction of feast.hip)

// Forward gather of ONE output float4 (column block q) of a row with nn > 0 entries from rbase on:
// sum_{e in row} sum_h fac[e, h] Hf[col e, h, 4q .. 4q+3], accumulated in registers over all entries and heads; with lw < 8 the
// 8 / lw head groups of the slab are combined by the fixed xor tree (every lane of the row group returns the row's sum).
__device__ __forceinline__ float4 mix_gather_row(const int* __restrict__ col, const float* __restrict__ Hf, int64_t ldh,
                                                 const float* fac, int heads, int C, int lw, int hp, int sub, int rbase, int nn,
                                                 int q) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int b0 = 0; b0 < nn; b0 += kEB) {
        auto batch = [&](auto ne_tag) {
            constexpr int NE = decltype(ne_tag)::value;
            const float* xp[NE];
            const float* fp[NE];
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                const int64_t e = rbase + min(b0 + k, nn - 1);
                xp[k] = Hf + (int64_t)col[e] * ldh + q * 4;
                fp[k] = fac + e * heads;
            }
            FOR_HEAD_PASSES(heads) {
                float4 x[NE];
                float f[NE];
#pragma unroll
                for (int k = 0; k < NE; ++k) {
                    x[k] = ld4(xp[k] + hh * C);
                    f[k] = fp[k][hh];
                }
#pragma unroll
                for (int k = 0; k < NE; ++k) fma4(acc, (hv && b0 + k < nn) ? f[k] : 0.f, x[k]);
            }
        };
        ROW_BATCH_SWITCH(b0, nn, batch)
    }
    if (lw < 8) {                                                 // the 8 / lw head groups of this slab -> one row
        acc.x = red_heads(acc.x, lw);
        acc.y = red_heads(acc.y, lw);
        acc.z = red_heads(acc.z, lw);
        acc.w = red_heads(acc.w, lw);
    }
    return acc;
}

// Edge-side dot products of a row with nn > 0 entries: gd[e, h] = grow[:] . Hf[col e, h, :] for every (entry, head), each reduced
// over the head's lw lanes by the fixed xor tree and written by the head's first lane.
__device__ __forceinline__ void mix_edge_dots(const int* __restrict__ col, const float* __restrict__ grow,
                                              const float* __restrict__ Hf, int64_t ldh, float* gd, int heads, int C, int lw,
                                              int hp, int sub, int q0, int rbase, int nn) {
    const int W = C >> 2;
    FOR_HEAD_PASSES(heads) {
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
                    const float4 y = ld4(grow + q * 4);
                    float4 x[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) x[k] = ld4(xp[k] + q * 4);
#pragma unroll
                    for (int k = 0; k < NE; ++k) acc[k] = dot4(y, x[k], acc[k]);
                }
#pragma unroll
                for (int k = 0; k < NE; ++k) {
                    const float t = red_sum(acc[k], lw);
                    if (b0 + k < nn && hv && q0 == 0) gd[(int64_t)(rbase + b0 + k) * heads + h] = t;
                }
            };
            ROW_BATCH_SWITCH(b0, nn, batch)
        }
    }
}

// Node-side gather of ONE float4 (head hh, column block q) of row j: sum_{e' in row j} fac[mirror e', hh] dOut[col e', 4q .. 4q+3]
// (the structure is symmetric: row j's own entries enumerate the targets j feeds).  nn == 0 gives 0.
__device__ __forceinline__ float4 mix_node_gather(const int* __restrict__ col, const int* __restrict__ mirror,
                                                  const float* __restrict__ dOut, int64_t lddo, const float* __restrict__ fac,
                                                  int heads, int hh, int rbase, int nn, int q) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
    for (int b0 = 0; b0 < nn; b0 += kEB) {
        auto batch = [&](auto ne_tag) {
            constexpr int NE = decltype(ne_tag)::value;
            float4 x[NE];
            float f[NE];
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                const int e = rbase + min(b0 + k, nn - 1);
                x[k] = ld4(dOut + (int64_t)col[e] * lddo + q * 4);
                const float v = fac[(int64_t)mirror[e] * heads + hh];
                f[k] = b0 + k < nn ? v : 0.f;
            }
#pragma unroll
            for (int k = 0; k < NE; ++k) fma4(acc, f[k], x[k]);
        };
        ROW_BATCH_SWITCH(b0, nn, batch)
    }
    return acc;
}

inline bool feast_dims_ok(int heads, int C) { return heads > 0 && heads <= kMaxHeads && C > 0 && (int64_t)heads * C < (1 << 24); }

}  // namespace

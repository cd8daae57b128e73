// The "mix `heads` gathered blocks by per-entry factors" work layout shared by feast.hip (factors = the head softmax beta) and
// gmm.hip (factors = the Gaussian-mixture weights w): the chunk prologue, the per-entry-count batch switch, the float4 helpers and
// the three gather loops (forward, the dot products of the edge-side backward, the node-side backward), parameterised on the
// [entries, heads] array the per-entry factors are read from.  Layout and conventions: the header comment of feast.hip.
#pragma once
#include "ddmp_common.h"

#include <type_traits>

namespace {

using namespace ddmp;

constexpr int kRB = 64;            // rows per workgroup
constexpr int kEB = 8;             // entries per batch
constexpr int kMaxHeads = 256;     // (one thread per head in the column-sum reduction of feast.hip)

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}
__device__ __forceinline__ void fma4(float4& acc, float s, float4 x) {
    acc.x = fmaf(s, x.x, acc.x);
    acc.y = fmaf(s, x.y, acc.y);
    acc.z = fmaf(s, x.z, acc.z);
    acc.w = fmaf(s, x.w, acc.w);
}
// fixed xor tree over the lw (1, 2, 4, 8; kernel-uniform) low lanes of an 8-lane row group
__device__ __forceinline__ float red_sum(float t, int lw) {
    if (lw > 1) t += __shfl_xor(t, 1, 64);
    if (lw > 2) t += __shfl_xor(t, 2, 64);
    if (lw > 4) t += __shfl_xor(t, 4, 64);
    return t;
}
// fixed xor tree over the 8 / lw lanes of a row group that hold the same columns (different heads)
__device__ __forceinline__ float red_heads(float t, int lw) {
    if (lw < 2) t += __shfl_xor(t, 1, 64);
    if (lw < 4) t += __shfl_xor(t, 2, 64);
    if (lw < 8) t += __shfl_xor(t, 4, 64);
    return t;
}
inline int lanes_per_head(int C) {
    const int W = C / 4;
    return (W == 1 || W == 2 || W == 4) ? W : 8;
}

// This workgroup's chunk, the lane's 8-lane row group and its place in a head pass (lw lanes per head, hp heads per pass).
#define FEAST_CHUNK_PROLOGUE                                                                       \
    const int chunk = (blockIdx.x & (kXcd - 1)) * chunks_per_xcd + (blockIdx.x >> 3);              \
    if (chunk >= n_chunks) return;                                                                 \
    const int r0 = chunk * kRB;                                                                    \
    const int nr = min(kRB, n_rows - r0);                                                          \
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                    \
    const int grp = lane >> 3, sl = lane & 7;                                                      \
    const int hp = 8 / lw, sub = sl / lw, q0 = sl & (lw - 1);

// Run `batch` with the entry count of this batch as a compile-time constant: the longest row's count among the wave's active
// rows (wave-uniform, from ballots).
#define FEAST_BATCH_SWITCH(b0, nn, batch)                                                          \
    {                                                                                              \
        int ne_w = 0;                                                                              \
        _Pragma("unroll") for (int k = 0; k < kEB; ++k) ne_w += __any((b0) + k < (nn)) ? 1 : 0;     \
        switch (ne_w) {                                                                            \
            case 1: batch(std::integral_constant<int, 1>()); break;                                \
            case 2: batch(std::integral_constant<int, 2>()); break;                                \
            case 3: batch(std::integral_constant<int, 3>()); break;                                \
            case 4: batch(std::integral_constant<int, 4>()); break;                                \
            case 5: batch(std::integral_constant<int, 5>()); break;                                \
            case 6: batch(std::integral_constant<int, 6>()); break;                                \
            case 7: batch(std::integral_constant<int, 7>()); break;                                \
            default: batch(std::integral_constant<int, 8>()); break;                               \
        }                                                                                          \
    }

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
#pragma unroll 1
            for (int hg = 0; hg < heads; hg += hp) {
                const int h = hg + sub;
                const bool hv = h < heads;
                const int hh = hv ? h : heads - 1;
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
        FEAST_BATCH_SWITCH(b0, nn, batch)
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
#pragma unroll 1
    for (int hg = 0; hg < heads; hg += hp) {
        const int h = hg + sub;
        const bool hv = h < heads;
        const int hh = hv ? h : heads - 1;
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
            FEAST_BATCH_SWITCH(b0, nn, batch)
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
        FEAST_BATCH_SWITCH(b0, nn, batch)
    }
    return acc;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool feast_graph_ok(const ddmp_graph* g) {
    return g && (g->valued & DDMP_GV_VALUED) && g->a && g->mirror && g->n_cols == g->n_rows && g->n_rows < (int64_t)INT32_MAX;
}
inline bool feast_dims_ok(int heads, int C) { return heads > 0 && heads <= kMaxHeads && C > 0 && (int64_t)heads * C < (1 << 24); }

}  // namespace

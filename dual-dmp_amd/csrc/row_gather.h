// The row-gather work layout of the graph-operator kernels (sddmm.hip, gat.hip, gatv2.hip, tconv.hip, rgate.hip, feast.hip,
// gmm.hip, gmax.hip, spline.hip, nstat.hip, pna.hip, gsoftmax.hip, cgate.hip, ppf.hip; gather_mix.h, colsum_final.h):
// the one place that fixes it.  (The SpMM files have their own variants of it; they do not include this header.)
//   * a workgroup (4 waves) owns a chunk of kRB = 64 consecutive rows; blockIdx -> chunk is XCD-aware (block b runs on XCD b % 8,
//     so XCD x takes the chunks x * chunks_per_xcd ..: the ~deg re-reads of a neighbour row by neighbouring output rows hit that
//     XCD's L2);
//   * 8 lanes x float4 cover one 128-byte slab of a row: 8 rows per wave step, two steps per chunk (local row
//     wave * 8 + grp + qq * 32, qq = 0, 1); the 8 lanes of a row group leave together;
//   * operators with heads walk a row in HEAD PASSES, so that a lane's head is fixed while it gathers and a float4 never straddles
//     a head.  With W = C / 4 float4 per head: W in {1, 2, 4} -> lw = W lanes per head and hp = 8 / W heads per pass (the 8 lanes
//     cover one slab of the row, eight / four / two heads inside it); any other W -> lw = 8, the 8 lanes walk one head's W float4,
//     8 at a time.  The lanes of the last pass that hold no valid head run head heads - 1 again and store nothing;
//   * per-(row, head) reductions are strided over the head's lanes and combined by a fixed xor tree;
//   * a row's entries are gathered kEB = 8 at a time with the batch compiled per entry count: the LONGEST row's count among the
//     wave's active rows (wave-uniform, from ballots).  The loads of a batch are unconditional -- a per-lane predicate on a load puts
//     a branch and a full wait behind every one of them, and the loads of a batch must be in flight together; a lane whose row is
//     shorter re-reads its last entry (an L1 hit) and its kernel masks that slot out.
// No atomics, every sum in a fixed order: bitwise reproducible.  Every row * stride product is int64.  Widths that are not a
// multiple of 4 (or operands that fail al16) take scalar kernels, one thread per row, 256 rows per workgroup.
// Also here, written once: the row loop and the head-pass loop (FOR_CHUNK_ROWS, FOR_CHUNK_ROW_ENTRIES, FOR_HEAD_PASSES) and the host's
// vector-or-scalar launch of every entry point (launch_rows, launch_head_rows).  The second stage of the two-stage column
// reductions is colsum_final.h.
#pragma once
#include "ddmp_common.h"

#include <type_traits>
#include <utility>

namespace {

using namespace ddmp;

constexpr int kRB = 64;            // rows per workgroup
constexpr int kEB = 8;             // entries per batch

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ int4 ld4i(const int* p) { return *reinterpret_cast<const int4*>(p); }
__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}
__device__ __forceinline__ void fma4(float4& acc, float s, float4 x) {
    acc.x = fmaf(s, x.x, acc.x);
    acc.y = fmaf(s, x.y, acc.y);
    acc.z = fmaf(s, x.z, acc.z);
    acc.w = fmaf(s, x.w, acc.w);
}
// fixed xor tree over the lw (1, 2, 4, 8; kernel-uniform) low lanes of an 8-lane row group: the lanes of one head
__device__ __forceinline__ float red_sum(float t, int lw) {
    if (lw > 1) t += __shfl_xor(t, 1, 64);
    if (lw > 2) t += __shfl_xor(t, 2, 64);
    if (lw > 4) t += __shfl_xor(t, 4, 64);
    return t;
}
__device__ __forceinline__ float red_max(float t, int lw) {
    if (lw > 1) t = fmaxf(t, __shfl_xor(t, 1, 64));
    if (lw > 2) t = fmaxf(t, __shfl_xor(t, 2, 64));
    if (lw > 4) t = fmaxf(t, __shfl_xor(t, 4, 64));
    return t;
}
// fixed xor tree over the 8 / lw lanes of a row group that hold the same columns (different heads)
__device__ __forceinline__ float red_heads(float t, int lw) {
    if (lw < 2) t += __shfl_xor(t, 1, 64);
    if (lw < 4) t += __shfl_xor(t, 2, 64);
    if (lw < 8) t += __shfl_xor(t, 4, 64);
    return t;
}
// the running extremum and its entry's id: replaced on a strict > (<) only, so the first entry in CSR order wins a tie
__device__ __forceinline__ void take_gt(float& m, int& id, float v, int j) {
    const bool w = v > m;
    m = w ? v : m;
    id = w ? j : id;
}
__device__ __forceinline__ void take_lt(float& m, int& id, float v, int j) {
    const bool w = v < m;
    m = w ? v : m;
    id = w ? j : id;
}
inline int lanes_per_head(int C) {
    const int W = C / 4;
    return (W == 1 || W == 2 || W == 4) ? W : 8;
}

// This workgroup's chunk and the lane's 8-lane row group (kernel parameters n_rows, chunks_per_xcd, n_chunks).
#define ROW_CHUNK_PROLOGUE                                                                         \
    const int chunk = (blockIdx.x & (kXcd - 1)) * chunks_per_xcd + (blockIdx.x >> 3);              \
    if (chunk >= n_chunks) return;                                                                 \
    const int r0 = chunk * kRB;                                                                    \
    const int nr = min(kRB, n_rows - r0);                                                          \
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                    \
    const int grp = lane >> 3, sl = lane & 7;

// The same, and the lane's place in a head pass (kernel parameter lw: lanes per head; hp heads per pass).
#define HEAD_CHUNK_PROLOGUE                                                                        \
    ROW_CHUNK_PROLOGUE                                                                             \
    const int hp = 8 / lw, sub = sl / lw, q0 = sl & (lw - 1);

// Run `batch` with the entry count of this batch as a compile-time constant: the longest row's count among the wave's active
// rows (wave-uniform, from ballots).
#define ROW_BATCH_SWITCH(b0, nn, batch)                                                            \
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

// The row loop, `FOR_CHUNK_ROWS { ... }`: the rows of this workgroup's chunk that the lane's row group takes, as `row` (the 8 lanes
// of a row group leave together; `continue` goes to the next row); FOR_CHUNK_ROW_ENTRIES also gives the row's entries rbase ..
// rbase + nn (kernel parameter rowptr).
#define FOR_CHUNK_ROWS                                                                             \
    _Pragma("unroll 1") for (int qq = 0; qq < 2; ++qq)                                             \
        if (const int lr = wave * 8 + grp + qq * 32; lr < nr)                                      \
            if (const int row = r0 + lr; true)
#define FOR_CHUNK_ROW_ENTRIES                                                                      \
    FOR_CHUNK_ROWS                                                                                 \
        if (const int rbase = rowptr[row], nn = rowptr[row + 1] - rbase; true)

// The head-pass loop, `FOR_HEAD_PASSES(heads) { ... }`: this lane's head h of every pass, hv: it is a valid one, hh: the head it
// runs -- a lane of the last pass that holds no valid head runs head heads - 1 again and stores nothing (`continue`: next pass).
#define FOR_HEAD_PASSES(heads)                                                                     \
    _Pragma("unroll 1") for (int hg = 0; hg < (heads); hg += hp)                                   \
        if (const int h = hg + sub; true)                                                          \
            if (const bool hv = h < (heads); true)                                                 \
                if (const int hh = hv ? h : (heads) - 1; true)

// ------------------------------------------------------------------------------------------------ the gather of one head pass
// out[row, hh, :] = init(q) + sum_{e in row} f_e X[col e, hh, :],  f_e = fac[(kMirror ? mirror[e] : e), hh].  The lanes of the
// pass that hold no valid head (hv false) run head hh = heads - 1 again and store nothing.
template <bool kMirror, class Init>
__device__ __forceinline__ void gather_pass(const int* __restrict__ col, const int* __restrict__ mirror, const float* fac,
                                            const float* __restrict__ X, int64_t ldx, float* orow, int rbase, int nn, int heads,
                                            int C, int hh, bool hv, int q0, int lw, Init init) {
    const int W = C >> 2;
    if (nn == 0) {
        for (int q = q0; q < W; q += lw)
            if (hv) *reinterpret_cast<float4*>(orow + hh * C + q * 4) = init(q);
        return;
    }
#pragma unroll 1
    for (int b0 = 0; b0 < nn; b0 += kEB) {
        auto batch = [&](auto ne_tag) {
            constexpr int NE = decltype(ne_tag)::value;
            const float* xp[NE];
            float f[NE];
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                const int e = rbase + min(b0 + k, nn - 1);
                xp[k] = X + (int64_t)col[e] * ldx + hh * C;
                const int64_t fe = kMirror ? mirror[e] : e;
                const float v = fac[fe * heads + hh];
                f[k] = b0 + k < nn ? v : 0.f;
            }
            for (int q = q0; q < W; q += lw) {
                float* op = orow + hh * C + q * 4;
                float4 acc = b0 == 0 ? init(q) : ld4(op);
                float4 x[NE];
#pragma unroll
                for (int k = 0; k < NE; ++k) x[k] = ld4(xp[k] + q * 4);
#pragma unroll
                for (int k = 0; k < NE; ++k) fma4(acc, f[k], x[k]);
                if (hv) *reinterpret_cast<float4*>(op) = acc;
            }
        };
        ROW_BATCH_SWITCH(b0, nn, batch)
    }
}

// ------------------------------------------------------------------------------------------------ host side
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// an OPTIONAL float32 / int32 [n, C] operand: present -> wide enough; `vec`: leading dimension % 4 == 0 and 16-byte aligned
inline bool wide(const void* m, int64_t ld, int64_t C) { return !m || ld >= C; }
inline bool vec_ok(const void* m, int64_t ld) { return !m || (ld % 4 == 0 && al16(m)); }

// The attention graph: the coalesced square structure of a valued graph.  `values`: the kernels also read the entries'
// multiplicities (g->a) and the mirror map; the arg-max gather reads neither.
inline bool attn_graph_ok(const ddmp_graph* g, bool values = true) {
    return g && (g->valued & DDMP_GV_VALUED) && (!values || (g->a && g->mirror)) && g->n_cols == g->n_rows &&
           g->n_rows < (int64_t)INT32_MAX;
}

// Launch geometry for n rows.  Vector kernels: `grid` workgroups of 256 threads, and the kernel arguments chunks_per_xcd = cpx
// and n_chunks; scalar kernels: scalar_grid(n) workgroups of 256 threads.
struct RowGrid {
    int n_chunks, cpx;
    dim3 grid;
};
inline RowGrid row_grid(int n) {
    const int n_chunks = (int)cdiv(n, kRB), cpx = (int)cdiv(n_chunks, kXcd);
    return {n_chunks, cpx, dim3(cpx * kXcd)};
}
inline dim3 scalar_grid(int n) { return dim3((unsigned)cdiv(n, 256)); }

// Launch the vector kernel (`vec`: the caller's alignment predicate holds) or the scalar kernel over n > 0 rows.  The vector
// kernel's parameters are the scalar kernel's, then (launch_head_rows) lw, then chunks_per_xcd, n_chunks.  Returns the status.
template <class VK, class SK, class... Args>
inline int launch_rows(hipStream_t st, int n, bool vec, VK vk, SK sk, Args... args) {
    if (vec) {
        const RowGrid rg = row_grid(n);
        hipLaunchKernelGGL(vk, rg.grid, dim3(256), 0, st, args..., rg.cpx, rg.n_chunks);
    } else {
        hipLaunchKernelGGL(sk, scalar_grid(n), dim3(256), 0, st, args...);
    }
    LAUNCH_TRY();
    return DDMP_OK;
}
template <class VK, class SK, class... Args>
inline int launch_head_rows(hipStream_t st, int n, bool vec, int lw, VK vk, SK sk, Args... args) {
    if (vec) {
        const RowGrid rg = row_grid(n);
        hipLaunchKernelGGL(vk, rg.grid, dim3(256), 0, st, args..., lw, rg.cpx, rg.n_chunks);
    } else {
        hipLaunchKernelGGL(sk, scalar_grid(n), dim3(256), 0, st, args...);
    }
    LAUNCH_TRY();
    return DDMP_OK;
}

// The subset dispatch of the kernels compiled per subset of their outputs: launch(std::integral_constant<int, kW>()) for the kW of
// the allowed subsets that equals `what`, so only the listed subsets are instantiated.  (The entry points' checks admit no other.)
template <int... kWs, class Launch>
inline int for_subset(std::integer_sequence<int, kWs...>, int what, Launch launch) {
    int st = DDMP_EINVAL;
    (void)((what == kWs && ((st = launch(std::integral_constant<int, kWs>())), true)) || ...);
    return st;
}

}  // namespace

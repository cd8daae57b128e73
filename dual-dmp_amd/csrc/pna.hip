// Neighbour moments (PNAConv): the fused mean-or-sum / max / min / std-or-var gather and its one-launch backward.
//
//   S[i,c]   = w_i sum_{e in row i} a_e B[col e, c] (+ R[i,c], mean) (+ deg_i R[i,c], sum),   w_i = 1 / deg_i (mean) or 1
//   Mx[i,c]  = max_{e in row i} B[col e, c] (+ R[i,c]),   argmx[i,c] = col e of the winning entry;   Mn, argmn likewise
//   V[i,c]   = the second central moment of the row's entries: with K = B[col rbase, c] (the row's first entry), d_e = B[col e, c] - K,
//              m1 = sum_e a_e d_e, m2 = sum_e a_e d_e d_e:   mu = K + m1 w,   var = max(m2 w - (m1 w)^2, 0),   w = 1 / deg_i,
//              V = var, or (std) var > 1e-5 ? sqrt(var) : 0 -- PyG 2.2.0's StdAggregation.  R is never added to V.
//   dB[j,c]  = sum_{e' in row j} ( a w_i dS[i,c] + (argmx[i,c] == j ? dMx[i,c] : 0) + (argmn[i,c] == j ? dMn[i,c] : 0) )
//              + B[j,c] sum_{e' in row j} a w_i dQ[i,c],   i = col e', a = mult[mirror e'], w_i = invdeg[i] or 1
//
// over the COALESCED CSR of the attention graph without loop handling, the graph of nstat.hip, whose rules the sum family and the
// extrema follow exactly: the sum is one fma per entry in CSR order and the mean ONE multiplication of it; the running extrema start
// at the row's first entry and are replaced on a strict > (<) only, so the smallest source id wins a tie.  A row without entries
// gets 0 in every block (whatever R is), -1 in the args, 0 in mu and invdeg.
// The second moment is SHIFTED by the row's first entry, which the extrema load anyway: the sums run over differences of the size
// of the row's spread, so a column 1000 + N(0, 1) keeps its variance to float32 rounding, where mean(x^2) - mean(x)^2 loses it
// entirely.  Every operation of an epilogue is an explicit single rounding (no contraction), so a block of a fused call has the
// bits of the same block requested alone, and without R the sum family and the extrema have the bits of nstat.hip.
// Tower-major output: column c of a statistic block lands at base + row * ld + (c / tw) * tstride + c % tw, so the row buffer can be
// [tower][aggregator][F]; tw == C is the plain layout.  The args, mu and invdeg are always plain.  The vector kernels need
// tw % 4 == 0 (a float4 never straddles a tower); anything else takes the scalar kernels.
// The backward's second stream dQ shares the factor a w_i with dS; its gathered sum is multiplied ONCE by the row's own B[j].
// On the row-gather layout (row_gather.h) without heads.  No LDS, no barrier, no atomics; every output is written completely.
//
// Resource usage of the vector kernels (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950): scratch 0 bytes and LDS 0
// bytes in every one, no AGPRs; VGPRs (waves per SIMD) per requested subset (s = sum family, x = max, n = min, v = moment /
// q = the dQ stream):
//   forward   s 78 (6)   x 82 (5)   sx 100 (4)   n 80 (6)   sn 98 (4)   xn 94 (5)   sxn 115 (4)   v 112 (4)   sv 148 (3)   xv 132 (3)
//             sxv 176 (2)   nv 130 (3)   snv 139 (3)   xnv 154 (3)   sxnv 169 (2)
//   backward  s 72 (7)   x 94 (5)   sx 127 (4)   n 94 (5)   sn 127 (4)   xn 129 (3)   sxn 128 (4)   sq 120 (4)   sxq 129 (3)
//             snq 129 (3)   sxnq 167 (3)
#include "row_gather.h"

namespace {

constexpr int kSum = 1, kMax = 2, kMin = 4, kVar = 8;
constexpr float kStdFloor = 1e-5f;

struct MomFwd {
    const float* B;
    int64_t ldb;
    const float* R;
    int64_t ldr;
    int mean, as_std;
    int tw;
    int64_t tstride;
    float* S;
    int64_t lds;
    float* Mx;
    int64_t ldmx;
    int* argmx;
    int64_t ldamx;
    float* Mn;
    int64_t ldmn;
    int* argmn;
    int64_t ldamn;
    float* V;
    int64_t ldv;
    float* mu;
    int64_t ldmu;
    float* invdeg;
};

struct MomBwd {
    const float* dS;
    int64_t ldds;
    const float* dQ;
    int64_t lddq;
    const float* B;
    int64_t ldb;
    const float* invdeg;
    const float* dMx;
    int64_t lddmx;
    const int* argmx;
    int64_t ldamx;
    const float* dMn;
    int64_t lddmn;
    const int* argmn;
    int64_t ldamn;
    float* dB;
    int64_t lddb;
};

// one entry of the shifted moments: d = x - K, m1 += a d, m2 += (a d) d
__device__ __forceinline__ void moment(float& m1, float& m2, float a, float x, float k) {
    const float d = __fsub_rn(x, k);
    m1 = fmaf(a, d, m1);
    m2 = fmaf(__fmul_rn(a, d), d, m2);
}
// the epilogue of S on a row with entries: (mean: one multiplication) + root (sum: deg x root), never contracted
__device__ __forceinline__ float finish_sum(float acc, float w, float deg, bool mean, bool has_r, float r) {
    float v = mean ? __fmul_rn(acc, w) : acc;
    if (has_r) v = __fadd_rn(v, mean ? r : __fmul_rn(deg, r));
    return v;
}
// the epilogue of the moments on a row with entries -> (V, mu)
__device__ __forceinline__ void finish_var(float m1, float m2, float k, float w, bool as_std, float& v, float& mu) {
    const float m = __fmul_rn(m1, w);
    mu = __fadd_rn(k, m);
    const float var = fmaxf(__fsub_rn(__fmul_rn(m2, w), __fmul_rn(m, m)), 0.f);
    v = as_std ? (var > kStdFloor ? __fsqrt_rn(var) : 0.f) : var;
}
// where column c of a statistic block lands in its row (tower-major; tw == C: c itself)
__device__ __forceinline__ int64_t tower_ofs(int c, int tw, int64_t tstride) { return (int64_t)(c / tw) * tstride + c % tw; }

// ------------------------------------------------------------------------------------------------ forward
template <int kW>
__global__ __launch_bounds__(256) void gather_moments_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ mult, MomFwd p, int n_rows, int C,
                                                             int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool hr = p.R != nullptr, mean = p.mean != 0, as_std = p.as_std != 0, plain = p.tw == C;
    FOR_CHUNK_ROW_ENTRIES {
        float w = 0.f, deg = 0.f;
        if (nn > 0 && ((kW & (kSum | kVar)) || p.invdeg)) {
            // deg_i from the multiplicities: the 8 lanes take the entries 8 apart (small integers: exact in any order)
            for (int e = sl; e < nn; e += 8) deg += mult[rbase + e];
            deg = red_sum(deg, 8);
            w = 1.f / deg;
        }
        if (p.invdeg && sl == 0) p.invdeg[row] = w;
        const int j0 = nn > 0 ? col[rbase] : -1;
        for (int q = sl; q < W; q += 8) {
            float4 s = zero4, mx = zero4, mn = zero4, m1 = zero4, m2 = zero4, k0 = zero4;
            int4 ix = make_int4(j0, j0, j0, j0), in = ix;
            if (nn > 0) {
                if (kW & (kMax | kMin | kVar)) k0 = mx = mn = ld4(p.B + (int64_t)j0 * p.ldb + q * 4);
#pragma unroll 1
                for (int b0 = 0; b0 < nn; b0 += kEB) {
                    auto batch = [&](auto ne_tag) {
                        constexpr int NE = decltype(ne_tag)::value;
                        int j[NE];
                        float f[NE];
                        float4 x[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            const int e = rbase + min(b0 + k, nn - 1);
                            j[k] = col[e];
                            if (kW & (kSum | kVar)) {
                                const float a = mult[e];
                                f[k] = b0 + k < nn ? a : 0.f;     // (a re-read last entry adds nothing)
                            }
                        }
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = ld4(p.B + (int64_t)j[k] * p.ldb + q * 4);
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            if (kW & kSum) fma4(s, f[k], x[k]);
                            if (kW & kVar) {
                                moment(m1.x, m2.x, f[k], x[k].x, k0.x);
                                moment(m1.y, m2.y, f[k], x[k].y, k0.y);
                                moment(m1.z, m2.z, f[k], x[k].z, k0.z);
                                moment(m1.w, m2.w, f[k], x[k].w, k0.w);
                            }
                            if (kW & kMax) {
                                take_gt(mx.x, ix.x, x[k].x, j[k]);
                                take_gt(mx.y, ix.y, x[k].y, j[k]);
                                take_gt(mx.z, ix.z, x[k].z, j[k]);
                                take_gt(mx.w, ix.w, x[k].w, j[k]);
                            }
                            if (kW & kMin) {
                                take_lt(mn.x, in.x, x[k].x, j[k]);
                                take_lt(mn.y, in.y, x[k].y, j[k]);
                                take_lt(mn.z, in.z, x[k].z, j[k]);
                                take_lt(mn.w, in.w, x[k].w, j[k]);
                            }
                        }
                    };
                    ROW_BATCH_SWITCH(b0, nn, batch)
                }
            }
            const bool add_r = hr && nn > 0;                      // (a row without entries: 0 whatever R is)
            const float4 r = add_r ? ld4(p.R + (int64_t)row * p.ldr + q * 4) : zero4;
            const int64_t to = plain ? q * 4 : tower_ofs(q * 4, p.tw, p.tstride);
            if (kW & kSum) {
                s.x = finish_sum(s.x, w, deg, mean, add_r, r.x);
                s.y = finish_sum(s.y, w, deg, mean, add_r, r.y);
                s.z = finish_sum(s.z, w, deg, mean, add_r, r.z);
                s.w = finish_sum(s.w, w, deg, mean, add_r, r.w);
                *reinterpret_cast<float4*>(p.S + (int64_t)row * p.lds + to) = s;
            }
            if (kW & kMax) {
                if (add_r) mx.x = __fadd_rn(mx.x, r.x), mx.y = __fadd_rn(mx.y, r.y), mx.z = __fadd_rn(mx.z, r.z), mx.w = __fadd_rn(mx.w, r.w);
                *reinterpret_cast<float4*>(p.Mx + (int64_t)row * p.ldmx + to) = mx;
                if (p.argmx) *reinterpret_cast<int4*>(p.argmx + (int64_t)row * p.ldamx + q * 4) = ix;
            }
            if (kW & kMin) {
                if (add_r) mn.x = __fadd_rn(mn.x, r.x), mn.y = __fadd_rn(mn.y, r.y), mn.z = __fadd_rn(mn.z, r.z), mn.w = __fadd_rn(mn.w, r.w);
                *reinterpret_cast<float4*>(p.Mn + (int64_t)row * p.ldmn + to) = mn;
                if (p.argmn) *reinterpret_cast<int4*>(p.argmn + (int64_t)row * p.ldamn + q * 4) = in;
            }
            if (kW & kVar) {
                float4 v = zero4, mu = zero4;
                if (nn > 0) {
                    finish_var(m1.x, m2.x, k0.x, w, as_std, v.x, mu.x);
                    finish_var(m1.y, m2.y, k0.y, w, as_std, v.y, mu.y);
                    finish_var(m1.z, m2.z, k0.z, w, as_std, v.z, mu.z);
                    finish_var(m1.w, m2.w, k0.w, w, as_std, v.w, mu.w);
                }
                *reinterpret_cast<float4*>(p.V + (int64_t)row * p.ldv + to) = v;
                *reinterpret_cast<float4*>(p.mu + (int64_t)row * p.ldmu + q * 4) = mu;
            }
        }
    }
}

// one thread per row; the statistics that are not requested have a null pointer
__global__ __launch_bounds__(256) void gather_moments_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const float* __restrict__ mult, MomFwd p, int n_rows, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float w = 0.f, deg = 0.f;
    if (e1 > e0) {
        for (int e = e0; e < e1; ++e) deg += mult[e];
        w = 1.f / deg;
    }
    if (p.invdeg) p.invdeg[row] = w;
    const bool mean = p.mean != 0, as_std = p.as_std != 0, add_r = p.R != nullptr && e1 > e0;
    for (int c = 0; c < C; ++c) {
        float s = 0.f, mx = 0.f, mn = 0.f, m1 = 0.f, m2 = 0.f, k0 = 0.f, v = 0.f, mu = 0.f;
        int ix = -1, in = -1;
        if (e1 > e0) {
            ix = in = col[e0];
            k0 = mx = mn = p.B[(int64_t)ix * p.ldb + c];
            for (int e = e0; e < e1; ++e) {
                const int j = col[e];
                const float x = p.B[(int64_t)j * p.ldb + c], a = mult[e];
                s = fmaf(a, x, s);
                moment(m1, m2, a, x, k0);
                take_gt(mx, ix, x, j);
                take_lt(mn, in, x, j);
            }
            finish_var(m1, m2, k0, w, as_std, v, mu);
        }
        const float r = add_r ? p.R[(int64_t)row * p.ldr + c] : 0.f;
        const int64_t to = tower_ofs(c, p.tw, p.tstride);
        if (p.S) p.S[(int64_t)row * p.lds + to] = e1 > e0 ? finish_sum(s, w, deg, mean, add_r, r) : 0.f;
        if (p.Mx) p.Mx[(int64_t)row * p.ldmx + to] = add_r ? __fadd_rn(mx, r) : mx;
        if (p.argmx) p.argmx[(int64_t)row * p.ldamx + c] = ix;
        if (p.Mn) p.Mn[(int64_t)row * p.ldmn + to] = add_r ? __fadd_rn(mn, r) : mn;
        if (p.argmn) p.argmn[(int64_t)row * p.ldamn + c] = in;
        if (p.V) p.V[(int64_t)row * p.ldv + to] = v;
        if (p.V) p.mu[(int64_t)row * p.ldmu + c] = mu;
    }
}

// ------------------------------------------------------------------------------------------------ backward (node side)
// The gradient streams of a batch are loaded and added one after the other (dS, dQ, the maximum's, the minimum's), so that at most
// 8 x (float4 + int4) loads are in flight per lane; the order is fixed.  (kSum: the dS stream, kVar: the dQ stream.)
template <int kW>
__global__ __launch_bounds__(256) void gather_moments_bwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                 const int* __restrict__ mirror, const float* __restrict__ mult,
                                                                 MomBwd p, int n_rows, int C, int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        for (int q = sl; q < W; q += 8) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), accq = acc;
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    int j[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) j[k] = col[rbase + min(b0 + k, nn - 1)];
                    if (kW & kSum) {
                        float f[NE];
                        float4 x[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            const float a = mult[mirror[rbase + min(b0 + k, nn - 1)]];
                            const float wi = p.invdeg ? p.invdeg[j[k]] : 1.f;
                            f[k] = b0 + k < nn ? a * wi : 0.f;   // (a re-read last entry adds nothing)
                        }
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = ld4(p.dS + (int64_t)j[k] * p.ldds + q * 4);
#pragma unroll
                        for (int k = 0; k < NE; ++k) fma4(acc, f[k], x[k]);
                        if (kW & kVar) {
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int k = 0; k < NE; ++k) x[k] = ld4(p.dQ + (int64_t)j[k] * p.lddq + q * 4);
#pragma unroll
                            for (int k = 0; k < NE; ++k) fma4(accq, f[k], x[k]);
                        }
                    }
                    auto extremum = [&](const float* dM, int64_t lddm, const int* arg, int64_t lda) {
                        int4 wn[NE];
                        float4 x[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            wn[k] = ld4i(arg + (int64_t)j[k] * lda + q * 4);
                            x[k] = ld4(dM + (int64_t)j[k] * lddm + q * 4);
                        }
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            const int me = b0 + k < nn ? row : -2;        // (a re-read last entry adds nothing; arg >= -1)
                            acc.x += wn[k].x == me ? x[k].x : 0.f;
                            acc.y += wn[k].y == me ? x[k].y : 0.f;
                            acc.z += wn[k].z == me ? x[k].z : 0.f;
                            acc.w += wn[k].w == me ? x[k].w : 0.f;
                        }
                    };
                    // (the scheduler may not pull the next stream's loads in front of this one's adds: registers)
                    if ((kW & kSum) && (kW & (kMax | kMin))) __builtin_amdgcn_sched_barrier(0);
                    if (kW & kMax) extremum(p.dMx, p.lddmx, p.argmx, p.ldamx);
                    if ((kW & kMax) && (kW & kMin)) __builtin_amdgcn_sched_barrier(0);
                    if (kW & kMin) extremum(p.dMn, p.lddmn, p.argmn, p.ldamn);
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
            if (kW & kVar) {
                const float4 b = ld4(p.B + (int64_t)row * p.ldb + q * 4);
                acc.x = fmaf(b.x, accq.x, acc.x), acc.y = fmaf(b.y, accq.y, acc.y);
                acc.z = fmaf(b.z, accq.z, acc.z), acc.w = fmaf(b.w, accq.w, acc.w);
            }
            *reinterpret_cast<float4*>(p.dB + (int64_t)row * p.lddb + q * 4) = acc;
        }
    }
}

__global__ __launch_bounds__(256) void gather_moments_bwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                        const int* __restrict__ mirror,
                                                                        const float* __restrict__ mult, MomBwd p, int n_rows,
                                                                        int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int c = 0; c < C; ++c) {
        float acc = 0.f, accq = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int64_t j = col[e];
            const float f = p.dS ? mult[mirror[e]] * (p.invdeg ? p.invdeg[j] : 1.f) : 0.f;
            if (p.dS) acc = fmaf(f, p.dS[j * p.ldds + c], acc);
            if (p.dQ) accq = fmaf(f, p.dQ[j * p.lddq + c], accq);
            if (p.dMx) acc += p.argmx[j * p.ldamx + c] == row ? p.dMx[j * p.lddmx + c] : 0.f;
            if (p.dMn) acc += p.argmn[j * p.ldamn + c] == row ? p.dMn[j * p.lddmn + c] : 0.f;
        }
        if (p.dQ) acc = fmaf(p.B[(int64_t)row * p.ldb + c], accq, acc);
        p.dB[(int64_t)row * p.lddb + c] = acc;
    }
}

// the attention graph WITHOUT loop handling: a_e counts the input edges of entry e, so sum_e a_e is the in-degree
inline bool moments_graph_ok(const ddmp_graph* g) { return attn_graph_ok(g) && g->valued == DDMP_GV_VALUED; }
// no two of the present pointers are equal
template <size_t N>
inline bool distinct(const void* const (&ptr)[N]) {
    for (size_t a = 0; a < N; ++a)
        for (size_t b = a + 1; b < N; ++b)
            if (ptr[a] && ptr[a] == ptr[b]) return false;
    return true;
}

template <int kW>
int launch_fwd(hipStream_t st, const ddmp_graph* g, bool vec, const MomFwd& p, int C) {
    return launch_rows(st, (int)g->n_rows, vec, gather_moments_kernel<kW>, gather_moments_scalar_kernel, g->rowptr, g->col, g->a, p,
                       (int)g->n_rows, C);
}
template <int kW>
int launch_bwd(hipStream_t st, const ddmp_graph* g, bool vec, const MomBwd& p, int C) {
    return launch_rows(st, (int)g->n_rows, vec, gather_moments_bwd_kernel<kW>, gather_moments_bwd_scalar_kernel, g->rowptr, g->col,
                       g->mirror, g->a, p, (int)g->n_rows, C);
}

using MomentSubsets = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15>;        // every non-empty subset
using MomentBwdSubsets = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 9, 11, 13, 15>;        // the dQ stream comes with dS

}  // namespace

extern "C" int ddmp_gather_moments_f32(const ddmp_graph* g, const float* B, int64_t ldb, int C, int mean, int as_std, const float* R,
                                       int64_t ldr, int tw, int64_t tstride, float* S, int64_t lds, float* Mx, int64_t ldmx,
                                       int32_t* argmx, int64_t ldamx, float* Mn, int64_t ldmn, int32_t* argmn, int64_t ldamn, float* V,
                                       int64_t ldv, float* mu, int64_t ldmu, float* invdeg, ddmp_stream stream) {
    ARG_TRY(moments_graph_ok(g) && B && C >= 1 && ldb >= C && tw >= 1 && tw <= C && C % tw == 0 && (tw == C || tstride >= tw));
    const int64_t span = (int64_t)(C / tw - 1) * (tw == C ? 0 : tstride) + tw;        // the columns a statistic block spans in its row
    const void* const ptr[] = {B, R, S, Mx, Mn, V, mu, argmx, argmn, invdeg};
    ARG_TRY((S || Mx || Mn || V) && (S || !mean) && (V || !as_std) && (!V == !mu) && (Mx || !argmx) && (Mn || !argmn) && wide(R, ldr, C) &&
            wide(S, lds, span) && wide(Mx, ldmx, span) && wide(Mn, ldmn, span) && wide(V, ldv, span) && wide(mu, ldmu, C) &&
            wide(argmx, ldamx, C) && wide(argmn, ldamn, C) && distinct(ptr));
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && tw % 4 == 0 && (tw == C || tstride % 4 == 0) && vec_ok(B, ldb) && vec_ok(R, ldr) && vec_ok(S, lds) &&
                     vec_ok(Mx, ldmx) && vec_ok(argmx, ldamx) && vec_ok(Mn, ldmn) && vec_ok(argmn, ldamn) && vec_ok(V, ldv) &&
                     vec_ok(mu, ldmu);
    const MomFwd p{B, ldb, R, ldr, mean, as_std, tw, tw == C ? 0 : tstride, S, lds, Mx, ldmx, argmx, ldamx, Mn, ldmn, argmn, ldamn,
                   V, ldv, mu, ldmu, invdeg};
    const int what = (S ? kSum : 0) | (Mx ? kMax : 0) | (Mn ? kMin : 0) | (V ? kVar : 0);
    return for_subset(MomentSubsets(), what, [&](auto kw) { return launch_fwd<kw()>((hipStream_t)stream, g, vec, p, C); });
}

extern "C" int ddmp_gather_moments_bwd_f32(const ddmp_graph* g, int C, const float* dS, int64_t ldds, const float* dQ, int64_t lddq,
                                           const float* B, int64_t ldb, const float* invdeg, const float* dMx,
                                           int64_t lddmx, const int32_t* argmx, int64_t ldamx, const float* dMn, int64_t lddmn,
                                           const int32_t* argmn, int64_t ldamn, float* dB, int64_t lddb, ddmp_stream stream) {
    ARG_TRY(moments_graph_ok(g) && dB && C >= 1 && lddb >= C && (dS || dMx || dMn) && (dS || (!invdeg && !dQ)) && (!dQ == !B) &&
            (!dMx == !argmx) && (!dMn == !argmn) && wide(dS, ldds, C) && wide(dQ, lddq, C) && wide(B, ldb, C) &&
            wide(dMx, lddmx, C) && wide(argmx, ldamx, C) && wide(dMn, lddmn, C) && wide(argmn, ldamn, C) && dB != dS && dB != dQ &&
            dB != B && dB != dMx && dB != dMn && (const void*)dB != (const void*)argmx && (const void*)dB != (const void*)argmn &&
            dB != invdeg);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(dS, ldds) && vec_ok(dQ, lddq) && vec_ok(B, ldb) &&
                     vec_ok(dMx, lddmx) && vec_ok(argmx, ldamx) && vec_ok(dMn, lddmn) && vec_ok(argmn, ldamn) && vec_ok(dB, lddb);
    const MomBwd p{dS, ldds, dQ, lddq, B, ldb, invdeg, dMx, lddmx, argmx, ldamx, dMn, lddmn, argmn, ldamn, dB, lddb};
    const int what = (dS ? kSum : 0) | (dMx ? kMax : 0) | (dMn ? kMin : 0) | (dQ ? kVar : 0);
    return for_subset(MomentBwdSubsets(), what, [&](auto kw) { return launch_bwd<kw()>((hipStream_t)stream, g, vec, p, C); });
}

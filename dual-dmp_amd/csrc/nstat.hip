// Neighbour statistics (SAGEConv): the fused mean-or-sum / max / min gather and its one-launch backward.
//
//   S[i,c]   = w_i sum_{e in row i} a_e X[col e, c] (+ R[i,c]) (+ bias[c]),   w_i = 1 / deg_i (mean) or 1,  deg_i = sum_{e in row i} a_e
//   Mx[i,c]  = max_{e in row i} X[col e, c],   argmx[i,c] = col e of the winning entry   (a row without entries: 0 and -1)
//   Mn[i,c]  = min_{e in row i} X[col e, c],   argmn[i,c] likewise
//   dX[j,c]  = dX0[j,c] + sum_{e' in row j} ( a_{mirror e'} w_i dS[i,c] + (argmx[i,c] == j ? dMx[i,c] : 0)
//                                                                       + (argmn[i,c] == j ? dMn[i,c] : 0) ),   i = col e'
//
// over the COALESCED CSR of the attention graph without loop handling (the graph of gmm.hip / spline.hip: a_e is the number of
// input edges of entry e, so deg_i is the number of input edges into i).  Every neighbour row is loaded ONCE per launch and feeds
// every requested statistic; the kernels are compiled per subset (kSum | kMax | kMin), so a statistic that is not requested costs
// neither a register nor an instruction.  The extrema follow gmax.hip: the running value starts at the row's first entry and is
// replaced on a strict > (<) only, so the first entry in CSR order -- the smallest source id -- wins a tie, and a multiplicity
// cannot matter.  The backward relies on the SYMMETRIC structure: row j's own entries enumerate the rows j feeds, the mirrored
// entry holds the multiplicity of j -> i, and arg holds node ids.
// On the row-gather layout (row_gather.h) without heads: the 8 lanes of a row group walk the C / 4 float4 of the row 8 at a time.
// A shorter row's re-read last entry can neither win a strict comparison nor -- with a zero factor -- add to a sum.  The running
// extrema, their ids and the sums stay in registers over ALL entries of the row: the 1200-entry hub row is exact like any other.
// The sum runs in CSR order, one fma per entry; the mean is ONE multiplication of that sum by 1 / deg_i, the root and the bias
// one addition each, none of them contracted: a block of a fused call has the bits of the same block requested alone.
// No LDS, no barrier, no atomics.
//
// Resource usage of the vector kernels (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950): scratch 0 bytes and LDS 0
// bytes in every one, no AGPRs; VGPRs (waves per SIMD) per requested subset:
//   subset                 sum      max      min      sum+max  sum+min  max+min  sum+max+min
//   gather_stats_kernel     80 (6)   83 (5)   81 (5)  102 (4)  100 (4)   95 (5)  116 (4)
//   gather_stats_bwd_kernel 78 (6)  102 (4)  102 (4)  132 (3)  132 (3)  135 (3)  156 (3)
#include "row_gather.h"

namespace {

constexpr int kSum = 1, kMax = 2, kMin = 4;

struct StatsFwd {
    const float* X;
    int64_t ldx;
    const float* R;
    int64_t ldr;
    const float* bias;
    int mean;
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
    float* invdeg;
    float* Xcopy;
    int64_t ldxc;
};

struct StatsBwd {
    const float* dS;
    int64_t ldds;
    const float* invdeg;
    const float* dMx;
    int64_t lddmx;
    const int* argmx;
    int64_t ldamx;
    const float* dMn;
    int64_t lddmn;
    const int* argmn;
    int64_t ldamn;
    const float* dX0;
    int64_t lddx0;
    float* dX;
    int64_t lddx;
    float* dR;
    int64_t lddr;
};

// the epilogue of S: (mean: one multiplication) + root + bias, never contracted into an fma
__device__ __forceinline__ float finish(float acc, float w, bool mean, bool has_r, float r, bool has_b, float b) {
    float v = mean ? __fmul_rn(acc, w) : acc;
    if (has_r) v = __fadd_rn(v, r);
    if (has_b) v = __fadd_rn(v, b);
    return v;
}

// ------------------------------------------------------------------------------------------------ forward
template <int kW>
__global__ __launch_bounds__(256) void gather_stats_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const float* __restrict__ mult, StatsFwd p, int n_rows, int C,
                                                           int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    FOR_CHUNK_ROW_ENTRIES {
        if (p.Xcopy)
            for (int q = sl; q < W; q += 8)
                *reinterpret_cast<float4*>(p.Xcopy + (int64_t)row * p.ldxc + q * 4) = ld4(p.X + (int64_t)row * p.ldx + q * 4);
        float w = 0.f;                                            // (a row without entries: the sum is 0 whatever w is)
        if (nn > 0 && ((kW & kSum) || p.invdeg)) {
            // deg_i from the multiplicities: the 8 lanes take the entries 8 apart (small integers: exact in any order)
            float deg = 0.f;
            for (int e = sl; e < nn; e += 8) deg += mult[rbase + e];
            deg = red_sum(deg, 8);
            w = 1.f / deg;
        }
        if (p.invdeg && sl == 0) p.invdeg[row] = w;
        const int j0 = nn > 0 ? col[rbase] : -1;
        for (int q = sl; q < W; q += 8) {
            float4 s = zero4, mx = zero4, mn = zero4;
            int4 ix = make_int4(j0, j0, j0, j0), in = ix;
            if (nn > 0) {
                if (kW & (kMax | kMin)) mx = mn = ld4(p.X + (int64_t)j0 * p.ldx + q * 4);
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
                            if (kW & kSum) {
                                const float a = mult[e];
                                f[k] = b0 + k < nn ? a : 0.f;     // (a re-read last entry adds nothing)
                            }
                        }
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = ld4(p.X + (int64_t)j[k] * p.ldx + q * 4);
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            if (kW & kSum) fma4(s, f[k], x[k]);
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
            if (kW & kSum) {
                const bool hr = p.R != nullptr, hb = p.bias != nullptr, mean = p.mean != 0;
                const float4 r = hr ? ld4(p.R + (int64_t)row * p.ldr + q * 4) : zero4;
                const float4 b = hb ? ld4(p.bias + q * 4) : zero4;
                s.x = finish(s.x, w, mean, hr, r.x, hb, b.x);
                s.y = finish(s.y, w, mean, hr, r.y, hb, b.y);
                s.z = finish(s.z, w, mean, hr, r.z, hb, b.z);
                s.w = finish(s.w, w, mean, hr, r.w, hb, b.w);
                *reinterpret_cast<float4*>(p.S + (int64_t)row * p.lds + q * 4) = s;
            }
            if (kW & kMax) {
                *reinterpret_cast<float4*>(p.Mx + (int64_t)row * p.ldmx + q * 4) = mx;
                if (p.argmx) *reinterpret_cast<int4*>(p.argmx + (int64_t)row * p.ldamx + q * 4) = ix;
            }
            if (kW & kMin) {
                *reinterpret_cast<float4*>(p.Mn + (int64_t)row * p.ldmn + q * 4) = mn;
                if (p.argmn) *reinterpret_cast<int4*>(p.argmn + (int64_t)row * p.ldamn + q * 4) = in;
            }
        }
    }
}

// one thread per row; the statistics that are not requested have a null pointer
__global__ __launch_bounds__(256) void gather_stats_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                  const float* __restrict__ mult, StatsFwd p, int n_rows, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float w = 0.f;
    if (e1 > e0) {
        float deg = 0.f;
        for (int e = e0; e < e1; ++e) deg += mult[e];
        w = 1.f / deg;
    }
    if (p.invdeg) p.invdeg[row] = w;
    const bool hr = p.R != nullptr, hb = p.bias != nullptr, mean = p.mean != 0;
    for (int c = 0; c < C; ++c) {
        if (p.Xcopy) p.Xcopy[(int64_t)row * p.ldxc + c] = p.X[(int64_t)row * p.ldx + c];
        float s = 0.f, mx = 0.f, mn = 0.f;
        int ix = -1, in = -1;
        if (e1 > e0) {
            ix = in = col[e0];
            mx = mn = p.X[(int64_t)ix * p.ldx + c];
            for (int e = e0; e < e1; ++e) {
                const int j = col[e];
                const float x = p.X[(int64_t)j * p.ldx + c];
                s = fmaf(mult[e], x, s);
                take_gt(mx, ix, x, j);
                take_lt(mn, in, x, j);
            }
        }
        if (p.S)
            p.S[(int64_t)row * p.lds + c] = finish(s, w, mean, hr, hr ? p.R[(int64_t)row * p.ldr + c] : 0.f, hb, hb ? p.bias[c] : 0.f);
        if (p.Mx) p.Mx[(int64_t)row * p.ldmx + c] = mx;
        if (p.argmx) p.argmx[(int64_t)row * p.ldamx + c] = ix;
        if (p.Mn) p.Mn[(int64_t)row * p.ldmn + c] = mn;
        if (p.argmn) p.argmn[(int64_t)row * p.ldamn + c] = in;
    }
}

// ------------------------------------------------------------------------------------------------ backward (node side)
// The three gradient streams of a batch are loaded and added one after the other (the sum's, the maximum's, the minimum's), so
// that at most 8 x (float4 + int4) loads are in flight per lane; the order is fixed.
template <int kW>
__global__ __launch_bounds__(256) void gather_stats_bwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               const int* __restrict__ mirror, const float* __restrict__ mult,
                                                               StatsBwd p, int n_rows, int C, int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    FOR_CHUNK_ROW_ENTRIES {
        if (p.dR)
            for (int q = sl; q < W; q += 8)
                *reinterpret_cast<float4*>(p.dR + (int64_t)row * p.lddr + q * 4) = ld4(p.dS + (int64_t)row * p.ldds + q * 4);
        for (int q = sl; q < W; q += 8) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
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
            if (p.dX0) {
                const float4 d = ld4(p.dX0 + (int64_t)row * p.lddx0 + q * 4);
                acc.x = d.x + acc.x, acc.y = d.y + acc.y, acc.z = d.z + acc.z, acc.w = d.w + acc.w;
            }
            *reinterpret_cast<float4*>(p.dX + (int64_t)row * p.lddx + q * 4) = acc;
        }
    }
}

__global__ __launch_bounds__(256) void gather_stats_bwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                      const int* __restrict__ mirror,
                                                                      const float* __restrict__ mult, StatsBwd p, int n_rows,
                                                                      int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int c = 0; c < C; ++c) {
        if (p.dR) p.dR[(int64_t)row * p.lddr + c] = p.dS[(int64_t)row * p.ldds + c];
        float acc = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int64_t j = col[e];
            if (p.dS) acc = fmaf(mult[mirror[e]] * (p.invdeg ? p.invdeg[j] : 1.f), p.dS[j * p.ldds + c], acc);
            if (p.dMx) acc += p.argmx[j * p.ldamx + c] == row ? p.dMx[j * p.lddmx + c] : 0.f;
            if (p.dMn) acc += p.argmn[j * p.ldamn + c] == row ? p.dMn[j * p.lddmn + c] : 0.f;
        }
        if (p.dX0) acc = p.dX0[(int64_t)row * p.lddx0 + c] + acc;
        p.dX[(int64_t)row * p.lddx + c] = acc;
    }
}

// the attention graph WITHOUT loop handling: a_e counts the input edges of entry e, so sum_e a_e is the in-degree
inline bool stats_graph_ok(const ddmp_graph* g) { return attn_graph_ok(g) && g->valued == DDMP_GV_VALUED; }

template <int kW>
int launch_fwd(hipStream_t st, const ddmp_graph* g, bool vec, const StatsFwd& p, int C) {
    return launch_rows(st, (int)g->n_rows, vec, gather_stats_kernel<kW>, gather_stats_scalar_kernel, g->rowptr, g->col, g->a, p,
                       (int)g->n_rows, C);
}
template <int kW>
int launch_bwd(hipStream_t st, const ddmp_graph* g, bool vec, const StatsBwd& p, int C) {
    return launch_rows(st, (int)g->n_rows, vec, gather_stats_bwd_kernel<kW>, gather_stats_bwd_scalar_kernel, g->rowptr, g->col,
                       g->mirror, g->a, p, (int)g->n_rows, C);
}

using StatsSubsets = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7>;        // every non-empty subset of sum, max, min

}  // namespace

extern "C" int ddmp_gather_stats_f32(const ddmp_graph* g, const float* X, int64_t ldx, int C, int mean, const float* R, int64_t ldr,
                                     const float* bias, float* S, int64_t lds, float* Mx, int64_t ldmx, int32_t* argmx,
                                     int64_t ldamx, float* Mn, int64_t ldmn, int32_t* argmn, int64_t ldamn, float* invdeg,
                                     float* Xcopy, int64_t ldxc, ddmp_stream stream) {
    ARG_TRY(stats_graph_ok(g) && X && C >= 1 && ldx >= C && (S || Mx || Mn) && (S || (!mean && !R && !bias)) && (Mx || !argmx) &&
            (Mn || !argmn) && wide(R, ldr, C) && wide(S, lds, C) && wide(Mx, ldmx, C) && wide(argmx, ldamx, C) && wide(Mn, ldmn, C) &&
            wide(argmn, ldamn, C) && wide(Xcopy, ldxc, C) && S != X && Mx != X && Mn != X && Xcopy != X && (!S || (S != R && S != Mx &&
            S != Mn && S != Xcopy)) && (!Mx || (Mx != Mn && Mx != Xcopy && Mx != R)) && (!Mn || (Mn != Xcopy && Mn != R)) &&
            (!Xcopy || Xcopy != R));
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(X, ldx) && vec_ok(R, ldr) && (!bias || al16(bias)) && vec_ok(S, lds) && vec_ok(Mx, ldmx) &&
                     vec_ok(argmx, ldamx) && vec_ok(Mn, ldmn) && vec_ok(argmn, ldamn) && vec_ok(Xcopy, ldxc);
    const StatsFwd p{X, ldx, R, ldr, bias, mean, S, lds, Mx, ldmx, argmx, ldamx, Mn, ldmn, argmn, ldamn, invdeg, Xcopy, ldxc};
    const int what = (S ? kSum : 0) | (Mx ? kMax : 0) | (Mn ? kMin : 0);
    return for_subset(StatsSubsets(), what, [&](auto kw) { return launch_fwd<kw()>((hipStream_t)stream, g, vec, p, C); });
}

extern "C" int ddmp_gather_stats_bwd_f32(const ddmp_graph* g, int C, const float* dS, int64_t ldds, const float* invdeg,
                                         const float* dMx, int64_t lddmx, const int32_t* argmx, int64_t ldamx, const float* dMn,
                                         int64_t lddmn, const int32_t* argmn, int64_t ldamn, const float* dX0, int64_t lddx0,
                                         float* dX, int64_t lddx, float* dR, int64_t lddr, ddmp_stream stream) {
    ARG_TRY(stats_graph_ok(g) && dX && C >= 1 && lddx >= C && (dS || dMx || dMn) && (dS || (!invdeg && !dR)) && (!dMx == !argmx) &&
            (!dMn == !argmn) && wide(dS, ldds, C) && wide(dMx, lddmx, C) && wide(argmx, ldamx, C) && wide(dMn, lddmn, C) &&
            wide(argmn, ldamn, C) && wide(dX0, lddx0, C) && wide(dR, lddr, C) && dX != dS && dX != dMx && dX != dMn && dX != dX0 &&
            dX != dR && (!dR || (dR != dS && dR != dMx && dR != dMn && dR != dX0)));
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(dS, ldds) && vec_ok(dMx, lddmx) && vec_ok(argmx, ldamx) && vec_ok(dMn, lddmn) &&
                     vec_ok(argmn, ldamn) && vec_ok(dX0, lddx0) && vec_ok(dX, lddx) && vec_ok(dR, lddr);
    const StatsBwd p{dS, ldds, invdeg, dMx, lddmx, argmx, ldamx, dMn, lddmn, argmn, ldamn, dX0, lddx0, dX, lddx, dR, lddr};
    const int what = (dS ? kSum : 0) | (dMx ? kMax : 0) | (dMn ? kMin : 0);
    return for_subset(StatsSubsets(), what, [&](auto kw) { return launch_bwd<kw()>((hipStream_t)stream, g, vec, p, C); });
}

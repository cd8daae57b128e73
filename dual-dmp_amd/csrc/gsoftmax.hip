// Per-channel softmax aggregation (GENConv / SoftmaxAggregation): the fused gather and its one-launch backward.
//
//   m_j[c]   = max(H[j,c], 0) + eps   (msg_eps >= 0 given)   or   H[j,c]   (no msg_eps): formed in registers, never written
//   p_e      = a_e exp(t m_e - mx) / sum_e a_e exp(t m_e - mx),   mx = max_e t m_e       (per row i AND per channel c)
//   Y[i,c]   = R[i,c] + sum_{e in row i} p_e m_e,      lse[i,c] = mx + log sum_e a_e exp(t m_e - mx)
//   backward, with i = col e', w = a_{mirror e'}, p = exp(t m_j - lse[i,c]), Y' = Y without R:
//   s[j,c]   = sum_{e' in row j} w p dOut[i,c],        r[j,c] = sum_{e' in row j} w p dOut[i,c] (m_j[c] - Y'[i,c])
//   dH[j,c]  = (s + t r) [H[j,c] > 0]  (no mask without msg_eps),   dR[j,:] = dOut[j,:],   dt_rows[j] = sum_c m_j[c] r[j,c]
//   (add_dout: dH[j,c] += dOut[j,c] -- the root term of a layer whose root IS H, one unfused addition after the mask)
//
// over the COALESCED CSR of the attention graph without loop handling (the graph of nstat.hip / pna.hip: a_e is the number of input
// edges of entry e).  On the row-gather layout (row_gather.h) without heads.  A per-channel softmax needs no reduction across lanes
// and no per-entry storage: each lane keeps the running maximum, denominator and numerator of its own four channels in registers
// over ALL entries of the row, so the 1200-entry hub row is exact like any other.  Every neighbour row is loaded ONCE per sweep;
// the row's first entry is read a second time ahead of the sweep, for K below, which pass 1 of every batch needs (the first batch
// re-reads that row from L1: no byte more from memory).
// The forward works on d_e = m_e - K, K the row's first message (which pna.hip's moments shift by too): the softmax does not see
// a shift, t d_e has the rounding of the row's spread and not of its offset, and the numerator sum p_e d_e gives Y = K + num / den,
// so a column 1000 + N(0, 1) keeps Y to float32 rounding.  Within a batch of kEB entries the batch's maximum is taken first and
// the running (mx, den, num) are rescaled ONCE per batch; each element then costs one v_exp_f32 with an argument <= 0 (the
// exponent runs in base 2: t is multiplied by log2 e once per launch, lse is converted back once per row).  A row of at most kEB
// entries is therefore an exact two-pass softmax in registers.  The products t' d are rounded the same way in both passes, so the
// maximal entry contributes exactly a_e >= 1: den >= 1.  A shorter row's re-read last entry cannot raise a maximum and enters the
// sums with a zero factor.  A row without entries gets its root row bit for bit (0 without root) and lse = 0.
// The backward recomputes p from the stored lse (three neighbour streams dOut, Y', lse; the row's own H read once) in the
// (m - Y') form -- E[m^2] - Y'^2 would cancel.  Its batches are gathered in two halves of at most four entries, so that at most
// 3 x 4 float4 loads are in flight per lane.  dt_rows is the one cross-lane sum: a fixed xor tree over the row's 8 lanes.
// No LDS, no barrier, no atomics; every sum in a fixed order: two runs give the same bits.
//
// Resource usage of the vector kernels (hipcc -O3 -Rpass-analysis=kernel-resource-usage, gfx950): scratch 0 bytes and LDS 0 bytes
// in every one, no AGPRs; VGPRs (waves per SIMD):
//   gather_softmax_kernel<msg>      100 (4)      gather_softmax_kernel<plain>      114 (4)
//   gather_softmax_bwd_kernel<msg>  126 (4)      gather_softmax_bwd_kernel<plain>  126 (4)
#include "row_gather.h"

namespace {

constexpr float kLog2e = 1.44269504088896340736f, kLn2 = 0.69314718055994530942f;

struct SmaxFwd {
    const float* H;
    int64_t ldh;
    const float* R;
    int64_t ldr;
    float t, eps;
    float* Y;
    int64_t ldy;
    float* lse;
    int64_t ldl;
};

struct SmaxBwd {
    const float* dO;
    int64_t lddo;
    const float* H;
    int64_t ldh;
    const float* Yp;
    int64_t ldyp;
    const float* lse;
    int64_t ldl;
    float t, eps;
    float* dH;
    int64_t lddh;
    float* dR;
    int64_t lddr;
    float* dt;
    int add_dout;
};

template <bool kMsg>
__device__ __forceinline__ float msg1(float h, float eps) {
    return kMsg ? __fadd_rn(fmaxf(h, 0.f), eps) : h;
}
template <bool kMsg>
__device__ __forceinline__ float4 msg4(float4 h, float eps) {
    return make_float4(msg1<kMsg>(h.x, eps), msg1<kMsg>(h.y, eps), msg1<kMsg>(h.z, eps), msg1<kMsg>(h.w, eps));
}
__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }       // x <= 0 (or tiny): one v_exp_f32

// pass 1 of a batch element: x <- d = x - K, bm <- max(bm, t' d)
__device__ __forceinline__ void shift_max(float& x, float k, float t2, float& bm) {
    x = __fsub_rn(x, k);
    bm = fmaxf(bm, __fmul_rn(t2, x));
}
// the once-per-batch rescale of one channel's running state to the new maximum (mx = -inf before the first batch: the factor is 0)
__device__ __forceinline__ void rescale(float& mx, float& den, float& num, float bm) {
    const float nm = fmaxf(mx, bm);
    const float sc = exp2_hw(__fsub_rn(mx, nm));
    den *= sc;
    num *= sc;
    mx = nm;
}
// pass 2: p = f 2^(t' d - mx), den += p, num += p d
__device__ __forceinline__ void accum(float d, float f, float t2, float mx, float& den, float& num) {
    const float p = f * exp2_hw(__fsub_rn(__fmul_rn(t2, d), mx));
    den += p;
    num = fmaf(p, d, num);
}
// the epilogue of one channel on a row with entries -> Y (without root), lse
__device__ __forceinline__ void finish(float k, float mx, float den, float num, float t, float& y, float& l) {
    y = __fadd_rn(k, num / den);
    l = fmaf(t, k, kLn2 * (mx + __log2f(den)));
}

// ------------------------------------------------------------------------------------------------ forward
template <bool kMsg>
__global__ __launch_bounds__(256) void gather_softmax_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                             const float* __restrict__ mult, SmaxFwd p, int n_rows, int C,
                                                             int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float t2 = p.t * kLog2e, ninf = -__builtin_huge_valf();
    const bool hr = p.R != nullptr;
    FOR_CHUNK_ROW_ENTRIES {
        for (int q = sl; q < W; q += 8) {
            const float4 r = hr ? ld4(p.R + (int64_t)row * p.ldr + q * 4) : zero4;
            float4 y = r, l = zero4;                              // (a row without entries: the root row bit for bit, lse 0)
            if (nn > 0) {
                const float4 k0 = msg4<kMsg>(ld4(p.H + (int64_t)col[rbase] * p.ldh + q * 4), p.eps);
                float4 mx = make_float4(ninf, ninf, ninf, ninf), den = zero4, num = zero4;
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
                            const float a = mult[e];
                            f[k] = b0 + k < nn ? a : 0.f;         // (a re-read last entry adds nothing)
                        }
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = ld4(p.H + (int64_t)j[k] * p.ldh + q * 4);
                        float4 bm = make_float4(ninf, ninf, ninf, ninf);
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            x[k] = msg4<kMsg>(x[k], p.eps);
                            shift_max(x[k].x, k0.x, t2, bm.x);
                            shift_max(x[k].y, k0.y, t2, bm.y);
                            shift_max(x[k].z, k0.z, t2, bm.z);
                            shift_max(x[k].w, k0.w, t2, bm.w);
                        }
                        rescale(mx.x, den.x, num.x, bm.x);
                        rescale(mx.y, den.y, num.y, bm.y);
                        rescale(mx.z, den.z, num.z, bm.z);
                        rescale(mx.w, den.w, num.w, bm.w);
#pragma unroll
                        for (int k = 0; k < NE; ++k) {
                            accum(x[k].x, f[k], t2, mx.x, den.x, num.x);
                            accum(x[k].y, f[k], t2, mx.y, den.y, num.y);
                            accum(x[k].z, f[k], t2, mx.z, den.z, num.z);
                            accum(x[k].w, f[k], t2, mx.w, den.w, num.w);
                        }
                    };
                    ROW_BATCH_SWITCH(b0, nn, batch)
                }
                finish(k0.x, mx.x, den.x, num.x, p.t, y.x, l.x);
                finish(k0.y, mx.y, den.y, num.y, p.t, y.y, l.y);
                finish(k0.z, mx.z, den.z, num.z, p.t, y.z, l.z);
                finish(k0.w, mx.w, den.w, num.w, p.t, y.w, l.w);
                if (hr) y.x = __fadd_rn(r.x, y.x), y.y = __fadd_rn(r.y, y.y), y.z = __fadd_rn(r.z, y.z), y.w = __fadd_rn(r.w, y.w);
            }
            *reinterpret_cast<float4*>(p.Y + (int64_t)row * p.ldy + q * 4) = y;
            if (p.lse) *reinterpret_cast<float4*>(p.lse + (int64_t)row * p.ldl + q * 4) = l;
        }
    }
}

// one thread per row: an exact two-pass softmax per channel (maximum, then sums), the same shifted form
template <bool kMsg>
__global__ __launch_bounds__(256) void gather_softmax_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                    const float* __restrict__ mult, SmaxFwd p, int n_rows, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    const float t2 = p.t * kLog2e;
    for (int c = 0; c < C; ++c) {
        const float r = p.R ? p.R[(int64_t)row * p.ldr + c] : 0.f;
        float y = r, l = 0.f;
        if (e1 > e0) {
            const float k0 = msg1<kMsg>(p.H[(int64_t)col[e0] * p.ldh + c], p.eps);
            float mx = -__builtin_huge_valf(), den = 0.f, num = 0.f;
            for (int e = e0; e < e1; ++e) {
                float x = msg1<kMsg>(p.H[(int64_t)col[e] * p.ldh + c], p.eps);
                shift_max(x, k0, t2, mx);
            }
            for (int e = e0; e < e1; ++e)
                accum(__fsub_rn(msg1<kMsg>(p.H[(int64_t)col[e] * p.ldh + c], p.eps), k0), mult[e], t2, mx, den, num);
            finish(k0, mx, den, num, p.t, y, l);
            if (p.R) y = __fadd_rn(r, y);
        }
        p.Y[(int64_t)row * p.ldy + c] = y;
        if (p.lse) p.lse[(int64_t)row * p.ldl + c] = l;
    }
}

// ------------------------------------------------------------------------------------------------ backward (node side)
// one entry of one channel: g = w p dOut, s += g, r += g (m - Y')
__device__ __forceinline__ void bwd1(float tm, float m, float w, float d, float yp, float l, float& s, float& r) {
    const float g = w * exp2_hw(kLog2e * __fsub_rn(tm, l)) * d;
    s += g;
    r = fmaf(g, __fsub_rn(m, yp), r);
}

template <bool kMsg>
__global__ __launch_bounds__(256) void gather_softmax_bwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                 const int* __restrict__ mirror, const float* __restrict__ mult,
                                                                 SmaxBwd p, int n_rows, int C, int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    FOR_CHUNK_ROW_ENTRIES {
        if (p.dR)
            for (int q = sl; q < W; q += 8)
                *reinterpret_cast<float4*>(p.dR + (int64_t)row * p.lddr + q * 4) = ld4(p.dO + (int64_t)row * p.lddo + q * 4);
        float dt = 0.f;
        for (int q = sl; q < W; q += 8) {
            const float4 h = ld4(p.H + (int64_t)row * p.ldh + q * 4);
            const float4 m = msg4<kMsg>(h, p.eps);
            const float4 tm = make_float4(__fmul_rn(p.t, m.x), __fmul_rn(p.t, m.y), __fmul_rn(p.t, m.z), __fmul_rn(p.t, m.w));
            float4 s = zero4, r = zero4;
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    int j[NE];
                    float w[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int e = rbase + min(b0 + k, nn - 1);
                        j[k] = col[e];
                        const float a = mult[mirror[e]];
                        w[k] = b0 + k < nn ? a : 0.f;             // (a re-read last entry adds nothing)
                    }
                    auto half = [&](auto k0_tag, auto np_tag) {
                        constexpr int K0 = decltype(k0_tag)::value, NP = decltype(np_tag)::value;
                        float4 d[NP], y[NP], l[NP];
#pragma unroll
                        for (int k = 0; k < NP; ++k) {
                            d[k] = ld4(p.dO + (int64_t)j[K0 + k] * p.lddo + q * 4);
                            y[k] = ld4(p.Yp + (int64_t)j[K0 + k] * p.ldyp + q * 4);
                            l[k] = ld4(p.lse + (int64_t)j[K0 + k] * p.ldl + q * 4);
                        }
#pragma unroll
                        for (int k = 0; k < NP; ++k) {
                            bwd1(tm.x, m.x, w[K0 + k], d[k].x, y[k].x, l[k].x, s.x, r.x);
                            bwd1(tm.y, m.y, w[K0 + k], d[k].y, y[k].y, l[k].y, s.y, r.y);
                            bwd1(tm.z, m.z, w[K0 + k], d[k].z, y[k].z, l[k].z, s.z, r.z);
                            bwd1(tm.w, m.w, w[K0 + k], d[k].w, y[k].w, l[k].w, s.w, r.w);
                        }
                    };
                    half(std::integral_constant<int, 0>(), std::integral_constant<int, (NE < 4 ? NE : 4)>());
                    if constexpr (NE > 4) {
                        // (the scheduler may not pull the second half's loads in front of the first half's sums: registers)
                        __builtin_amdgcn_sched_barrier(0);
                        half(std::integral_constant<int, 4>(), std::integral_constant<int, NE - 4>());
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
            float4 g = make_float4(fmaf(p.t, r.x, s.x), fmaf(p.t, r.y, s.y), fmaf(p.t, r.z, s.z), fmaf(p.t, r.w, s.w));
            if (kMsg) g.x = h.x > 0.f ? g.x : 0.f, g.y = h.y > 0.f ? g.y : 0.f, g.z = h.z > 0.f ? g.z : 0.f, g.w = h.w > 0.f ? g.w : 0.f;
            if (p.add_dout) {
                const float4 d = ld4(p.dO + (int64_t)row * p.lddo + q * 4);
                g.x = __fadd_rn(d.x, g.x), g.y = __fadd_rn(d.y, g.y), g.z = __fadd_rn(d.z, g.z), g.w = __fadd_rn(d.w, g.w);
            }
            *reinterpret_cast<float4*>(p.dH + (int64_t)row * p.lddh + q * 4) = g;
            dt = dot4(m, r, dt);
        }
        if (p.dt) {
            dt = red_sum(dt, 8);
            if (sl == 0) p.dt[row] = dt;
        }
    }
}

template <bool kMsg>
__global__ __launch_bounds__(256) void gather_softmax_bwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                        const int* __restrict__ mirror,
                                                                        const float* __restrict__ mult, SmaxBwd p, int n_rows,
                                                                        int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float dt = 0.f;
    for (int c = 0; c < C; ++c) {
        if (p.dR) p.dR[(int64_t)row * p.lddr + c] = p.dO[(int64_t)row * p.lddo + c];
        const float h = p.H[(int64_t)row * p.ldh + c], m = msg1<kMsg>(h, p.eps), tm = __fmul_rn(p.t, m);
        float s = 0.f, r = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int64_t i = col[e];
            bwd1(tm, m, mult[mirror[e]], p.dO[i * p.lddo + c], p.Yp[i * p.ldyp + c], p.lse[i * p.ldl + c], s, r);
        }
        float g = (kMsg && !(h > 0.f)) ? 0.f : fmaf(p.t, r, s);
        if (p.add_dout) g = __fadd_rn(p.dO[(int64_t)row * p.lddo + c], g);
        p.dH[(int64_t)row * p.lddh + c] = g;
        dt = fmaf(m, r, dt);
    }
    if (p.dt) p.dt[row] = dt;
}

// the attention graph WITHOUT loop handling: a_e counts the input edges of entry e
inline bool smax_graph_ok(const ddmp_graph* g) { return attn_graph_ok(g) && g->valued == DDMP_GV_VALUED; }
inline bool finite_f(float v) { return v == v && v - v == 0.f; }

template <bool kMsg>
int launch_fwd(hipStream_t st, const ddmp_graph* g, bool vec, const SmaxFwd& p, int C) {
    return launch_rows(st, (int)g->n_rows, vec, gather_softmax_kernel<kMsg>, gather_softmax_scalar_kernel<kMsg>, g->rowptr, g->col,
                       g->a, p, (int)g->n_rows, C);
}
template <bool kMsg>
int launch_bwd(hipStream_t st, const ddmp_graph* g, bool vec, const SmaxBwd& p, int C) {
    return launch_rows(st, (int)g->n_rows, vec, gather_softmax_bwd_kernel<kMsg>, gather_softmax_bwd_scalar_kernel<kMsg>, g->rowptr,
                       g->col, g->mirror, g->a, p, (int)g->n_rows, C);
}

}  // namespace

extern "C" int ddmp_gather_softmax_f32(const ddmp_graph* g, const float* H, int64_t ldh, int C, float t, int has_eps, float msg_eps,
                                       const float* R, int64_t ldr, float* Y, int64_t ldy, float* lse, int64_t ldl,
                                       ddmp_stream stream) {
    ARG_TRY(smax_graph_ok(g) && H && Y && C >= 1 && ldh >= C && ldy >= C && wide(R, ldr, C) && wide(lse, ldl, C) && finite_f(t) &&
            (!has_eps || (finite_f(msg_eps) && msg_eps >= 0.f)) && Y != H && Y != R && Y != lse && lse != H && (!lse || lse != R));
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(H, ldh) && vec_ok(R, ldr) && vec_ok(Y, ldy) && vec_ok(lse, ldl);
    const SmaxFwd p{H, ldh, R, ldr, t, has_eps ? msg_eps : 0.f, Y, ldy, lse, ldl};
    return has_eps ? launch_fwd<true>((hipStream_t)stream, g, vec, p, C) : launch_fwd<false>((hipStream_t)stream, g, vec, p, C);
}

extern "C" int ddmp_gather_softmax_bwd_f32(const ddmp_graph* g, int C, const float* dOut, int64_t lddo, const float* H, int64_t ldh,
                                           const float* Yp, int64_t ldyp, const float* lse, int64_t ldl, float t, int has_eps,
                                           float msg_eps, int add_dout, float* dH, int64_t lddh, float* dR, int64_t lddr,
                                           float* dt_rows, ddmp_stream stream) {
    ARG_TRY(smax_graph_ok(g) && dOut && H && Yp && lse && dH && C >= 1 && lddo >= C && ldh >= C && ldyp >= C && ldl >= C && lddh >= C &&
            wide(dR, lddr, C) && finite_f(t) && (!has_eps || (finite_f(msg_eps) && msg_eps >= 0.f)) && dH != dOut && dH != H &&
            dH != Yp && dH != lse && dH != dR && dH != dt_rows && (!dR || (dR != dOut && dR != H && dR != Yp && dR != lse && dR != dt_rows)) &&
            (!dt_rows || (dt_rows != dOut && dt_rows != H && dt_rows != Yp && dt_rows != lse)));
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && vec_ok(dOut, lddo) && vec_ok(H, ldh) && vec_ok(Yp, ldyp) && vec_ok(lse, ldl) && vec_ok(dH, lddh) &&
                     vec_ok(dR, lddr);
    const SmaxBwd p{dOut, lddo, H, ldh, Yp, ldyp, lse, ldl, t, has_eps ? msg_eps : 0.f, dH, lddh, dR, lddr, dt_rows, add_dout};
    return has_eps ? launch_bwd<true>((hipStream_t)stream, g, vec, p, C) : launch_bwd<false>((hipStream_t)stream, g, vec, p, C);
}

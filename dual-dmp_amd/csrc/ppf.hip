// Max aggregation of an edge-conditioned message with its winner (PPFConv): the point-pair features of the
// coalesced entries, the fused arg-max gather over B[col e] + F[e] E, and its one-launch backward.
//
//   F[e,:]   = [ |d|, angle(n_i, d), angle(n_j, d), angle(n_i, n_j) ],  d = pos_j - pos_i,  angle(a, b) = atan2(|a x b|, a . b),
//              for the entry e = (i, j = col e); exactly 0 for j == i
//   Y[i,c]   = max_{e in row i} msg(e, c),   arg[i,c] = col e of the winning entry      (a row without entries: 0 and -1)
//   msg(e,c) = fma(F[e,3], E[3,c], fma(F[e,2], E[2,c], fma(F[e,1], E[1,c], F[e,0] * E[0,c]))) + B[col e, c]     -- THIS order
//   dB[j,c]  = sum_{e' in row j} (arg[col e', c] == j ? dG[col e', c] : 0)
//   P[r,d,c] = sum over the rows i of the 8-row group r = i >> 3 of dG[i,c] F[entry(i, arg[i,c]), d]        (column sum over r: dE)
//
// over the COALESCED CSR of a valued graph (gmax.hip's graph; the entries kernel also reads its mirror map: the row of entry e is
// col[mirror[e]]).  The backward relies on the SYMMETRIC structure like gmax.hip's.  Ties go to the first entry in CSR order: the
// running maximum starts at the row's first entry and is replaced on a strict > only.
// On the row-gather layout (row_gather.h) without heads.  Forward: a lane holds kNQ column slabs (float4) at once -- the E rows
// of those columns, the running maxima and their ids stay in registers over ALL entries of the row -- and F[e], one float4 per
// entry, is loaded once per batch slot for all of them (kNQ = 2 covers C <= 64 in one pass; wider rows take further passes).
// Backward: ONE walk of row r's entries serves both sides -- the node side is gmax.hip's sum, the row side SELECTS, per column,
// the F of the entry whose id equals arg[r,c] (a selection, not a sum: exact) and multiplies by dG[r,c] once.
// The row side leaves the kernel per 8-ROW GROUP, not per row: the 8 row groups of a wave step are the consecutive rows
// 8 (r >> 3) .. + 7, the lanes l, l ^ 8, l ^ 16, l ^ 32 hold the same columns of those rows and are summed by the fixed xor tree
// over lane bits 3-5 (group8_sum: the pairings of __shfl_xor by 8, 16, 32 in that order), and row group 0 stores.  ALL 64 LANES
// MUST TAKE PART IN THAT TREE: the backward therefore does NOT use FOR_CHUNK_ROWS, whose `if (lr < nr)` leaves the lanes of a row
// beyond n out of everything behind it.  It leaves a wave step only when ALL of its 8 rows are beyond n (wave-uniform); a row
// group whose row is beyond n, a row without entries and a lane whose slab is beyond C run with zero entries, contribute zeros and
// store nothing, and the tree stands outside the (per-row-group divergent) entry loop.
// No LDS, no barrier, no atomics.
#include "row_gather.h"

namespace {

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// a b - c d as a compensated difference of products (Kahan): w = rn(c d), its rounding error fma(-c, d, w) is exact
__device__ __forceinline__ float diff_of_products(float a, float b, float c, float d) {
    const float w = __fmul_rn(c, d);
    return __fadd_rn(fmaf(a, b, -w), fmaf(-c, d, w));
}
__device__ __forceinline__ float angle3(float ax, float ay, float az, float bx, float by, float bz) {
    const float cx = diff_of_products(ay, bz, az, by);
    const float cy = diff_of_products(az, bx, ax, bz);
    const float cz = diff_of_products(ax, by, ay, bx);
    const float s = sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
    const float c = fmaf(az, bz, fmaf(ay, by, ax * bx));
    return atan2f(s, c);
}

// ------------------------------------------------------------------------------------------------ the features, one thread per entry
__global__ __launch_bounds__(256) void ppf_entries_kernel(const int* __restrict__ col, const int* __restrict__ mirror,
                                                          const float* __restrict__ pos, int64_t ldp,
                                                          const float* __restrict__ nrm, int64_t ldn, float* __restrict__ F,
                                                          int64_t n_entries) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_entries) return;
    const int j = col[e], i = col[mirror[e]];
    float4 f = zero4();
    if (j != i) {                                                 // (a loop: exactly 0, nothing evaluated)
        const float* pi = pos + (int64_t)i * ldp;
        const float* pj = pos + (int64_t)j * ldp;
        const float* ni = nrm + (int64_t)i * ldn;
        const float* nj = nrm + (int64_t)j * ldn;
        const float dx = pj[0] - pi[0], dy = pj[1] - pi[1], dz = pj[2] - pi[2];
        const float nix = ni[0], niy = ni[1], niz = ni[2], njx = nj[0], njy = nj[1], njz = nj[2];
        f.x = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        f.y = angle3(nix, niy, niz, dx, dy, dz);
        f.z = angle3(njx, njy, njz, dx, dy, dz);
        f.w = angle3(nix, niy, niz, njx, njy, njz);
    }
    float* o = F + e * 4;
    o[0] = f.x, o[1] = f.y, o[2] = f.z, o[3] = f.w;               // (adjacent dwords of one lane: one 16-byte store where F is aligned)
}

// ------------------------------------------------------------------------------------------------ forward
__device__ __forceinline__ float msg1(float f0, float f1, float f2, float f3, float e0, float e1, float e2, float e3, float b) {
    return __fadd_rn(fmaf(f3, e3, fmaf(f2, e2, fmaf(f1, e1, __fmul_rn(f0, e0)))), b);
}
__device__ __forceinline__ float4 msg4(float4 f, float4 e0, float4 e1, float4 e2, float4 e3, float4 b) {
    return make_float4(msg1(f.x, f.y, f.z, f.w, e0.x, e1.x, e2.x, e3.x, b.x), msg1(f.x, f.y, f.z, f.w, e0.y, e1.y, e2.y, e3.y, b.y),
                       msg1(f.x, f.y, f.z, f.w, e0.z, e1.z, e2.z, e3.z, b.z), msg1(f.x, f.y, f.z, f.w, e0.w, e1.w, e2.w, e3.w, b.w));
}

template <int kNQ, bool kHasB>
__global__ __launch_bounds__(256) void gather_max_attr_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                              const float* __restrict__ B, int64_t ldb, const float* __restrict__ F,
                                                              const float* __restrict__ E, float* __restrict__ Y, int64_t ldy,
                                                              int* __restrict__ arg, int64_t ldg, int n_rows, int C,
                                                              int chunks_per_xcd, int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    const float4* F4 = reinterpret_cast<const float4*>(F);
    FOR_CHUNK_ROW_ENTRIES {
        float* yrow = Y + (int64_t)row * ldy;
        int* grow = arg ? arg + (int64_t)row * ldg : nullptr;
        if (nn == 0) {
            for (int q = sl; q < W; q += 8) {
                *reinterpret_cast<float4*>(yrow + q * 4) = zero4();
                if (grow) *reinterpret_cast<int4*>(grow + q * 4) = make_int4(-1, -1, -1, -1);
            }
            continue;
        }
        const int j0 = col[rbase];
        const float4 f0 = F4[rbase];
        for (int qb = sl; qb < W; qb += 8 * kNQ) {               // a pass: the lane's slabs qb, qb + 8 ... (a slab beyond W runs slab qb
            int qc[kNQ];                                         // again and stores nothing)
            float4 e0[kNQ], e1[kNQ], e2[kNQ], e3[kNQ], m[kNQ];
            int4 id[kNQ];
#pragma unroll
            for (int s = 0; s < kNQ; ++s) {
                qc[s] = qb + 8 * s < W ? qb + 8 * s : qb;
                e0[s] = ld4(E + qc[s] * 4), e1[s] = ld4(E + C + qc[s] * 4);
                e2[s] = ld4(E + 2 * C + qc[s] * 4), e3[s] = ld4(E + 3 * C + qc[s] * 4);
                m[s] = msg4(f0, e0[s], e1[s], e2[s], e3[s], kHasB ? ld4(B + (int64_t)j0 * ldb + qc[s] * 4) : zero4());
                id[s] = make_int4(j0, j0, j0, j0);
            }
#pragma unroll 1
            for (int b0 = 0; b0 < nn; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    int j[NE];
                    float4 f[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int e = rbase + min(b0 + k, nn - 1);
                        j[k] = col[e];
                        f[k] = F4[e];                            // once per batch slot, for every slab of the pass
                    }
#pragma unroll
                    for (int s = 0; s < kNQ; ++s) {
                        float4 x[NE];
#pragma unroll
                        for (int k = 0; k < NE; ++k) x[k] = kHasB ? ld4(B + (int64_t)j[k] * ldb + qc[s] * 4) : zero4();
#pragma unroll
                        for (int k = 0; k < NE; ++k) {           // (a shorter row's re-read last entry cannot win a strict >)
                            const float4 t = msg4(f[k], e0[s], e1[s], e2[s], e3[s], x[k]);
                            take_gt(m[s].x, id[s].x, t.x, j[k]);
                            take_gt(m[s].y, id[s].y, t.y, j[k]);
                            take_gt(m[s].z, id[s].z, t.z, j[k]);
                            take_gt(m[s].w, id[s].w, t.w, j[k]);
                        }
                    }
                };
                ROW_BATCH_SWITCH(b0, nn, batch)
            }
#pragma unroll
            for (int s = 0; s < kNQ; ++s) {
                const int q = qb + 8 * s;
                if (q < W) {
                    *reinterpret_cast<float4*>(yrow + q * 4) = m[s];
                    if (grow) *reinterpret_cast<int4*>(grow + q * 4) = id[s];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void gather_max_attr_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                     const float* __restrict__ B, int64_t ldb,
                                                                     const float* __restrict__ F, const float* __restrict__ E,
                                                                     float* __restrict__ Y, int64_t ldy, int* __restrict__ arg,
                                                                     int64_t ldg, int n_rows, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    float* yrow = Y + (int64_t)row * ldy;
    int* grow = arg ? arg + (int64_t)row * ldg : nullptr;
    for (int c = 0; c < C; ++c) {
        const float w0 = E[c], w1 = E[C + c], w2 = E[2 * C + c], w3 = E[3 * C + c];
        float m = 0.f;
        int id = -1;
        for (int e = e0; e < e1; ++e) {
            const int j = col[e];
            const float* f = F + (int64_t)e * 4;
            const float t = msg1(f[0], f[1], f[2], f[3], w0, w1, w2, w3, B ? B[(int64_t)j * ldb + c] : 0.f);
            if (e == e0) m = t, id = j;
            else take_gt(m, id, t, j);
        }
        yrow[c] = m;
        if (grow) grow[c] = id;
    }
}

// ------------------------------------------------------------------------------------------------ backward
template <bool kParts>
__global__ __launch_bounds__(256) void gather_max_attr_bwd_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                  const float* __restrict__ dG, int64_t lddg,
                                                                  const int* __restrict__ arg, int64_t ldg,
                                                                  const float* __restrict__ F, float* __restrict__ dB, int64_t lddb,
                                                                  float* __restrict__ P, int n_rows, int C, int chunks_per_xcd,
                                                                  int n_chunks) {
    ROW_CHUNK_PROLOGUE
    const int W = C >> 2;
    const float4* F4 = reinterpret_cast<const float4*>(F);
#pragma unroll 1
    for (int qq = 0; qq < 2; ++qq) {
        const int lr0 = wave * 8 + qq * 32;                       // the first of the wave step's 8 consecutive rows
        if (lr0 >= nr) break;                                     // wave-uniform: all 8 rows are beyond n
        const bool live = lr0 + grp < nr;
        const int row = r0 + (live ? lr0 + grp : lr0);
        const int rbase = rowptr[row], nn = live ? rowptr[row + 1] - rbase : 0;
        float* prow = kParts ? P + (int64_t)((r0 + lr0) >> 3) * 4 * C : nullptr;
#pragma unroll 1
        for (int qb = 0; qb < W; qb += 8) {                       // the same trip count in every lane
            const int q = qb + sl;
            const bool mine = q < W && nn > 0;                    // else: zero entries, zeros into the tree, no gathered load
            const int ne = mine ? nn : 0;
            float4 acc = zero4(), g = zero4(), s0 = zero4(), s1 = zero4(), s2 = zero4(), s3 = zero4();
            int4 own = make_int4(-2, -2, -2, -2);
            if (kParts && mine) {
                g = ld4(dG + (int64_t)row * lddg + q * 4);
                own = ld4i(arg + (int64_t)row * ldg + q * 4);
            }
#pragma unroll 1
            for (int b0 = 0; b0 < ne; b0 += kEB) {
                auto batch = [&](auto ne_tag) {
                    constexpr int NE = decltype(ne_tag)::value;
                    int j[NE];
                    float4 f[NE];
                    int4 w[NE];
                    float4 x[NE];
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int e = rbase + min(b0 + k, ne - 1);
                        j[k] = col[e];
                        if (kParts) f[k] = F4[e];
                    }
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        w[k] = ld4i(arg + (int64_t)j[k] * ldg + q * 4);
                        x[k] = ld4(dG + (int64_t)j[k] * lddg + q * 4);
                    }
#pragma unroll
                    for (int k = 0; k < NE; ++k) {
                        const int me = b0 + k < ne ? row : -2;            // (a re-read last entry adds nothing; arg >= -1)
                        acc.x += w[k].x == me ? x[k].x : 0.f;
                        acc.y += w[k].y == me ? x[k].y : 0.f;
                        acc.z += w[k].z == me ? x[k].z : 0.f;
                        acc.w += w[k].w == me ? x[k].w : 0.f;
                        if (kParts) {                                     // (re-selecting the re-read last entry changes nothing)
                            const bool hx = own.x == j[k], hy = own.y == j[k], hz = own.z == j[k], hw = own.w == j[k];
                            s0.x = hx ? f[k].x : s0.x, s1.x = hx ? f[k].y : s1.x, s2.x = hx ? f[k].z : s2.x, s3.x = hx ? f[k].w : s3.x;
                            s0.y = hy ? f[k].x : s0.y, s1.y = hy ? f[k].y : s1.y, s2.y = hy ? f[k].z : s2.y, s3.y = hy ? f[k].w : s3.y;
                            s0.z = hz ? f[k].x : s0.z, s1.z = hz ? f[k].y : s1.z, s2.z = hz ? f[k].z : s2.z, s3.z = hz ? f[k].w : s3.z;
                            s0.w = hw ? f[k].x : s0.w, s1.w = hw ? f[k].y : s1.w, s2.w = hw ? f[k].z : s2.w, s3.w = hw ? f[k].w : s3.w;
                        }
                    }
                };
                ROW_BATCH_SWITCH(b0, ne, batch)
            }
            if (live && q < W) *reinterpret_cast<float4*>(dB + (int64_t)row * lddb + q * 4) = acc;
            if (kParts) {                                         // all 64 lanes: the 8 rows' shares, summed over lane bits 3-5
                float4 p[4] = {s0, s1, s2, s3};
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    p[d].x = group8_sum(__fmul_rn(g.x, p[d].x));
                    p[d].y = group8_sum(__fmul_rn(g.y, p[d].y));
                    p[d].z = group8_sum(__fmul_rn(g.z, p[d].z));
                    p[d].w = group8_sum(__fmul_rn(g.w, p[d].w));
                    if (grp == 0 && q < W) *reinterpret_cast<float4*>(prow + d * C + q * 4) = p[d];
                }
            }
        }
    }
}

template <bool kParts>
__global__ __launch_bounds__(256) void gather_max_attr_bwd_scalar_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                         const float* __restrict__ dG, int64_t lddg,
                                                                         const int* __restrict__ arg, int64_t ldg,
                                                                         const float* __restrict__ F, float* __restrict__ dB,
                                                                         int64_t lddb, float* __restrict__ P, int n_rows, int C) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    for (int c = 0; c < C; ++c) {
        float acc = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int64_t j = col[e];
            acc += arg[j * ldg + c] == row ? dG[j * lddg + c] : 0.f;
        }
        dB[(int64_t)row * lddb + c] = acc;
    }
    if (!kParts || (row & 7)) return;
    // the 8-row group's shares by a plain loop, rows in ascending order (the thread of the group's first row)
    float* prow = P + (int64_t)(row >> 3) * 4 * C;
    const int rend = min(row + 8, n_rows);
    for (int c = 0; c < C; ++c) {
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
        for (int r = row; r < rend; ++r) {
            const int a = arg[(int64_t)r * ldg + c];
            const float gv = dG[(int64_t)r * lddg + c];
            for (int e = rowptr[r]; e < rowptr[r + 1]; ++e)
                if (col[e] == a) {
                    const float* f = F + (int64_t)e * 4;
                    p0 += gv * f[0], p1 += gv * f[1], p2 += gv * f[2], p3 += gv * f[3];
                    break;
                }
        }
        prow[c] = p0, prow[C + c] = p1, prow[2 * C + c] = p2, prow[3 * C + c] = p3;
    }
}

}  // namespace

extern "C" int ddmp_ppf_entries_f32(const ddmp_graph* g, const float* pos, int64_t ldp, const float* normal, int64_t ldn, float* F,
                                    ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g) && pos && normal && F && ldp >= 3 && ldn >= 3 && F != pos && F != normal && g->nnz < (int64_t)INT32_MAX);
    if (g->nnz == 0) return DDMP_OK;
    hipLaunchKernelGGL(ppf_entries_kernel, dim3((unsigned)cdiv(g->nnz, 256)), dim3(256), 0, (hipStream_t)stream, g->col, g->mirror,
                       pos, ldp, normal, ldn, F, g->nnz);
    LAUNCH_TRY();
    return DDMP_OK;
}

extern "C" int ddmp_gather_max_attr_f32(const ddmp_graph* g, const float* B, int64_t ldb, const float* F, const float* E, int C,
                                        float* Y, int64_t ldy, int32_t* arg, int64_t ldarg, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g, false) && F && E && Y && C >= 1 && wide(B, ldb, C) && ldy >= C && wide(arg, ldarg, C) && Y != B && Y != F &&
            Y != E && (const void*)arg != (const void*)F && (const void*)arg != (const void*)E && (const void*)arg != (const void*)B &&
            (const void*)arg != (const void*)Y);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && ldy % 4 == 0 && al16(Y) && al16(F) && al16(E) && vec_ok(B, ldb) && vec_ok(arg, ldarg);
    const hipStream_t st = (hipStream_t)stream;
    const int n = (int)g->n_rows;
    auto go = [&](auto vk) {
        return launch_rows(st, n, vec, vk, gather_max_attr_scalar_kernel, g->rowptr, g->col, B, ldb, F, E, Y, ldy, arg, ldarg, n, C);
    };
    if (C > 32) return B ? go(gather_max_attr_kernel<2, true>) : go(gather_max_attr_kernel<2, false>);
    return B ? go(gather_max_attr_kernel<1, true>) : go(gather_max_attr_kernel<1, false>);
}

extern "C" int ddmp_gather_max_attr_bwd_f32(const ddmp_graph* g, const float* dG, int64_t lddg, const int32_t* arg, int64_t ldarg,
                                            const float* F, int C, float* dB, int64_t lddb, float* P, ddmp_stream stream) {
    ARG_TRY(attn_graph_ok(g, false) && dG && arg && F && dB && C >= 1 && lddg >= C && ldarg >= C && lddb >= C && dB != dG && dB != F &&
            (const void*)dB != (const void*)arg && P != dG && P != F && P != dB && (const void*)P != (const void*)arg);
    if (g->n_rows == 0) return DDMP_OK;
    const bool vec = C % 4 == 0 && lddg % 4 == 0 && ldarg % 4 == 0 && lddb % 4 == 0 && al16(dG) && al16(arg) && al16(F) && al16(dB) &&
                     (!P || al16(P));
    const hipStream_t st = (hipStream_t)stream;
    const int n = (int)g->n_rows;
    if (P)
        return launch_rows(st, n, vec, gather_max_attr_bwd_kernel<true>, gather_max_attr_bwd_scalar_kernel<true>, g->rowptr, g->col, dG,
                           lddg, arg, ldarg, F, dB, lddb, P, n, C);
    return launch_rows(st, n, vec, gather_max_attr_bwd_kernel<false>, gather_max_attr_bwd_scalar_kernel<false>, g->rowptr, g->col, dG,
                       lddg, arg, ldarg, F, dB, lddb, P, n, C);
}

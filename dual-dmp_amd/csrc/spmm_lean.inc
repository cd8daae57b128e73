// Lean forms of the slab kernel (included by spmm.hip; float32 features, 8 lanes x float4 per 128-byte slab).
//
// What the counters and two probes said about spmm_slab_kernel (scripts/spmm_pmc.sh, DESIGN.md 4.2):
//   * ~155 VALU wave-instructions per eight-row step and slab, half of them quarter-rate: the 64-bit `col * ldx` of every
//     gathered row (v_mul_lo_u32 x2 + v_mad_u64_u32 + v_add3 + v_lshl_add_u64 per entry and slab), clamping of a partial
//     batch, a staged / not-staged branch per entry with a serialised LDS read behind it;
//   * every load costs L1 -> register bandwidth whether it hits or not: n more guaranteed-hit loads per row cost
//     n x 72 us per million rows at C = 512 (= 28 TB/s of the 34 TB/s the 256 L1s deliver), ADDED to the streaming time.
// So (1): everything that does not depend on the slab is done once per chunk at staging time -- an entry is staged as
// (row offset in 16-byte units, weight), its address is ONE v_lshl_add_u64 on the lane's slab base, rows own fixed slots
// padded to whole quads (two ds_read_b128 per four entries, no clamping, no branch).  Same sums in the same order as
// spmm_slab_kernel.  (2) is NOT solved: sharing fetched rows between four consecutive output rows (a cluster kernel on
// precomputed distinct-column lists: 4.4 instead of 7 loads per row on the vertex graph) needs 92-116 registers for its
// four accumulators + weights and runs at 4-5 waves per SIMD instead of 8 -- measured slower (573 vs 544 us on the vertex
// graph, 970 vs 869 on the face graph at C = 512; profiles/r02_experiments/spmm_cluster_prototype.txt).
// The row's quad count and dinv[row] are staged in TWO arrays on purpose: packed in one 64-bit LDS word, the epilogue's
// v_pk_fma_f32 ... op_sel:[0,1,0] on the ds_read_b64 pair returned 0 in its low lane for 16 lanes at a time whenever the f16x3
// panel GEMM ran on the same CUs from a second stream (tests/test_gpu_kernels.py::test_spmm_forms_are_bit_stable_beside_panel_gemm).
// RED: 0 nothing | 1 the BatchNorm-backward reductions of the output (BnRed) | 2 the BatchNorm STATISTICS of the output (round 3:
// transform-first layers, forward): per column sum (y - ref), sum (y - ref)^2 with ref = red.mean = a per-column reference
// close to the mean (the engine passes the previous iteration's batch mean), float32 over a wave's 16 rows, float64 from
// there on; fpartials_reduce undoes the shift.  Around ref the float32 partial sums are well conditioned whatever mean / std is.
// Round 5 -- rows of ANY length, decided per 64-row chunk: a row's slots are its own quads (no padding to the graph's longest
// row), packed one row after the other; the chunk's 64 quad counts are prefix-summed by every wave (lane = row) and thread t
// stages the slots k = t & 3, + 4, ... of row t >> 2.  A chunk whose packed slots exceed the LDS array (more than 16 entries
// per row on average -- a hub of several hundred neighbours) reads its entries from global memory instead (same sums in the
// same order; slow, correct): one hub vertex costs its own chunk, not the graph.  `chunk_list` (nullable): the chunks to
// process, one per workgroup -- the LDS-patch kernel's heavy list (ddmp_graph::heavy).
// AXP (ddmp_spmm_axpby_f32): the affine epilogue a * (gather) + b * X[row] + c * Z[row] + d * Z2[row] -- see Axpby in spmm.hip; the
// row's own operands are requested where RED = 1 requests its Yp row: before the neighbour loop.
constexpr int kLeanSlots = kRB * 16;
// EWU: the unstaged (hub-chunk) path reads the entry's factor from `ew` like the staged one -- valued graphs (DESIGN.md 4.7), whose
// factor is not dinv[col]; a separate instantiation: the unvalued kernels are unchanged.
template <bool PRO, int RED, bool BWD, bool AXP = false, bool EWU = false>
__global__ __launch_bounds__(256) void spmm_lean_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ ew, const float* __restrict__ dinv,
    const float* __restrict__ dinv_r, const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int n_rows, int C,
    const float* __restrict__ bias, const float* __restrict__ pscale, const float* __restrict__ pshift,
    float slope, int chunks_per_xcd, int n_chunks, const int* __restrict__ chunk_list, BnRed red = BnRed(),
    BnBwdGather bwd = BnBwdGather(), Axpby ax = Axpby()) {
    static_assert(!BWD || (PRO && !RED), "BWD: coefficients a, b come as the prologue's");
    static_assert(!AXP || (!PRO && !RED && !BWD), "the affine epilogue: plain gather only");
    static_assert(RED >= 0 && RED <= 2, "epilogue reduction");
    constexpr int LANES = 8, CS = 32, RPW = 8, RPB = 32;
    __shared__ int s_rowptr[kRB + 1];
    __shared__ int s_slot[kRB];                                  // (first quad of the row's slots) * 512 + its quad count
    __shared__ float s_di[kRB];                                  // dinv[row]
    __shared__ int s_perm[kRB];                                  // the chunk's rows, longest first (chunk_rank_desc)
    __shared__ __attribute__((aligned(16))) uint2 s_ent[kLeanSlots];
    __shared__ float s_part[RED ? 2 : 1][RED ? 4 : 1][8][8];     // RED: the waves' partials of a slab (see the epilogue)

    int chunk;
    if (chunk_list) {
        if ((int)blockIdx.x >= n_chunks) return;
        chunk = chunk_list[blockIdx.x];
    } else {
        chunk = (blockIdx.x & (kXcd - 1)) * chunks_per_xcd + (blockIdx.x >> 3);
        if (chunk >= n_chunks) return;
    }
    const int r0 = chunk * kRB;
    const int nr = min(kRB, n_rows - r0);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    // (round 6) a chunk's set-up is two round trips, not four: every wave reads the row pointers itself (lane = row; no LDS hop and
    // barrier before the entries can be addressed), the entries' weights come from `ew` = dinv[col[e]] beside col, not behind it
    const int rp_l = rowptr[r0 + min(lane, nr)];
    const int rp_n = rowptr[r0 + min(lane + 1, nr)];
    if (wave == 0) {
        if (lane < nr) s_rowptr[lane] = rp_l;
        if (lane == nr - 1) s_rowptr[nr] = rp_n;
    }
    const unsigned ld16 = (unsigned)(ldx >> 2);
    // every wave: quad counts of the chunk's rows (lane = row) and their exclusive prefix sum
    const int nn_l = lane < nr ? rp_n - rp_l : 0;
    const int nq_l = (nn_l + 3) >> 2;
    // regular meshes: every row of the chunk has the same quad count -- one ballot instead of the scan (six cross-lane steps on
    // the critical path of a chunk's set-up, which is what bounds the narrow widths and small meshes)
    const int nq0 = __builtin_amdgcn_readfirstlane(nq_l);
    const bool uni = __ballot(nq_l != nq0) == 0ull;
    int incl = (lane + 1) * nq0;
    if (!uni) {
        incl = nq_l;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
    }
    const int qoff_l = incl - nq_l;
    const bool staged = (uni ? 64 * nq0 : __shfl(incl, 63, 64)) * 4 <= kLeanSlots;  // (the same in every wave)
    // rows of similar length share a wave step (8 rows in lockstep): ordered by quad count, longest first
    const int rank_l = chunk_rank_desc(lane < nr ? min(nq_l, 31) : -1, lane);
    if (wave == 0) {
        s_perm[rank_l] = lane;
        if (lane < nr) {
            s_slot[lane] = staged ? qoff_l * 512 + nq_l : 0;
            s_di[lane] = dinv_r[r0 + lane];
        }
    }
    if (staged) {
        const int lr = tid >> 2;                                 // rows 16 w .. 16 w + 15 in wave w
        const int rb = __shfl(rp_l, lr, 64);
        const int nn = __shfl(nn_l, lr, 64), nq = (nn + 3) >> 2;
        const int qo = uni ? lr * nq0 : __shfl(qoff_l, lr, 64);
        for (int k = tid & 3; k < 4 * nq; k += 4) {              // padding: the row's last entry again, weight 0
            const int e = rb + min(k, nn - 1);
            s_ent[4 * qo + k] = make_uint2((unsigned)col[e] * ld16, k < nn ? __float_as_uint(ew[e]) : 0u);
        }
    }
    __syncthreads();

    const int grp = lane / LANES, sl = lane % LANES;
    // slab groups (gridDim.y > 1: small graphs, launch_lean): this workgroup walks only its share of the C / 32 slabs, so a
    // 13k-row graph (205 chunks on 256 CUs, 16 slabs each in sequence at C = 512) becomes ~1600 short workgroups
    const int slabs_per_group = (C / CS + (int)gridDim.y - 1) / (int)gridDim.y;
    const int c_begin = (int)blockIdx.y * slabs_per_group * CS, c_end = min(C, c_begin + slabs_per_group * CS);
    // this lane's rows (at most two of the chunk's 64: positions p, p + 32 of the ordered rows), -1: none
    int lrs[2];
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
        const int pos = wave * RPW + grp + qq * RPB;
        lrs[qq] = pos < nr ? s_perm[pos] : -1;
    }
    auto slabs = [&](auto staged_tag) {
    constexpr bool STAGED = decltype(staged_tag)::value;
    for (int c0 = c_begin; c0 < c_end; c0 += CS) {
        const int off = c0 + sl * 4;
        float4 ra, rb4, rmu, rrs, q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (RED == 1) {
            ra = *reinterpret_cast<const float4*>(red.scale + off);
            rb4 = *reinterpret_cast<const float4*>(red.shift + off);
            rmu = *reinterpret_cast<const float4*>(red.mean + off);
            rrs = *reinterpret_cast<const float4*>(red.rstd + off);
        }
        if (RED == 2) rmu = *reinterpret_cast<const float4*>(red.mean + off);
        float4 pa = make_float4(1.f, 1.f, 1.f, 1.f), pb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (PRO) {
            pa = *reinterpret_cast<const float4*>(pscale + off);
            pb = *reinterpret_cast<const float4*>(pshift + off);
        }
        const float4 bs = bias ? *reinterpret_cast<const float4*>(bias + off) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 k1 = make_float4(0.f, 0.f, 0.f, 0.f), k0 = k1;
        if (BWD) {
            k1 = *reinterpret_cast<const float4*>(bwd.c1 + off);
            k0 = *reinterpret_cast<const float4*>(bwd.c0 + off);
        }
        const char* xb = reinterpret_cast<const char*>(X + off);
        const char* yb = BWD ? reinterpret_cast<const char*>(bwd.Yb + off) : nullptr;
        char* ob = reinterpret_cast<char*>((AXP ? ax.Y : Y) + off);
        const unsigned ldy16 = (unsigned)(ldy >> 2);
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) {
            const int lr = lrs[qq];
            if (lr < 0) break;
            int nq, rbase = 0, nn = 0;
            const uint4* ep = nullptr;
            if (STAGED) {
                const int sq = s_slot[lr];
                nq = sq & 511;
                ep = reinterpret_cast<const uint4*>(&s_ent[4 * (sq >> 9)]);
            } else {
                rbase = s_rowptr[lr];
                nn = s_rowptr[lr + 1] - rbase;
                nq = (nn + 3) >> 2;
            }
            // (RED = 1: the row of Yp the epilogue needs does not depend on the gather -- requested before it, not behind it)
            float4 yred = make_float4(0.f, 0.f, 0.f, 0.f);
            if (RED == 1) yred = *reinterpret_cast<const float4*>(red.Yp + (int64_t)(r0 + lr) * red.ldyp + off);
            float4 ox, oz, oz2;
            if (AXP) axpby_rows(ax, X, ldx, r0 + lr, off, ox, oz, oz2);
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int q = 0; q < nq; ++q) {
                unsigned o[4];
                float w[4];
                if (STAGED) {
                    const uint4 ea = ep[2 * q], eb = ep[2 * q + 1];
                    o[0] = ea.x; o[1] = ea.z; o[2] = eb.x; o[3] = eb.z;
                    w[0] = __uint_as_float(ea.y); w[1] = __uint_as_float(ea.w);
                    w[2] = __uint_as_float(eb.y); w[3] = __uint_as_float(eb.w);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int e = rbase + min(4 * q + k, nn - 1);
                        const int c = col[e];
                        o[k] = (unsigned)c * ld16;
                        w[k] = 4 * q + k < nn ? (EWU ? ew[e] : dinv[c]) : 0.f;
                    }
                }
                float4 v[4], vy[BWD ? 4 : 1];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    v[k] = *reinterpret_cast<const float4*>(xb + ((uint64_t)o[k] << 4));
                    if (BWD) vy[BWD ? k : 0] = *reinterpret_cast<const float4*>(yb + ((uint64_t)o[k] << 4));
                }
                // the fourth piece is padding for every row of the wave on graphs of odd regular degree (vertex graph of a
                // regular mesh: 7 entries): a load costs L1 bandwidth even when it hits, so that one is skipped wave-wide
                v[3] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (BWD) vy[BWD ? 3 : 0] = v[3];
                if (__any(w[3] != 0.f)) {
                    v[3] = *reinterpret_cast<const float4*>(xb + ((uint64_t)o[3] << 4));
                    if (BWD) vy[BWD ? 3 : 0] = *reinterpret_cast<const float4*>(yb + ((uint64_t)o[3] << 4));
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float4 t = v[k];
                    if (BWD) {
                        const float4 y = vy[BWD ? k : 0];
                        t.x = fmaf(pa.x, t.x * lrelu_grad(fmaf(y.x, pa.x, pb.x), slope), fmaf(k1.x, y.x, k0.x));
                        t.y = fmaf(pa.y, t.y * lrelu_grad(fmaf(y.y, pa.y, pb.y), slope), fmaf(k1.y, y.y, k0.y));
                        t.z = fmaf(pa.z, t.z * lrelu_grad(fmaf(y.z, pa.z, pb.z), slope), fmaf(k1.z, y.z, k0.z));
                        t.w = fmaf(pa.w, t.w * lrelu_grad(fmaf(y.w, pa.w, pb.w), slope), fmaf(k1.w, y.w, k0.w));
                    } else if (PRO) {
                        t = f4_affine_lrelu(t, pa, pb, slope);
                    }
                    acc.x = fmaf(w[k], t.x, acc.x);
                    acc.y = fmaf(w[k], t.y, acc.y);
                    acc.z = fmaf(w[k], t.z, acc.z);
                    acc.w = fmaf(w[k], t.w, acc.w);
                }
            }
            const int row = r0 + lr;
            const float di = s_di[lr];
            float4 o4;
            o4.x = fmaf(acc.x, di, bs.x);
            o4.y = fmaf(acc.y, di, bs.y);
            o4.z = fmaf(acc.z, di, bs.z);
            o4.w = fmaf(acc.w, di, bs.w);
            if (AXP) o4 = axpby4(ax, acc, di, ox, oz, oz2);
            nt_store4(reinterpret_cast<float*>(ob + ((uint64_t)((unsigned)row * ldy16) << 4)), o4);
            if (RED == 2) {
                const float d0 = o4.x - rmu.x, d1 = o4.y - rmu.y, d2 = o4.z - rmu.z, d3 = o4.w - rmu.w;
                q0.x += d0; q0.y += d1; q0.z += d2; q0.w += d3;
                q1.x = fmaf(d0, d0, q1.x);
                q1.y = fmaf(d1, d1, q1.y);
                q1.z = fmaf(d2, d2, q1.z);
                q1.w = fmaf(d3, d3, q1.w);
            }
            if (RED == 1) {
                const float4 y = yred;
                const float g0 = o4.x * lrelu_grad(fmaf(y.x, ra.x, rb4.x), slope);
                const float g1 = o4.y * lrelu_grad(fmaf(y.y, ra.y, rb4.y), slope);
                const float g2 = o4.z * lrelu_grad(fmaf(y.z, ra.z, rb4.z), slope);
                const float g3 = o4.w * lrelu_grad(fmaf(y.w, ra.w, rb4.w), slope);
                q0.x += g0; q0.y += g1; q0.z += g2; q0.w += g3;
                q1.x = fmaf(g0, (y.x - rmu.x) * rrs.x, q1.x);
                q1.y = fmaf(g1, (y.y - rmu.y) * rrs.y, q1.y);
                q1.z = fmaf(g2, (y.z - rmu.z) * rrs.z, q1.z);
                q1.w = fmaf(g3, (y.w - rmu.w) * rrs.w, q1.w);
            }
        }
        if (RED) {
            // this wave's rows -> one partial per channel and wave; the four waves' partials -> ONE record per channel and 64-row
            // chunk (round 4: through LDS, summed in float64, rounded once).  With one record per wave the partial tensor was
            // 12.5 % of the feature tensor's bytes, written here and read back by fpartials_reduce: ~3 GB per training step at
            // 1M faces.  Two LDS buffers by slab parity: one barrier per slab.
            float vv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) vv[e] = group8_sum(vv[e]);
            float(*sp)[LANES][8] = s_part[((c0 - c_begin) / CS) & 1];
            if (grp == 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) sp[wave][sl][e] = vv[e];
            }
            __syncthreads();
            if (wave == 0 && grp == 0) {
                float r[8];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    r[e] = (float)((double)sp[0][sl][e] + (double)sp[1][sl][e] + (double)sp[2][sl][e] + (double)sp[3][sl][e]);
                float* pp = red.part + ((int64_t)chunk * 2) * C + off;
                *reinterpret_cast<float4*>(pp) = make_float4(r[0], r[1], r[2], r[3]);
                *reinterpret_cast<float4*>(pp + C) = make_float4(r[4], r[5], r[6], r[7]);
            }
        }
    }
    };
    if (staged) slabs(std::true_type());
    else slabs(std::false_type());
}

// Which form runs: offsets in 16-byte units fit 32 bits (row lengths are handled per chunk inside the kernel).
// DDMP_SPMM_LEAN=0 -> spmm_slab_kernel (A/B).
struct LeanPlan {
    int kind;                                                    // 0: spmm_slab_kernel, 1: spmm_lean_kernel
    int n_chunks;
};
inline LeanPlan lean_plan(const ddmp_graph* g, int64_t ldx, int64_t ldy, int C, int /*form*/ = 1) {
    static int mode = -1;
    if (mode < 0) {
        const char* e = getenv("DDMP_SPMM_LEAN");
        mode = e ? atoi(e) : 1;
    }
    (void)C;
    LeanPlan p{0, 0};
    if (mode == 0 || (ldx & 3)) return p;
    if ((uint64_t)g->n_cols * (uint64_t)(ldx >> 2) >= (1ull << 32)) return p;
    if ((ldy & 3) || (uint64_t)g->n_rows * (uint64_t)(ldy >> 2) >= (1ull << 32)) return p;
    p.kind = 1;
    p.n_chunks = (int)cdiv(g->n_rows, kRB);
    return p;
}

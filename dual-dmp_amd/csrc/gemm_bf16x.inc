// Split-precision GEMMs on the bf16 matrix cores (included by gemm.hip inside its anonymous namespace).
//
// gfx950's f32-input MFMA runs at the f32 VECTOR rate (157 TF), 1/16 of v_mfma_f32_32x32x16_bf16.  Every f32
// operand is therefore split on the fly into bf16 terms  x = x1 + x2 + x3  (round-to-nearest-even at each
// step: |x - x1 - x2 - x3| <= 2^-27 |x|, so the three terms carry the full 24-bit significand) and the
// products are accumulated in f32 by the bf16 MFMA:
//     NTERM = 3 ("bf16x6"): a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1       dropped terms <= 2^-25 |a||b|
//     NTERM = 2 ("bf16x3"): a1b1 + a1b2 + a2b1                            dropped terms <= 2^-16 |a||b|
// Each bf16 x bf16 product is exact in f32, so bf16x6 has the accuracy of an f32 FMA chain (one f32 rounding
// per accumulation step, dropped terms below half an f32 ulp) at 16/6 = 2.67x the f32-MFMA rate.
//
// Layout: block tile 128 x (64*TN), BK = 32 (two K=16 MFMA chunks); operands go global -> registers (f32,
// BatchNorm+LeakyReLU prologue) -> split -> LDS as NTERM bf16 images [row][32 + 8 pad] (80-byte rows:
// conflict-free ds_read_b128 fragments: 20*r mod 64 is distinct for the 16 rows of a lane group) -> MFMA.
// Operands whose reduction index is the slow (row) axis -- W in the NN form, both operands of the wgrad --
// are loaded as dwords, 8 consecutive reduction rows per thread, lanes along the feature axis (coalesced), so
// that the 8-deep bf16 fragment is produced in registers and written with one ds_write_b128 per term.

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

constexpr int kLdh = kBK + 8;   // LDS row stride in bf16 elements (80 bytes)

// 16-bit element type of a split: __bf16 (terms of 8 significand bits, f32 exponent range) or _Float16 (terms of 11
// bits, 5-bit exponent: the operand is scaled into range first, see gemm_f16s.inc)
template <typename E> struct V16;
template <> struct V16<__bf16> { typedef bf16x8 v8; typedef bf16x4 v4; };
template <> struct V16<_Float16> { typedef f16x8 v8; typedef f16x4 v4; };
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

template <int NTERM, typename E>
__device__ __forceinline__ void split1(float x, E (&t)[NTERM]) {
    const E h = (E)x;
    t[0] = h;
    const float r = x - (float)h;
    const E m = (E)r;
    t[1] = m;
    if (NTERM > 2) t[2] = (E)(r - (float)m);
}

template <int NTERM, typename E>
__device__ __forceinline__ void split4_store(float4 v, E* const (&dst)[NTERM]) {
    E a[NTERM], b[NTERM], c[NTERM], d[NTERM];
    split1<NTERM>(v.x, a);
    split1<NTERM>(v.y, b);
    split1<NTERM>(v.z, c);
    split1<NTERM>(v.w, d);
#pragma unroll
    for (int t = 0; t < NTERM; ++t) {
        typename V16<E>::v4 p;
        p[0] = a[t]; p[1] = b[t]; p[2] = c[t]; p[3] = d[t];
        *reinterpret_cast<typename V16<E>::v4*>(dst[t]) = p;
    }
}

template <int NTERM, typename E>
__device__ __forceinline__ void split8_store(const float (&v)[8], E* const (&dst)[NTERM]) {
    typename V16<E>::v8 p[NTERM];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        E s[NTERM];
        split1<NTERM>(v[e], s);
#pragma unroll
        for (int t = 0; t < NTERM; ++t) p[t][e] = s[t];
    }
#pragma unroll
    for (int t = 0; t < NTERM; ++t) *reinterpret_cast<typename V16<E>::v8*>(dst[t]) = p[t];
}

// _Float16, two terms (the f16x3 forms of the panel kernels): the pair helper of ddmp_common.h -- same bits, fewer operations
template <>
__device__ __forceinline__ void split4_store<2, _Float16>(float4 v, _Float16* const (&dst)[2]) {
    uint2 h, m;
    f16_split_quad(v, h, m);
    *reinterpret_cast<uint2*>(dst[0]) = h;
    *reinterpret_cast<uint2*>(dst[1]) = m;
}
template <>
__device__ __forceinline__ void split8_store<2, _Float16>(const float (&v)[8], _Float16* const (&dst)[2]) {
    uint2 h0, m0, h1, m1;
    f16_split_quad(make_float4(v[0], v[1], v[2], v[3]), h0, m0);
    f16_split_quad(make_float4(v[4], v[5], v[6], v[7]), h1, m1);
    *reinterpret_cast<uint4*>(dst[0]) = make_uint4(h0.x, h0.y, h1.x, h1.y);
    *reinterpret_cast<uint4*>(dst[1]) = make_uint4(m0.x, m0.y, m1.x, m1.y);
}

template <int NTERM>
__device__ __forceinline__ f32x16 mfma_split(const bf16x8 (&a)[NTERM], const bf16x8 (&b)[NTERM], f32x16 acc) {
    if (NTERM > 2) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], acc, 0, 0, 0);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
    return acc;
}

// ------------------------------------------------------------------------------------------------
//  Software pipeline (both kernels): stages of 16 reduction indices, two LDS stage buffers, ONE barrier per
//  stage.  Inside a stage the wave's instruction stream holds, independent of each other,
//     (a) the MFMAs on stage s           (matrix pipe),
//     (b) prologue + bf16 split + ds_write of stage s+1 from registers      (VALU + LDS),
//     (c) the global loads of stage s+2 into registers                      (VMEM),
//  and sched_group_barrier interleaves (b) into the shadows of (a): measured before pipelining, time was
//  staging + MFMA (a x6 -> x3 change removed exactly the MFMA time), i.e. nothing overlapped.
// ------------------------------------------------------------------------------------------------
constexpr int kSK = 16;          // reduction indices per stage
constexpr int kLds = kSK + 8;    // LDS row stride in bf16 (48 bytes: 12*r mod 64 distinct over a lane group)

// Left to itself the scheduler sinks every ds_read to just before its MFMA (s_waitcnt lgkmcnt(1) in front of each
// of the first 12 MFMAs of a stage: one LDS latency exposed per fragment).  The stage therefore issues all of its
// fragment reads first, fenced with sched_barrier, and the interleave pattern covers only what follows the fence.
#define DDMP_FENCE() __builtin_amdgcn_sched_barrier(0)
#define DDMP_INTERLEAVE(N_MFMA, VALU_PER, DSW_EVERY)                                   \
    _Pragma("unroll") for (int q_ = 0; q_ < (N_MFMA); ++q_) {                           \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                              \
        __builtin_amdgcn_sched_group_barrier(0x002, (VALU_PER), 0);                     \
        if ((q_ % (DSW_EVERY)) == 0) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); \
    }

// W [M,K] f32 -> NTERM bf16 planes, each [R][Cc]: (R,Cc) = (M,K) as is, or (K,M) transposed (NN form: the
// reduction index must be the contiguous one so that a lane's 8-deep fragment is one 16-byte load)
template <int NTERM>
__device__ __forceinline__ void split_w_body(const float* __restrict__ W, int64_t ldw, int M, int K, int transpose,
                                             __bf16* __restrict__ planes, int bid, int nblk) {
    const int total = M * K;
    for (int idx = bid * 256 + threadIdx.x; idx < total; idx += nblk * 256) {
        const int r = transpose ? idx / M : idx / K;          // output row
        const int c = transpose ? idx % M : idx % K;          // output column (reduction index)
        const float x = transpose ? W[(int64_t)c * ldw + r] : W[(int64_t)r * ldw + c];
        __bf16 t[NTERM];
        split1<NTERM>(x, t);
#pragma unroll
        for (int q = 0; q < NTERM; ++q) planes[(int64_t)q * total + idx] = t[q];
    }
}
template <int NTERM>
__global__ __launch_bounds__(256) void split_w_kernel(const float* __restrict__ W, int64_t ldw, int M, int K,
                                                      int transpose, __bf16* __restrict__ planes) {
    split_w_body<NTERM>(W, ldw, M, K, transpose, planes, blockIdx.x, gridDim.x);
}

constexpr int kMaxProK = 512;  // widest fused prologue (scale/shift staged in LDS)
constexpr int kPF = 3;         // stages of global loads kept in flight (register ring).  With one stage the
                               // operands of stage s+1 were requested 768 MFMA-cycles (~0.4 us) before use:
                               // measured 47 % of wave-cycles parked in s_waitcnt, MFMA pipe 38 % busy.

//  Y[n, MD] = f(A[n, KD]) . op(B)   (NT: B is [MD, KD];  KMAJOR: B is [KD, MD])
template <int TN, int NTERM, bool B_KMAJOR, bool PRO, bool KTAIL, bool BPRE>
__global__ __launch_bounds__(256) void gemm_rows_bf16_kernel(
    const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
    float* __restrict__ Y, int64_t ldy, int n_rows, int KD, int MD,
    const float* __restrict__ bias, const float* __restrict__ pscale, const float* __restrict__ pshift,
    float slope, int n_row_tiles, int n_col_tiles) {
    constexpr int BN = 64 * TN;
    constexpr int NB = B_KMAJOR ? 1 : BN / 64;
    // one carved LDS buffer: [A stages | B stages | prologue scale,shift]; the epilogue re-uses the operand
    // part as the 128 x BN output tile
    constexpr int LDC = BN + 4;                                  // output tile row stride (floats)
    constexpr size_t kABytes = sizeof(__bf16) * 2 * NTERM * kBM * kLds;
    constexpr size_t kBBytes = sizeof(__bf16) * 2 * NTERM * BN * kLds;
    constexpr size_t kTileBytes = sizeof(float) * kBM * LDC;
    constexpr size_t kOpBytes = (kABytes + kBBytes > kTileBytes ? kABytes + kBBytes : kTileBytes);
    __shared__ __attribute__((aligned(16))) unsigned char smem[kOpBytes + (PRO ? 2 * kMaxProK * 4 : 16)];
    typedef __bf16 (*StageA)[NTERM][kBM * kLds];
    typedef __bf16 (*StageB)[NTERM][BN * kLds];
    StageA As = reinterpret_cast<StageA>(smem);
    StageB Bs = reinterpret_cast<StageB>(smem + kABytes);
    float* s_pro = reinterpret_cast<float*>(smem + kOpBytes);

    const int per_xcd = (int)cdiv((int64_t)n_row_tiles, kXcd) * n_col_tiles;
    const int lin = (blockIdx.x & (kXcd - 1)) * per_xcd + (blockIdx.x >> 3);
    const int row_tile = lin / n_col_tiles, col_tile = lin % n_col_tiles;
    if (row_tile >= n_row_tiles) return;
    const int row0 = row_tile * kBM, col0 = col_tile * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int kq = tid & 3, rr = tid >> 2;                       // row-major staging: (k quad, row) 64 rows/pass
    if (PRO) {                                                   // visible after the first __syncthreads()
        for (int i = tid; i < KD; i += 256) {
            s_pro[i] = pscale[i];
            s_pro[kMaxProK + i] = pshift[i];
        }
    }
    const int bj = tid % BN, bg = (tid / BN) & 1;                // k-major staging: (feature, 8-row k group);
                                                                 // BN = 64: waves 2,3 repeat the work of waves 0,1
    // BPRE: B points to NTERM pre-split bf16 planes [MD][KD] (reduction index contiguous; see split_w_kernel):
    // thread -> (row = tid/2 of the BN-row tile, 8-element half), one 16-byte load + one ds_write_b128 per term
    const __bf16* Bp = reinterpret_cast<const __bf16*>(B);
    const int prow = (tid >> 1) % BN, phalf = tid & 1;
    const int64_t plane = (int64_t)MD * KD;
    const __bf16* prow_ptr = Bp + (int64_t)min(col0 + prow, MD - 1) * KD;
    struct Regs {
        float4 a[2];
        float4 b[BPRE ? 1 : NB];
        float bk[BPRE ? 1 : 8];
        uint4 bp[BPRE ? NTERM : 1];
    };
    Regs R[kPF];

    // Row / column indices are clamped into the matrices and never masked: clamped duplicates only reach outputs
    // that are not stored.  Only a K tail (KD % 16 != 0) needs zeroing, done with 0/1 multipliers (KTAIL).
    const float* arow[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) arow[p] = A + (int64_t)min(row0 + p * 64 + rr, n_rows - 1) * lda;
    const float* brow[NB];
#pragma unroll
    for (int p = 0; p < NB; ++p) brow[p] = B + (int64_t)min(col0 + p * 64 + rr, MD - 1) * ldb;
    const float* bcol = B + min(col0 + bj, MD - 1);

    auto load_stage = [&](int k0, Regs& r) {
#if defined(DDMP_ABLATE) && (DDMP_ABLATE & 32)
        const int kcol = min((k0 & 16) + kq * 4, KD - 4);
#else
        const int kcol = min(k0 + kq * 4, KD - 4);
#endif
#pragma unroll
        for (int p = 0; p < 2; ++p) r.a[p] = *reinterpret_cast<const float4*>(arow[p] + kcol);
        if (BPRE) {
#if defined(DDMP_ABLATE) && (DDMP_ABLATE & 16)
            const int kc = min((k0 & 16) + phalf * 8, KD - 8);
#else
            const int kc = min(k0 + phalf * 8, KD - 8);
#endif
#pragma unroll
            for (int t = 0; t < NTERM; ++t) r.bp[t] = *reinterpret_cast<const uint4*>(prow_ptr + t * plane + kc);
        } else if (!B_KMAJOR) {
#pragma unroll
            for (int p = 0; p < NB; ++p) r.b[p] = *reinterpret_cast<const float4*>(brow[p] + kcol);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) r.bk[e] = bcol[(int64_t)min(k0 + bg * 8 + e, KD - 1) * ldb];
        }
    };
    auto store_stage = [&](int buf, int k0, const Regs& r) {
        const float km = (!KTAIL || k0 + kq * 4 < KD) ? 1.f : 0.f;
        float4 sc, sh;
        if (PRO) {
            const int kcol = min(k0 + kq * 4, KD - 4);
            sc = *reinterpret_cast<const float4*>(&s_pro[kcol]);
            sh = *reinterpret_cast<const float4*>(&s_pro[kMaxProK + kcol]);
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float4 v = r.a[p];
            if (PRO) v = f4_affine_lrelu(v, sc, sh, slope);
            if (KTAIL) { v.x *= km; v.y *= km; v.z *= km; v.w *= km; }
            __bf16* dst[NTERM];
#pragma unroll
            for (int t = 0; t < NTERM; ++t) dst[t] = &As[buf][t][(p * 64 + rr) * kLds + kq * 4];
            split4_store<NTERM>(v, dst);
        }
        if (BPRE) {
            const bool pz = KTAIL && (k0 + phalf * 8 >= KD);
#pragma unroll
            for (int t = 0; t < NTERM; ++t) {
                uint4 w = r.bp[t];
                if (pz) w = make_uint4(0u, 0u, 0u, 0u);
                *reinterpret_cast<uint4*>(&Bs[buf][t][prow * kLds + phalf * 8]) = w;
            }
        } else if (!B_KMAJOR) {
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                float4 v = r.b[p];
                if (KTAIL) { v.x *= km; v.y *= km; v.z *= km; v.w *= km; }
                __bf16* dst[NTERM];
#pragma unroll
                for (int t = 0; t < NTERM; ++t) dst[t] = &Bs[buf][t][(p * 64 + rr) * kLds + kq * 4];
                split4_store<NTERM>(v, dst);
            }
        } else {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (KTAIL && k0 + bg * 8 + e >= KD) ? 0.f : r.bk[e];
            __bf16* dst[NTERM];
#pragma unroll
            for (int t = 0; t < NTERM; ++t) dst[t] = &Bs[buf][t][bj * kLds + bg * 8];
            split8_store<NTERM>(v, dst);
        }
    };

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    bf16x8 af[2][NTERM], bf[TN][NTERM];
    auto read_a = [&](int buf, int i, int t) {
        af[i][t] = *reinterpret_cast<const bf16x8*>(&As[buf][t][(wm * 64 + i * 32 + l31) * kLds + lh * 8]);
    };
    auto read_b = [&](int buf, int j, int t) {
        bf[j][t] = *reinterpret_cast<const bf16x8*>(&Bs[buf][t][(wn * 32 * TN + j * 32 + l31) * kLds + lh * 8]);
    };
    auto read_frags = [&](int buf) {                             // in the order mfma_split consumes them
#pragma unroll
        for (int t = 0; t < NTERM; ++t) {
            read_a(buf, 0, t);
            read_b(buf, 0, NTERM - 1 - t);
        }
#pragma unroll
        for (int j = 1; j < TN; ++j)
#pragma unroll
            for (int t = 0; t < NTERM; ++t) read_b(buf, j, NTERM - 1 - t);
#pragma unroll
        for (int t = 0; t < NTERM; ++t) read_a(buf, 1, t);
    };
    auto compute = [&](int buf) {
        read_frags(buf);
        DDMP_FENCE();
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = mfma_split<NTERM>(af[i], bf[j], acc[i][j]);
    };

    // Ring invariant at the top of stage s: slot (s+d) % kPF holds the raw operands of stage s+d, d = 1..kPF.
    // Stores of stages >= ns go to the idle LDS buffer and loads beyond K are clamped: the body is branch-free.
    const int ns = (KD + kSK - 1) / kSK;
#pragma unroll
    for (int d = 0; d < kPF; ++d) load_stage(d * kSK, R[d]);
    if (PRO) __syncthreads();                                    // s_pro is read by store_stage
    store_stage(0, 0, R[0]);
    load_stage(kPF * kSK, R[0]);
    __syncthreads();
    int s = 0;
    for (; s + kPF <= ns; s += kPF) {
#pragma unroll
        for (int u = 0; u < kPF; ++u) {
            const int buf = (s + u) & 1;
#ifndef DDMP_ABLATE                                              // timing-only diagnostic builds (results invalid)
            compute(buf);
            store_stage(buf ^ 1, (s + u + 1) * kSK, R[(u + 1) % kPF]);
            load_stage((s + u + 1 + kPF) * kSK, R[(u + 1) % kPF]);
            DDMP_INTERLEAVE(2 * TN * (NTERM == 3 ? 6 : 3), 5, 2)
            __syncthreads();
#else
            if (!(DDMP_ABLATE & 4)) compute(buf);
            if (!(DDMP_ABLATE & 1)) store_stage(buf ^ 1, (s + u + 1) * kSK, R[(u + 1) % kPF]);
            else asm volatile("" ::"v"(R[(u + 1) % kPF].a[0].x), "v"(R[(u + 1) % kPF].a[1].x), "v"(R[(u + 1) % kPF].bp[0].x),
                              "v"(R[(u + 1) % kPF].bp[BPRE ? 1 : 0].x), "v"(R[(u + 1) % kPF].bp[BPRE ? NTERM - 1 : 0].x));
            if (!(DDMP_ABLATE & 2)) load_stage((s + u + 1 + kPF) * kSK, R[(u + 1) % kPF]);
            DDMP_INTERLEAVE(2 * TN * (NTERM == 3 ? 6 : 3), 5, 2)
            if (!(DDMP_ABLATE & 8)) __syncthreads();
#endif
        }
    }
#pragma unroll
    for (int u = 0; u < kPF - 1; ++u) {                          // ns % kPF leftover stages
        if (s + u < ns) {
            const int buf = (s + u) & 1;
            compute(buf);
            store_stage(buf ^ 1, (s + u + 1) * kSK, R[(u + 1) % kPF]);
            __syncthreads();
        }
    }

    // Epilogue through LDS: the C/D fragment layout gives each lane 4-byte pieces of 32 different rows, i.e. 64
    // dword-store instructions per thread; measured, that store burst cost 20-24 % of the kernel (250 us per GB
    // written, not overlapped).  Staging the 128 x BN tile in the (now idle) operand buffers turns it into
    // 16 float4 stores per thread of full, coalesced row segments (+ bias).
    {
        float* ct = reinterpret_cast<float*>(smem);
        constexpr bool FITS = true;
        if constexpr (FITS) {
            __syncthreads();                                     // all waves are done reading the operand tiles
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        ct[row * LDC + wn * 32 * TN + j * 32 + l31] = acc[i][j][r];
                    }
            __syncthreads();
            constexpr int QPR = BN / 4;                          // float4 per row
            const int q = tid % QPR, r0 = tid / QPR;
            const int c = col0 + q * 4;
            float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
            // (element loads: no entry point asks for a 16-byte aligned bias, and a view into a longer vector is not)
            if (bias && c + 3 < MD) bv = make_float4(bias[c], bias[c + 1], bias[c + 2], bias[c + 3]);
            const bool vec_ok = (c + 3 < MD) && ((ldy & 3) == 0) && ((reinterpret_cast<uintptr_t>(Y) & 15) == 0);
#pragma unroll 4
            for (int row = r0; row < kBM; row += 256 / QPR) {
                const int grow = row0 + row;
                if (grow >= n_rows) break;
                float4 v = *reinterpret_cast<const float4*>(&ct[row * LDC + q * 4]);
                if (vec_ok) {
                    v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
                    *reinterpret_cast<float4*>(Y + (int64_t)grow * ldy + c) = v;
                } else {
                    const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < MD) Y[(int64_t)grow * ldy + c + e] = vv[e] + (bias ? bias[c + e] : 0.f);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int c = col0 + wn * 32 * TN + j * 32 + l31;
                if (c >= MD) continue;
                const float bv = bias ? bias[c] : 0.f;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = row0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        if (row < n_rows) Y[(int64_t)row * ldy + c] = acc[i][j][r] + bv;
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
//  wgrad: partial[s][m][k] = sum_{rows of split s} G[row][m] * f(Z[row][k])
// ------------------------------------------------------------------------------------------------
// SK: reduction rows per stage.  64 x 64 tiles (T = 1: the narrow layers) take 32: a 16-row stage there is 12 KB of input
// behind one barrier -- measured ~3 us per stage whatever the tile size, i.e. latency-, not bandwidth-bound -- and with
// four 8-row groups per stage all four waves stage distinct rows (with 16 rows waves 2,3 repeated the work of waves 0,1).
// GDUAL: the G operand is the BatchNorm+LeakyReLU backward of (G = dZ, G2 = Yb) rebuilt on the load,
//     dY = a * dZ * lrelu'(a * Yb + b) + c1 * Yb + c0   per column of M (= BwdApplyF, bn.hip; narrow aggregate-first layers)
template <int T, int NTERM, bool PRO, int SK = kSK, bool GDUAL = false>
__global__ __launch_bounds__(256) void gemm_tn_bf16_kernel(
    const float* __restrict__ G, int64_t ldg, const float* __restrict__ Z, int64_t ldz,
    float* __restrict__ out, int64_t ld_out, int64_t split_stride, int n_rows, int M, int K,
    int rows_per_split, int n_tiles_m, int n_tiles_k, int n_splits,
    const float* __restrict__ pscale, const float* __restrict__ pshift, float slope,
    const float* __restrict__ G2 = nullptr, int64_t ldg2 = 0, const float* __restrict__ ga = nullptr,
    const float* __restrict__ gb = nullptr, const float* __restrict__ gk1 = nullptr, const float* __restrict__ gk0 = nullptr) {
    constexpr int BT = 64 * T;
    constexpr int LDT = SK + 8;                  // LDS row stride in bf16 (48 | 80 bytes: conflict-free ds_read_b128)
    static_assert(256 / BT >= SK / 8, "one (column, 8-row group) item per thread");
    __shared__ __attribute__((aligned(16))) __bf16 Gs[2][NTERM][BT * LDT];
    __shared__ __attribute__((aligned(16))) __bf16 Zs[2][NTERM][BT * LDT];

    const int n_tiles = n_tiles_m * n_tiles_k;
    const int xcd = blockIdx.x & (kXcd - 1), local = blockIdx.x >> 3;
    const int tile = local % n_tiles;
    const int split = (local / n_tiles) * kXcd + xcd;
    if (split >= n_splits) return;
    const int tm0 = (tile / n_tiles_k) * BT, tk0 = (tile % n_tiles_k) * BT;
    const int r_begin = split * rows_per_split;
    const int r_end = min(n_rows, r_begin + rows_per_split);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int c = tid % BT, g = (tid / BT) % (SK / 8);      // one 8-row group of the stage
    const int gc = tm0 + c, zc = tk0 + c;
    const float* gcolp = G + min(gc, M - 1);        // columns beyond M / K only reach entries never stored
    const float* zcolp = Z + min(zc, K - 1);
    float sc = 1.f, sh = 0.f;
    if (PRO && zc < K) {
        sc = pscale[zc];
        sh = pshift[zc];
    }
    struct Regs {
        float g[8], z[8], y[GDUAL ? 8 : 1];
    };
    Regs R[kPF];
    float da = 0.f, db = 0.f, dk1 = 0.f, dk0 = 0.f;
    const float* ycolp = nullptr;
    if (GDUAL) {
        const int cc = min(gc, M - 1);
        da = ga[cc]; db = gb[cc]; dk1 = gk1[cc]; dk0 = gk0[cc];
        ycolp = G2 + cc;
    }
    // Running row pointers (one 64-bit add per element instead of min(row, r_end - 1) * ld: two v_mul_lo_u32 + v_mad_u64_u32
    // + ... per element and operand) as in the panel wgrads -- for the 64 x 64 tiles only (-3..-10 %).  The second copy of the
    // loop for rows past the matrix end costs ~40 registers, and the 128 x 128 tiles lose a wave per SIMD to it (+7 %): those
    // keep the multiply.  Rows in [r_end, n_rows) belong to the next split (valid memory, zeroed on the G side by store_stage).
    int lrow = r_begin + g * 8;                                  // wave-uniform
    const float* gp = gcolp + (int64_t)lrow * ldg;
    const float* zp = zcolp + (int64_t)lrow * ldz;
    const float* yp = GDUAL ? ycolp + (int64_t)lrow * ldg2 : nullptr;
    // `safe` (compile time, T == 1): the caller guarantees lrow + 8 <= n_rows -- unconditional straight-line loads.  With the
    // run-time test inside the main loop every load sat in an exec-masked side block: no interleaving with the MFMAs across
    // blocks and, since the compiler cannot count loads over a block that may be skipped, vmcnt(0) at the uses (round 4:
    // profiles/r04_tn_ablation.txt found this in the wide wgrad; the same pattern was here).
    auto load_stage = [&](int r0, Regs& r, auto safe) __attribute__((always_inline)) {
        if constexpr (T == 1) {
            if (decltype(safe)::value || lrow + 8 <= n_rows) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    r.g[e] = gp[(int64_t)e * ldg];
                    r.z[e] = zp[(int64_t)e * ldz];
                    if (GDUAL) r.y[GDUAL ? e : 0] = yp[(int64_t)e * ldg2];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int64_t back = (int64_t)(lrow + e) - min(lrow + e, n_rows - 1);
                    r.g[e] = gp[((int64_t)e - back) * ldg];
                    r.z[e] = zp[((int64_t)e - back) * ldz];
                    if (GDUAL) r.y[GDUAL ? e : 0] = yp[((int64_t)e - back) * ldg2];
                }
            }
            lrow += SK;
            gp += (int64_t)SK * ldg;
            zp += (int64_t)SK * ldz;
            if (GDUAL) yp += (int64_t)SK * ldg2;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int64_t row = min(r0 + g * 8 + e, r_end - 1);
                r.g[e] = gcolp[row * ldg];
                r.z[e] = zcolp[row * ldz];
                if (GDUAL) r.y[GDUAL ? e : 0] = ycolp[row * ldg2];
            }
        }
    };
    // rows beyond r_end (only in the last stage of a split) are zeroed on the G side: G = 0 kills the product
    auto store_stage = [&](int buf, int r0, const Regs& r) {
        float vg[8], vz[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float z = r.z[e];
            if (PRO) z = lrelu(fmaf(z, sc, sh), slope);
            vz[e] = z;
            float gv = r.g[e];
            if (GDUAL) {
                const float y = r.y[GDUAL ? e : 0];
                gv = fmaf(da, gv * lrelu_grad(fmaf(y, da, db), slope), fmaf(dk1, y, dk0));
            }
            vg[e] = (r0 + g * 8 + e < r_end) ? gv : 0.f;
        }
        __bf16 *dg[NTERM], *dz[NTERM];
#pragma unroll
        for (int t = 0; t < NTERM; ++t) {
            dg[t] = &Gs[buf][t][c * LDT + g * 8];
            dz[t] = &Zs[buf][t][c * LDT + g * 8];
        }
        split8_store<NTERM>(vg, dg);
        split8_store<NTERM>(vz, dz);
    };

    f32x16 acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int buf) {
#pragma unroll
        for (int kk = 0; kk < SK / 16; ++kk) {
            bf16x8 af[T][NTERM], bf[T][NTERM];
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int q = 0; q < NTERM; ++q)
                    af[i][q] = *reinterpret_cast<const bf16x8*>(&Gs[buf][q][(wm * 32 * T + i * 32 + l31) * LDT + kk * 16 + lh * 8]);
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int q = 0; q < NTERM; ++q)
                    bf[j][q] = *reinterpret_cast<const bf16x8*>(&Zs[buf][q][(wn * 32 * T + j * 32 + l31) * LDT + kk * 16 + lh * 8]);
            if (SK == 16) DDMP_FENCE();
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] = mfma_split<NTERM>(af[i], bf[j], acc[i][j]);
        }
    };

    const int ns = (r_end - r_begin + SK - 1) / SK;
    auto prologue = [&](auto safe) __attribute__((always_inline)) {
#pragma unroll
        for (int d = 0; d < kPF; ++d) load_stage(r_begin + d * SK, R[d], safe);
        store_stage(0, r_begin, R[0]);
        load_stage(r_begin + kPF * SK, R[0], safe);
    };
    auto group = [&](int s, auto safe) __attribute__((always_inline)) {      // kPF iterations; requests stages up to s + 2 kPF
#pragma unroll
        for (int u = 0; u < kPF; ++u) {
            const int buf = (s + u) & 1;
            compute(buf);
            store_stage(buf ^ 1, r_begin + (s + u + 1) * SK, R[(u + 1) % kPF]);
            load_stage(r_begin + (s + u + 1 + kPF) * SK, R[(u + 1) % kPF], safe);
            DDMP_INTERLEAVE(T * T * (NTERM == 3 ? 6 : 3) * (SK / 16), 5, 4)
            __syncthreads();
        }
    };
    int s = 0;
    // a group starting at s requests rows below r_begin + (s + 2 kPF + 1) SK: while those are rows of the matrix (every split
    // but the tail of the last) the T == 1 loads need no bounds test.  The safe loop is entered from the safe prologue only.
    const int s_lim = (n_rows - r_begin) / SK - 2 * kPF - 1;
    if (T == 1 && ns > 0 && s_lim >= 0) {
        prologue(std::true_type());
        __syncthreads();
        for (; s + kPF <= ns && s <= s_lim; s += kPF) group(s, std::true_type());
    } else {
        if (ns > 0) prologue(std::false_type());
        __syncthreads();
    }
    for (; s + kPF <= ns; s += kPF) group(s, std::false_type());
#pragma unroll
    for (int u = 0; u < kPF - 1; ++u) {
        if (s + u < ns) {
            const int buf = (s + u) & 1;
            compute(buf);
            store_stage(buf ^ 1, r_begin + (s + u + 1) * SK, R[(u + 1) % kPF]);
            __syncthreads();
        }
    }

    float* o = out + (int64_t)split * split_stride;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int k = tk0 + wn * 32 * T + j * 32 + l31;
        if (k >= K) continue;
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = tm0 + wm * 32 * T + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m < M) o[(int64_t)m * ld_out + k] = acc[i][j][r];
            }
    }
}

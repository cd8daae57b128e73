// f16 split-precision arithmetic of the panel GEMMs (included by gemm_panel.inc).
//
// A _Float16 term carries 11 significand bits (a bf16 term 8), so TWO terms  x s = h1 + h2  hold 22-23 bits of an f32
// operand and three (f16x3: h1h1 + h1h2 + h2h1, dropped h2h2 <= 2^-22 |a||b|) or four (f16x4: all four, what is left is
// the representation error <= 2^-23 of each operand) MFMAs replace the six of bf16x6 -- the scheme known as 3xTF32 on
// other hardware (TF32 has the same 11 bits).  What f16 lacks is exponent range (max 65504, subnormal step 2^-24):
// every operand is multiplied by a power of two s that puts its absolute maximum just below 2^target, which makes the
// pair (h1, h2) a fixed-point number with 24 + target bits below that maximum; the accumulators are unscaled exactly
// (powers of two) in the epilogue.  Elements more than 2^target / 2 below the maximum lose RELATIVE precision, the
// error of the contraction stays <= 2^-(24 + target) max|a| max|b| per product, far below the f32 accumulation error.
//
// Where s comes from -- a "scale slot", float[4] in device memory per operand:
//     [0] absolute maximum the scale is derived from          (read by the GEMM kernel)
//     [1] absolute maximum seen by the kernel, uint bits, atomicMax   (free: every element passes through the split)
//     [2] overflow flag: an element exceeded 65504 after scaling and was clamped
//     [3] healed events (float count; -1 = an operand was infinite: see below.  The maxima are taken with fmaxf, which
//         drops NaN -- a NaN operand is not seen here; trainer.check_scales tests the parameter and gradient arenas
//         for finiteness instead, which a NaN activation or gradient cannot miss)
// Without caller slots the library measures [0] exactly in a pre-pass over the operand (one more read of it; target
// 2^15).  A training loop passes persistent slots (DDMP_OPT_SCALES) and rolls [1] into [0] once per iteration
// (ddmp_gemm_scales_roll): the scale then lags one iteration behind the data, target 2^10 leaves a factor 64 of
// head-room, growth beyond that is clamped AND flagged.  SELF-HEALING: every GEMM launch that runs on a stale scale is
// followed by a second launch of the same kernel in `heal` mode.  That launch returns at once while the flag is clear;
// when the first launch raised it (or an earlier GEMM on the same operand did), it redoes the whole product with the
// scale derived from [1] -- the operand's exact maximum as the first launch has just recorded it -- and overwrites
// the clamped result before anything consumes it.  The roll then counts the event in [3] and clears the flag; the
// results of an iteration are never built on clamped operands (engine.check_scales reports the count and raises only
// for non-finite operands).

constexpr int kF16TargetExact = 15;
constexpr int kF16TargetStale = 10;
constexpr float kF16Max = 65504.f;

// power of two s with amax * s < 2^target  (1 for amax = 0 or non-finite)
__device__ __forceinline__ float f16s_scale(float amax, int target) {
    const int e = (int)((__float_as_uint(amax) >> 23) & 255u);   // amax in [2^(e-127), 2^(e-126))
    if (e == 0 || e == 255) return 1.f;
    int se = target - (e - 126);
    se = se < -126 ? -126 : se > 127 ? 127 : se;
    return __uint_as_float((unsigned)(se + 127) << 23);
}

__device__ __forceinline__ float f16s_scale1(float x, float s, float& amax) {
    amax = fmaxf(amax, fabsf(x));
    return __builtin_amdgcn_fmed3f(x * s, -kF16Max, kF16Max);
}

__device__ __forceinline__ float4 f16s_scale4(float4 v, float s, float& amax) {
    amax = fmaxf(fmaxf(amax, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
    float4 o;
    o.x = __builtin_amdgcn_fmed3f(v.x * s, -kF16Max, kF16Max);
    o.y = __builtin_amdgcn_fmed3f(v.y * s, -kF16Max, kF16Max);
    o.z = __builtin_amdgcn_fmed3f(v.z * s, -kF16Max, kF16Max);
    o.w = __builtin_amdgcn_fmed3f(v.w * s, -kF16Max, kF16Max);
    return o;
}

__device__ __forceinline__ float f16s_wave_max(float m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    return m;
}

// end of a GEMM kernel: what this wave saw goes into the slot (one atomic per wave)
__device__ __forceinline__ void f16s_publish(float* slot, float amax, float s) {
    amax = f16s_wave_max(amax);
    if ((threadIdx.x & 63) == 0) {
        if (!(amax <= 3.0e38f)) amax = 3.0e38f;                   // NaN / inf operands: flag them as overflow
        atomicMax(reinterpret_cast<unsigned*>(slot) + 1, __float_as_uint(amax));
        if (amax * s > kF16Max) atomicOr(reinterpret_cast<unsigned*>(slot) + 2, 1u);
    }
}

// Column normalisation of a rebuilt dY = a g + k1 y + k0 (the wide wgrad, gemm_tn_rm.hip).  The split is fixed point relative to
// the operand's global maximum, with a floor 2^-40 below it: a column whose scale a is more than kF16ColGap binades below the
// largest a of the matrix would keep fewer than 24 - (40 - gap - 24) bits, or none.  Such a column is lifted to the largest a's
// binade: a, b, k1, k0 times the power of two p = 2^(emax - e) give p dY exactly and leave the gate's sign alone, and row c of
// dW is multiplied by 1 / p afterwards.  Every other column has p = 1: results are bit for bit those without the lift.
constexpr int kF16ColGap = 12;
__device__ __forceinline__ int f16s_expo(float a) {              // biased exponent; 0: zero, subnormal or non-finite (never lifted)
    const int e = (int)((__float_as_uint(a) >> 23) & 0xffu);
    return e == 255 ? 0 : e;
}
__device__ __forceinline__ float f16s_colnorm(float a, int emax, bool inverse = false) {
    const int e = f16s_expo(a), k = min(emax - e, 100);
    if (e == 0 || k <= kF16ColGap) return 1.f;
    return __uint_as_float((unsigned)(127 + (inverse ? -k : k)) << 23);
}
// (emax, emin) of a[0..M) for the whole workgroup through two LDS ints; emin over the columns that have an exponent
__device__ __forceinline__ int2 f16s_block_expo(const float* __restrict__ a, int M, int* sh) {
    if (threadIdx.x == 0) { sh[0] = 0; sh[1] = 255; }
    __syncthreads();
    int hi = 0, lo = 255;
    for (int c = threadIdx.x; c < M; c += blockDim.x) {
        const int e = f16s_expo(a[c]);
        hi = max(hi, e);
        if (e) lo = min(lo, e);
    }
    atomicMax(&sh[0], hi);
    atomicMin(&sh[1], lo);
    __syncthreads();
    return make_int2(sh[0], sh[1]);
}

// pm 3: pm 2 with the column normalisation
__device__ __forceinline__ float f16s_operand(float x, float y, float a, float b, float k1, float k0, float slope, int pm, int emax = 0) {
    if (pm == 1) return lrelu(fmaf(x, a, b), slope);
    if (pm == 2) return fmaf(a, x * lrelu_grad(fmaf(y, a, b), slope), fmaf(k1, y, k0));
    if (pm == 3) return f16s_colnorm(a, emax) * fmaf(a, x * lrelu_grad(fmaf(y, a, b), slope), fmaf(k1, y, k0));
    return x;
}

// pre-pass: slot[0] = max |f(A)| over [n_rows, C] (slot zeroed by the caller).  PM as in gemm_panel_kernel.
template <int PM>
__global__ __launch_bounds__(256) void f16s_absmax_kernel(const float* __restrict__ A, int64_t lda,
                                                          const float* __restrict__ A2, int64_t lda2, int64_t n_rows,
                                                          int C, const float* __restrict__ pa, const float* __restrict__ pb,
                                                          const float* __restrict__ pk1, const float* __restrict__ pk0,
                                                          float slope, float* __restrict__ slot) {
    const int cq = C / 4;                                        // C % 4 == 0, rows 16-byte aligned (dispatcher)
    const int64_t total = n_rows * cq;
    float m = 0.f;
    __shared__ int sh_e[2];
    int emax = 0;
    if (PM == 3) emax = f16s_block_expo(pa, C, sh_e).x;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cq;
        const int c = (int)(i - r * cq) * 4;
        const float4 x = *reinterpret_cast<const float4*>(A + r * lda + c);
        float4 y = make_float4(0.f, 0.f, 0.f, 0.f), a = y, b = y, k1 = y, k0 = y;
        if (PM >= 2) y = *reinterpret_cast<const float4*>(A2 + r * lda2 + c);
        if (PM >= 1) {
            a = *reinterpret_cast<const float4*>(pa + c);
            b = *reinterpret_cast<const float4*>(pb + c);
        }
        if (PM >= 2) {
            k1 = *reinterpret_cast<const float4*>(pk1 + c);
            k0 = *reinterpret_cast<const float4*>(pk0 + c);
        }
        m = fmaxf(m, fabsf(f16s_operand(x.x, y.x, a.x, b.x, k1.x, k0.x, slope, PM, emax)));
        m = fmaxf(m, fabsf(f16s_operand(x.y, y.y, a.y, b.y, k1.y, k0.y, slope, PM, emax)));
        m = fmaxf(m, fabsf(f16s_operand(x.z, y.z, a.z, b.z, k1.z, k0.z, slope, PM, emax)));
        m = fmaxf(m, fabsf(f16s_operand(x.w, y.w, a.w, b.w, k1.w, k0.w, slope, PM, emax)));
    }
    m = f16s_wave_max(m);
    if ((threadIdx.x & 63) == 0) {
        if (!(m <= 3.0e38f)) m = 3.0e38f;
        atomicMax(reinterpret_cast<unsigned*>(slot), __float_as_uint(m));
    }
}

// W side: wmax[0] (zeroed by the caller) = max |W| as uint bits; the kernels that use W derive its scale from it
__global__ __launch_bounds__(256) void f16s_wmax_kernel(const float* __restrict__ W, int64_t ldw, int rows, int cols,
                                                        float* __restrict__ wmax) {
    float m = 0.f;
    for (int r = blockIdx.x; r < rows; r += gridDim.x)
        for (int c = threadIdx.x; c < cols; c += 256) m = fmaxf(m, fabsf(W[(int64_t)r * ldw + c]));
    m = f16s_wave_max(m);
    if ((threadIdx.x & 63) == 0) {
        if (!(m <= 3.0e38f)) m = 3.0e38f;
        atomicMax(reinterpret_cast<unsigned*>(wmax), __float_as_uint(m));
    }
}
__device__ __forceinline__ float f16s_wscale(const float* wmax) { return f16s_scale(*wmax, kF16TargetExact); }

// once per training iteration: the maxima collected by this iteration's kernels become the next iteration's scales
__global__ void f16s_roll_kernel(float* __restrict__ slots, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* s = slots + 4 * i;
    const float seen = s[1];
    if (reinterpret_cast<const unsigned*>(s)[2] != 0u) {         // this iteration's GEMMs on the slot were redone (healed)
        s[3] = (seen >= 3.0e38f || s[3] < 0.f) ? -1.f : s[3] + 1.f;
        s[2] = 0.f;
    }
    if (seen > 0.f) s[0] = seen;
    s[1] = 0.f;
}

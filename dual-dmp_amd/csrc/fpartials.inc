// Two-stage column reduction of float32 / float64 partials (included inside the anonymous namespace of spmm.hip and gemm.hip):
//     part[groups][2][ld] (float)  ->  sums[2C] (double) = (sum over groups of row 0, of row 1) per column
// (#include "finalize.h" first.)  Stage 1: grid (C/32, S) -- 32 columns x 8 group slices per workgroup, 8 independent loads in flight per slice, one
// float64 partial per (slice block, column).  Stage 2: one thread per output sums the S partials.  (A single stage with
// C/32 workgroups took ~250 us for 15.6k groups: more than the 2 GB pass it replaces.)  Deterministic, no atomics.
constexpr int kFpMaxS = 64;

template <typename PT>
__global__ __launch_bounds__(256) void fpartials_stage1_kernel(const PT* __restrict__ part, int groups, int ld, int C,
                                                               int S, double* __restrict__ mid /*[S][2][C]*/) {
    __shared__ double sm[2][256];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), sl = threadIdx.x >> 5;
    const int per = (groups + S - 1) / S;
    const int g0 = blockIdx.y * per, g1 = min(groups, g0 + per);
    double t0 = 0.0, t1 = 0.0;
    if (c < C) {
        int gi = g0 + sl;
        for (; gi + 56 < g1; gi += 64) {
            PT a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                a[u] = part[((int64_t)(gi + 8 * u) * 2) * ld + c];
                b[u] = part[((int64_t)(gi + 8 * u) * 2 + 1) * ld + c];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                t0 += (double)a[u];
                t1 += (double)b[u];
            }
        }
        for (; gi < g1; gi += 8) {
            t0 += (double)part[((int64_t)gi * 2) * ld + c];
            t1 += (double)part[((int64_t)gi * 2 + 1) * ld + c];
        }
    }
    sm[0][threadIdx.x] = t0;
    sm[1][threadIdx.x] = t1;
    __syncthreads();
    if (sl == 0 && c < C) {
        double r0 = 0.0, r1 = 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            r0 += sm[0][u * 32 + threadIdx.x];
            r1 += sm[1][u * 32 + threadIdx.x];
        }
        mid[((int64_t)blockIdx.y * 2) * C + c] = r0;
        mid[((int64_t)blockIdx.y * 2 + 1) * C + c] = r1;
    }
}

// one thread per column: both sums (+ the coefficients the call was asked for: finalize.h)
// shift_ref (nullable): the partials are sums of (y - ref[c]) and (y - ref[c])^2 over shift_n rows; undone here
__global__ void fpartials_stage2_kernel(const double* __restrict__ mid, int S, int C, double* __restrict__ sums,
                                        ddmp::FinalizeArgs fin, const float* __restrict__ shift_ref, double shift_n) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double t0 = 0.0, t1 = 0.0;
    int s = 0;
    for (; s + 7 < S; s += 8) {                                  // eight loads per sum in flight, the same order of additions
        double v[8], w[8];                                       // (one dependent load per step took 17 us for S = 64)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            v[u] = mid[(int64_t)(s + u) * 2 * C + c];
            w[u] = mid[(int64_t)(s + u) * 2 * C + C + c];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            t0 += v[u];
            t1 += w[u];
        }
    }
    for (; s < S; ++s) {
        t0 += mid[(int64_t)s * 2 * C + c];
        t1 += mid[(int64_t)s * 2 * C + C + c];
    }
    if (shift_ref) {
        const double r = (double)shift_ref[c];
        t1 = t1 + 2.0 * r * t0 + shift_n * r * r;
        t0 = t0 + shift_n * r;
    }
    sums[c] = t0;
    sums[C + c] = t1;
    ddmp::finalize_column(fin, c, t0, t1);
}

// Few groups (small meshes: 13k faces = 204 chunks): ONE kernel -- 32 columns x 32 group slices per 1024-thread workgroup, the
// slices meet in LDS, the thread that holds a column's two sums finalises it as the second stage would.  One launch less per
// reduction: 48 per training iteration, ~10 % of the launches of a 13k-face mesh (profiles/r05_small_mesh.txt).
constexpr int kFpSingleGroups = 512;
template <typename PT>
__global__ __launch_bounds__(1024) void fpartials_single_kernel(const PT* __restrict__ part, int groups, int ld, int C,
                                                                double* __restrict__ sums, ddmp::FinalizeArgs fin,
                                                                const float* __restrict__ shift_ref, double shift_n) {
    __shared__ double sm[2][1024];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), sl = threadIdx.x >> 5;
    double t0 = 0.0, t1 = 0.0;
    if (c < C) {
        int gi = sl;
        for (; gi + 96 < groups; gi += 128) {                    // four loads per sum in flight
            PT a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = part[((int64_t)(gi + 32 * u) * 2) * ld + c];
                b[u] = part[((int64_t)(gi + 32 * u) * 2 + 1) * ld + c];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                t0 += (double)a[u];
                t1 += (double)b[u];
            }
        }
        for (; gi < groups; gi += 32) {
            t0 += (double)part[((int64_t)gi * 2) * ld + c];
            t1 += (double)part[((int64_t)gi * 2 + 1) * ld + c];
        }
    }
    sm[0][threadIdx.x] = t0;
    sm[1][threadIdx.x] = t1;
    __syncthreads();
    if (sl == 0 && c < C) {
        double r0 = 0.0, r1 = 0.0;
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            r0 += sm[0][u * 32 + threadIdx.x];
            r1 += sm[1][u * 32 + threadIdx.x];
        }
        if (shift_ref) {
            const double r = (double)shift_ref[c];
            r1 = r1 + 2.0 * r * r0 + shift_n * r * r;
            r0 = r0 + shift_n * r;
        }
        sums[c] = r0;
        sums[C + c] = r1;
        ddmp::finalize_column(fin, c, r0, r1);
    }
}

inline size_t fpartials_mid_bytes(int C) { return (size_t)kFpMaxS * 2 * (size_t)C * sizeof(double); }

// `mid` = scratch of fpartials_mid_bytes(C); `fin`: the coefficients to write with the sums (ctx.take_fin(C))
template <typename PT>
inline void fpartials_reduce(const PT* part, int groups, int ld, int C, double* mid, double* sums, hipStream_t st,
                             const ddmp::FinalizeArgs& fin, const float* shift_ref = nullptr, double shift_n = 0.0) {
    if (groups <= kFpSingleGroups) {
        hipLaunchKernelGGL((fpartials_single_kernel<PT>), dim3((unsigned)((C + 31) / 32)), dim3(1024), 0, st, part, groups, ld, C,
                           sums, fin, shift_ref, shift_n);
        return;
    }
    const int S = (int)std::max<int64_t>(1, std::min<int64_t>(kFpMaxS, groups / 64));
    hipLaunchKernelGGL((fpartials_stage1_kernel<PT>), dim3((unsigned)((C + 31) / 32), (unsigned)S), dim3(256), 0, st, part, groups,
                       ld, C, S, mid);
    hipLaunchKernelGGL(fpartials_stage2_kernel, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, mid, S, C, sums,
                       fin, shift_ref, shift_n);
}

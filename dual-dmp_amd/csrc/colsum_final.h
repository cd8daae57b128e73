// The second stage of the two-stage column reductions (gat.hip and gatv2.hip: the attention-vector gradients; feast.hip: the offset
// gradient, also the route of gmm.hip's [dmu | dsigma]).  The first stages differ per operator and stay with it.
#pragma once
#include "row_gather.h"

namespace {

// out[c] = sum over the n_chunks partials of partial[chunk, c], c < width; column c < split goes to out0[c], any other to
// out1[c - split].  64 columns per workgroup; four lanes per column take the partials 4 apart (float64), combined in a fixed order.
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ partial, int n_chunks, int width,
                                                           float* __restrict__ out0, float* __restrict__ out1, int split) {
    __shared__ double sm[4][64];
    const int cl = threadIdx.x & 63, pt = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    double a = 0.0;
    if (c < width)
        for (int ch = pt; ch < n_chunks; ch += 4) a += (double)partial[(int64_t)ch * width + c];
    sm[pt][cl] = a;
    __syncthreads();
    if (pt == 0 && c < width) {
        const float v = (float)(((sm[0][cl] + sm[1][cl]) + sm[2][cl]) + sm[3][cl]);
        if (c < split)
            out0[c] = v;
        else
            out1[c - split] = v;
    }
}

// The second stage of a two-stage column reduction (colsum_final_kernel) on the stream.
inline int launch_colsum_final(hipStream_t st, const float* partial, int n_chunks, int width, float* out0, float* out1, int split) {
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)cdiv(width, 64)), dim3(256), 0, st, partial, n_chunks, width, out0, out1,
                       split);
    LAUNCH_TRY();
    return DDMP_OK;
}

}  // namespace

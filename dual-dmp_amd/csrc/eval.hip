// On-device evaluation block (main.py:117-123 of the reference): face normals of the predicted positions
// (util/mesh.py:87-92; the reference feeds float32 positions, so the cross product / normalisation run in
// float32 there too) and the mean angular difference to ground-truth normals (util/loss.py:261-272: inner
// product, clip, arccos, degrees, mean -- float64).  Replaces a D2H copy + numpy pass every 10 iterations.
#include "ddmp_common.h"

#include <algorithm>

namespace {
using namespace ddmp;
constexpr int kNB = 256;

// a * b - c * d with the rounding error of c * d recovered by one fma (Kahan's difference of products, <= 1.5 ulp).  A plain
// a * b - c * d is contracted into fma(a, b, -(c * d)), which keeps the rounding error of c * d alone: the cross product of two
// EQUAL edges (a face with two corners at one position) came out as that error, ~1e-8, and was then normalised to a unit
// vector instead of the reference's exact (0, 0, 0); and a sliver's normal was off by |a||b| 2^-24 / |a x b|.
__device__ __forceinline__ float diff_of_products(float a, float b, float c, float d) {
#pragma clang fp contract(off)
    const float w = c * d;
    const float e = fmaf(-c, d, w);      // w - c d, exact
    const float f = fmaf(a, b, -w);
    return f + e;
}

// An edge vector component x - y as hi + lo, exactly (TwoSum): positions of unlike magnitude or sign (z of a flat mesh
// around 0, say) do not subtract exactly, and on a sliver the 2^-24 |a| that is lost reaches the normal as 2^-24 |a||b| / |a x b|.
struct Diff {
    float hi, lo;
};
__device__ __forceinline__ Diff two_diff(float x, float y) {
#pragma clang fp contract(off)
    const float hi = x - y;
    const float t = hi - x;
    return {hi, (x - (hi - t)) + (-y - t)};
}
// One component of (a_hi + a_lo) x (b_hi + b_lo): a1 b2 - a2 b1, the first-order terms in the low parts added plainly.  Every
// product is rounded on its own and paired with its mirror image, so that equal edges give an exact 0.
__device__ __forceinline__ float cross_component(Diff a1, Diff b2, Diff a2, Diff b1) {
#pragma clang fp contract(off)
    return diff_of_products(a1.hi, b2.hi, a2.hi, b1.hi) + ((a1.lo * b2.hi - a2.hi * b1.lo) + (a1.hi * b2.lo - a2.lo * b1.hi));
}

__global__ __launch_bounds__(256) void face_normals_kernel(int F, const float* __restrict__ pos,
                                                           const int* __restrict__ faces, float* __restrict__ fn,
                                                           float* __restrict__ fa) {
    for (int f = blockIdx.x * 256 + threadIdx.x; f < F; f += gridDim.x * 256) {
        const int i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
        Diff a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p0 = pos[3 * (int64_t)i0 + c];
            a[c] = two_diff(pos[3 * (int64_t)i1 + c], p0);
            b[c] = two_diff(pos[3 * (int64_t)i2 + c], p0);
        }
        const float cx = cross_component(a[1], b[2], a[2], b[1]), cy = cross_component(a[2], b[0], a[0], b[2]),
                    cz = cross_component(a[0], b[1], a[1], b[0]);
        const float len = sqrtf(cx * cx + cy * cy + cz * cz);
        const float nrm = len + 1e-24f;
        fn[3 * (int64_t)f] = cx / nrm;
        fn[3 * (int64_t)f + 1] = cy / nrm;
        fn[3 * (int64_t)f + 2] = cz / nrm;
        if (fa) fa[f] = 0.5f * len;
    }
}

__global__ __launch_bounds__(256) void mad_kernel(int F, const float* __restrict__ n1, const double* __restrict__ n2,
                                                  double* __restrict__ partial) {
    __shared__ double sm[4];
    double s = 0.0;
    for (int f = blockIdx.x * 256 + threadIdx.x; f < F; f += kNB * 256) {
        double inner = (double)n1[3 * (int64_t)f] * n2[3 * (int64_t)f] + (double)n1[3 * (int64_t)f + 1] * n2[3 * (int64_t)f + 1] +
                       (double)n1[3 * (int64_t)f + 2] * n2[3 * (int64_t)f + 2];
        inner = inner < -1.0 ? -1.0 : (inner > 1.0 ? 1.0 : inner);
        s += acos(inner) * (180.0 / 3.14159265358979323846);
    }
    const double t = block_sum(s, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ void mad_final_kernel(const double* __restrict__ partial, int F, double* __restrict__ out) {
    __shared__ double sm[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < kNB; i += blockDim.x) s += partial[i];
    const double t = block_sum(s, sm);
    if (threadIdx.x == 0) out[0] = t / (double)F;
}
// ---- vertex update from predicted normals (util/models.py:31-44).  Per sweep: c_f = centroid of the current
// positions; p_v += (1/|F(v)|) sum_{f in F(v)} ((c_f - p_v) . n_f) n_f.  The reference updates vertices one by one
// in a Python loop, but each update reads only the centroids computed BEFORE the loop and the vertex's own
// position, so the sweep is order-independent and a parallel pass is the same computation.
// Two passes per sweep.  Per face: the three scalars d_k = (c_f - p_fk) . n_f, with c_f - p_fk formed from the face's EDGE
// vectors ((p1 - p0) + (p2 - p0)) / 3, ...: differences of neighbouring float32 positions are exact (or nearly), so d_k is good
// to 1e-7 of an edge wherever the mesh sits.  (A centroid rounded to float32 first is only good to an ulp of the COORDINATE:
// at |p| ~ 700 that put 4e-5 of an edge into every component of the update.)  Per vertex: p_v += mean_k d_k n_f over its
// corners; it reads no other vertex, so the update is in place.
// With `lo` (ddmp_vertex_update_pair_f32) a position is the float32 pair pos + lo between sweeps: stored as one float32, x and y
// in the hundreds come back rounded to 6e-5, and the next sweep's d_k carries that through n_f into the small components
// (measured at 1M faces, three sweeps: 8e-5 where 2e-6 is asked).  `pos` is always the pair's sum rounded once.
__global__ __launch_bounds__(256) void corner_offset_kernel(int F, const float* __restrict__ pos,
                                                            const float* __restrict__ lo /*nullable*/,
                                                            const float* __restrict__ nrm, const int* __restrict__ faces,
                                                            float* __restrict__ dcorner) {
    for (int f = blockIdx.x * 256 + threadIdx.x; f < F; f += gridDim.x * 256) {
        const int i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p0 = pos[3 * (int64_t)i0 + c], p1 = pos[3 * (int64_t)i1 + c], p2 = pos[3 * (int64_t)i2 + c];
            float q01 = p1 - p0, q02 = p2 - p0, q12 = p2 - p1;
            if (lo) {
                const float l0 = lo[3 * (int64_t)i0 + c], l1 = lo[3 * (int64_t)i1 + c], l2 = lo[3 * (int64_t)i2 + c];
                q01 += l1 - l0; q02 += l2 - l0; q12 += l2 - l1;
            }
            const float n = nrm[3 * (int64_t)f + c];
            d0 += n * ((q01 + q02) / 3.0f);
            d1 += n * ((q12 - q01) / 3.0f);
            d2 -= n * ((q02 + q12) / 3.0f);
        }
        dcorner[3 * (int64_t)f] = d0;
        dcorner[3 * (int64_t)f + 1] = d1;
        dcorner[3 * (int64_t)f + 2] = d2;
    }
}

// hi + lo = a + b exactly, hi = fl(a + b) (TwoSum)
__device__ __forceinline__ void two_sum(float a, float b, float& hi, float& lo) {
#pragma clang fp contract(off)
    hi = a + b;
    const float t = hi - a;
    lo = (a - (hi - t)) + (b - t);
}

__global__ __launch_bounds__(256) void vertex_update_kernel(int V, float* __restrict__ pos, float* __restrict__ lo /*nullable*/,
                                                            const float* __restrict__ dcorner, const float* __restrict__ nrm,
                                                            const int* __restrict__ vf_ptr, const int* __restrict__ vf_corner) {
    for (int v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256) {
        float dx = 0.f, dy = 0.f, dz = 0.f;
        const int b = vf_ptr[v], e = vf_ptr[v + 1];
        for (int k = b; k < e; ++k) {
            const int corner = vf_corner[k], f = corner / 3;
            const float d = dcorner[corner];
            dx += d * nrm[3 * (int64_t)f]; dy += d * nrm[3 * (int64_t)f + 1]; dz += d * nrm[3 * (int64_t)f + 2];
        }
        const float cnt = (float)(e - b);
        const float inc[3] = {dx / cnt, dy / cnt, dz / cnt};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (lo) two_sum(pos[3 * (int64_t)v + c], lo[3 * (int64_t)v + c] + inc[c], pos[3 * (int64_t)v + c], lo[3 * (int64_t)v + c]);
            else pos[3 * (int64_t)v + c] += inc[c];
        }
    }
}

int vertex_update(int64_t V, int64_t F, float* pos, const float* norm, const int32_t* faces, const int32_t* vf_ptr,
                  const int32_t* vf_corner, float* corner_scratch, float* lo, int loop, ddmp_stream stream) {
    ARG_TRY(V > 0 && V < INT32_MAX / 3 && F > 0 && F < INT32_MAX / 3 && pos && norm && faces && vf_ptr && vf_corner);
    ARG_TRY(corner_scratch && loop >= 0);
    hipStream_t st = (hipStream_t)stream;
    const int gf = (int)std::min<int64_t>(cdiv(F, 256), 2048), gv = (int)std::min<int64_t>(cdiv(V, 256), 2048);
    if (lo && loop > 0) HIP_TRY(hipMemsetAsync(lo, 0, sizeof(float) * 3 * (size_t)V, st));
    for (int it = 0; it < loop; ++it) {
        hipLaunchKernelGGL(corner_offset_kernel, dim3(gf), dim3(256), 0, st, (int)F, pos, lo, norm, faces, corner_scratch);
        LAUNCH_TRY();
        hipLaunchKernelGGL(vertex_update_kernel, dim3(gv), dim3(256), 0, st, (int)V, pos, lo, corner_scratch, norm, vf_ptr,
                           vf_corner);
        LAUNCH_TRY();
    }
    return DDMP_OK;
}
}  // namespace

extern "C" int ddmp_vertex_update_f32(int64_t V, int64_t F, float* pos, const float* norm, const int32_t* faces,
                                      const int32_t* vf_ptr, const int32_t* vf_corner, float* fc_scratch, int loop,
                                      ddmp_stream stream) {
    return vertex_update(V, F, pos, norm, faces, vf_ptr, vf_corner, fc_scratch, nullptr, loop, stream);
}
extern "C" int ddmp_vertex_update_pair_f32(int64_t V, int64_t F, float* pos, const float* norm, const int32_t* faces,
                                           const int32_t* vf_ptr, const int32_t* vf_corner, float* corner_scratch,
                                           float* lo_scratch, int loop, ddmp_stream stream) {
    ARG_TRY(lo_scratch);
    return vertex_update(V, F, pos, norm, faces, vf_ptr, vf_corner, corner_scratch, lo_scratch, loop, stream);
}

extern "C" int ddmp_face_normals_f32(int64_t F, const float* pos, const int32_t* faces, float* fn, float* fa,
                                     ddmp_stream stream) {
    ARG_TRY(F > 0 && F < INT32_MAX / 3 && pos && faces && fn);
    const int grid = (int)std::min<int64_t>(cdiv(F, 256), 2048);
    hipLaunchKernelGGL(face_normals_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (int)F, pos, faces, fn, fa);
    LAUNCH_TRY();
    return DDMP_OK;
}

extern "C" size_t ddmp_mad_workspace_bytes(void) { return sizeof(double) * kNB; }

extern "C" int ddmp_mad_f64(int64_t F, const float* n1, const double* n2, double* out, void* ws, size_t ws_bytes,
                            ddmp_stream stream) {
    ARG_TRY(F > 0 && F < INT32_MAX / 3 && n1 && n2 && out);
    if (!ws || ws_bytes < sizeof(double) * kNB) return DDMP_EWORKSPACE;
    hipLaunchKernelGGL(mad_kernel, dim3(kNB), dim3(256), 0, (hipStream_t)stream, (int)F, n1, n2, (double*)ws);
    LAUNCH_TRY();
    hipLaunchKernelGGL(mad_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)ws, (int)F, out);
    LAUNCH_TRY();
    return DDMP_OK;
}

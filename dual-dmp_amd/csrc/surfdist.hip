// Point-to-surface distance over a uniform grid (the reference's check/hausdorff_checker.py, which asks MeshLab for the
// one-sided mean distance from the vertices of one mesh to the surface of another).
//
// Grid build (ddmp_surfdist_build), all on the device:
//   pack      triangles -> [F,12] f32 (a, b, c, 3 pad: three 16-byte loads per candidate), bbox + edge-length partials
//   params    one block: bbox, cell size h = kCellEdge * mean edge, grown until the cell count fits kCellsPerFace * F
//   count     per triangle: +1 in every cell its AABB overlaps (integer atomics)
//   scan      exclusive scan of the counts (tiles of 2048 cells, block sums, one-block scan of the block sums)
//   fill      per triangle: its index at a cursor of every overlapped cell (order inside a cell varies; the minimum does not)
// Query (ddmp_surfdist_query): one lane per point, Chebyshev shells r = 0, 1, ... around the point's (clamped) cell; exact
// point-triangle distance by Voronoi region; stop once best^2 <= (distance to the outside of the visited block)^2.  That is
// exact: the closest point of a triangle lies in its AABB, so the triangle is listed in that point's cell.  Statistics: a
// separate pass over the per-sample distances in index order (deterministic per-block partials + one block, no float
// atomics), so the optional counting sort of the queries by cell changes nothing in the results.
#include "ddmp_common.h"

#include <algorithm>
#include <cmath>

// No implicit multiply-add contraction in this file: the distance of one (point, triangle) pair must round the same in
// every copy the compiler makes of the candidate loop (unrolled body, remainder, the three call sites), or the minimum
// would depend on where the triangle sits in its cell's list -- which varies from build to build.  fmaf is written out.
#pragma clang fp contract(off)

namespace {
using namespace ddmp;
constexpr int kNB = 256;             // blocks of the partial reductions (as mad_kernel)
constexpr int kThreads = 256;        // 4 waves of 64
constexpr int kTile = kThreads * 8;  // cells per scan block
constexpr float kCellEdge = 1.0f;    // cell size in mean edge lengths (before the cap)
constexpr int64_t kCellsPerFace = 4; // cell cap: kCellsPerFace * F (at least kMinCells, at most kMaxCells)
constexpr int64_t kMinCells = 64;
constexpr int64_t kMaxCells = int64_t(1) << 28;
constexpr int kStats = 12;           // n, sum, sumsq, min, max, n_dropped, bbox min xyz, bbox max xyz

struct GridHdr {
    float org[3];
    float h, inv_h, slack;  // slack: bound on the distance between a float cell assignment and the geometric cell
    int dims[3];
    int ncells;
    long long total;        // references (sum of the counts)
    int bad;                // a face index out of range
    int ready;              // kReady once the references are filled (a query on anything else returns NaN)
    int nonfinite;          // a vertex coordinate of a face is inf / NaN, or no cell size fits (nothing is built)
    int pad;
};
constexpr int kReady = 0x53444731;
static_assert(sizeof(GridHdr) <= 256, "grid header");

inline size_t al(size_t x) { return (x + 255) & ~size_t(255); }

inline int64_t cell_cap(int64_t F) { return std::min(kMaxCells, std::max(kMinCells, kCellsPerFace * F)); }

// Workspace of one grid: header | bbox partials | packed triangles | offsets [cap+1] | cursors [cap] | block sums | refs
struct Layout {
    size_t part, tri, off, cnt, bsum, refs, end;
    int64_t cap, nb, max_refs;
    Layout(int64_t F, int64_t max_refs_) : max_refs(max_refs_) {
        cap = cell_cap(F);
        nb = cdiv(cap, kTile);
        part = al(sizeof(GridHdr));
        tri = part + al(sizeof(double) * kNB * 8);
        off = tri + al(sizeof(float) * 12 * (size_t)F);
        cnt = off + al(sizeof(int) * (size_t)(cap + 1));
        bsum = cnt + al(sizeof(int) * (size_t)cap);
        refs = bsum + al(sizeof(long long) * (size_t)nb);
        end = refs + al(sizeof(int) * (size_t)std::max<int64_t>(max_refs, 0));
    }
};

// Query workspace: distances [Q] | stats partials | sort: total, offsets [cap+1], cursors [cap], block sums, permutation [Q]
struct QLayout {
    size_t dist, part, total, qoff, qcnt, bsum, perm, end;
    int64_t cap, nb;
    QLayout(int64_t Q, int64_t F) {
        cap = cell_cap(F);
        nb = cdiv(cap, kTile);
        dist = 0;
        part = al(sizeof(float) * (size_t)Q);
        total = part + al(sizeof(double) * kNB * kStats);
        qoff = total + al(sizeof(long long));
        qcnt = qoff + al(sizeof(int) * (size_t)(cap + 1));
        bsum = qcnt + al(sizeof(int) * (size_t)cap);
        perm = bsum + al(sizeof(long long) * (size_t)nb);
        end = perm + al(sizeof(int) * (size_t)Q);
    }
};

// ---------------------------------------------------------------------------------------------- block reductions
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
// all threads of the block end with the result (blockDim.x == kThreads: 4 waves)
template <typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* sm) {
    v = wave_reduce(v, op);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = sm[0];
#pragma unroll
    for (int i = 1; i < kThreads / 64; ++i) t = op(t, sm[i]);
    return t;
}
struct OpAdd { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };
struct OpMin { __device__ float operator()(float a, float b) const { return fminf(a, b); }
               __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct OpMax { __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
               __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// exclusive scan of one value per thread over the block (kThreads); *total = block sum
__device__ __forceinline__ long long block_excl_scan(long long v, long long* sm, long long* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) sm[w] = inc;
    __syncthreads();
    long long base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) {
        if (i < w) base += sm[i];
        tot += sm[i];
    }
    *total = tot;
    return base + inc - v;
}

// --------------------------------------------------------------------------------------------------- geometry
__device__ __forceinline__ int cell_of(float x, float o, float inv_h, int n) {
    float t = (x - o) * inv_h;
    if (!(t >= 0.f)) t = 0.f;                                    // (NaN too)
    t = fminf(t, (float)(n - 1));                                // (float)(n - 1) may round up: clamp the integer as well
    return min((int)t, n - 1);
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }
__device__ __forceinline__ V3 axpy(float s, V3 d, V3 e) { return {e.x - s * d.x, e.y - s * d.y, e.z - s * d.z}; }  // e - s*d
__device__ __forceinline__ float sq(V3 a) { return dot(a, a); }

// squared distance from p to segment (a, a + d); ap = p - a
__device__ __forceinline__ float seg_d2(V3 ap, V3 d) {
    const float dd = dot(d, d);
    float t = dd > 0.f ? dot(ap, d) / dd : 0.f;
    t = fminf(fmaxf(t, 0.f), 1.f);
    return sq(axpy(t, d, ap));
}

// Squared distance from p to triangle (a, b, c): closest point by Voronoi region (vertex A, B, C, edge AB, AC, BC, face).
// Every difference with p is formed against the vertex it belongs to (one rounding each).  Degenerate triangles (a repeated
// vertex, three collinear vertices: |ab x ac|^2 <= 1e-12 |ab|^2 |ac|^2) take the minimum over their three segments.
__device__ __forceinline__ float point_tri_d2(V3 p, V3 a, V3 b, V3 c) {
    const V3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
    const V3 n = {ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x};
    const float nn = sq(n), l2 = sq(ab) * sq(ac);
    const V3 bp = sub(p, b);
    if (!(nn > 1e-12f * l2)) {
        const V3 bc = sub(c, b);
        return fminf(seg_d2(ap, ab), fminf(seg_d2(ap, ac), seg_d2(bp, bc)));
    }
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.f && d2 <= 0.f) return sq(ap);                                       // A
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.f && d4 <= d3) return sq(bp);                                        // B
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {                                       // AB
        const float den = d1 - d3;
        const float v = den > 0.f ? fminf(d1 / den, 1.f) : 0.f;
        return sq(axpy(v, ab, ap));
    }
    const V3 cp = sub(p, c);
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.f && d5 <= d6) return sq(cp);                                        // C
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {                                       // AC
        const float den = d2 - d6;
        const float w = den > 0.f ? fminf(d2 / den, 1.f) : 0.f;
        return sq(axpy(w, ac, ap));
    }
    const float va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) {                                     // BC
        const float den = e43 + e56;
        const float w = den > 0.f ? fminf(e43 / den, 1.f) : 0.f;
        return sq(axpy(w, sub(c, b), bp));
    }
    const float inv = 1.f / (va + vb + vc);                                          // face: va, vb, vc > 0 here
    const float v = vb * inv, w = vc * inv;
    const V3 q = {fmaf(v, ab.x, w * ac.x), fmaf(v, ab.y, w * ac.y), fmaf(v, ab.z, w * ac.z)};
    return sq(sub(ap, q));
}

// ----------------------------------------------------------------------------------------------- grid build
__global__ __launch_bounds__(kThreads) void pack_kernel(int V, int F, const float* __restrict__ pos,
                                                        const int* __restrict__ faces, float4* __restrict__ tri,
                                                        double* __restrict__ part, GridHdr* __restrict__ hdr) {
    __shared__ double smd[kThreads / 64];
    __shared__ float smf[kThreads / 64];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    double esum = 0.0;
    for (int f = blockIdx.x * kThreads + threadIdx.x; f < F; f += kNB * kThreads) {
        int id[3];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            id[k] = faces[3 * (int64_t)f + k];
            ok = ok && id[k] >= 0 && id[k] < V;
        }
        float v[9];
        if (ok) {
#pragma unroll
            for (int k = 0; k < 9; ++k) v[k] = pos[3 * (int64_t)id[k / 3] + k % 3];
        } else {
            hdr->bad = 1;
#pragma unroll
            for (int k = 0; k < 9; ++k) v[k] = 0.f;
        }
        tri[3 * (int64_t)f] = make_float4(v[0], v[1], v[2], v[3]);
        tri[3 * (int64_t)f + 1] = make_float4(v[4], v[5], v[6], v[7]);
        tri[3 * (int64_t)f + 2] = make_float4(v[8], 0.f, 0.f, 0.f);
        if (!ok) continue;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            mn[k % 3] = fminf(mn[k % 3], v[k]);
            mx[k % 3] = fmaxf(mx[k % 3], v[k]);
        }
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) fin = fin && isfinite(v[k]);
        if (!fin) hdr->nonfinite = 1;                                // (fminf / fmaxf would skip a NaN: flag it here)
        const V3 a = {v[0], v[1], v[2]}, b = {v[3], v[4], v[5]}, c = {v[6], v[7], v[8]};
        esum += (double)sqrtf(sq(sub(b, a))) + (double)sqrtf(sq(sub(c, b))) + (double)sqrtf(sq(sub(a, c)));
    }
    double r[8];
    for (int k = 0; k < 3; ++k) r[k] = (double)block_reduce(mn[k], OpMin(), smf);
    for (int k = 0; k < 3; ++k) r[3 + k] = (double)block_reduce(mx[k], OpMax(), smf);
    r[6] = block_reduce(esum, OpAdd(), smd);
    r[7] = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < 8; ++k) part[8 * blockIdx.x + k] = r[k];
}

__global__ __launch_bounds__(kThreads) void params_kernel(int F, long long cap, const double* __restrict__ part,
                                                          GridHdr* __restrict__ hdr) {
    __shared__ double sm[kThreads / 64];
    double r[7];
    for (int k = 0; k < 3; ++k) r[k] = block_reduce(part[8 * threadIdx.x + k], OpMin(), sm);
    for (int k = 3; k < 6; ++k) r[k] = block_reduce(part[8 * threadIdx.x + k], OpMax(), sm);
    r[6] = block_reduce(part[8 * threadIdx.x + 6], OpAdd(), sm);
    if (threadIdx.x != 0) return;
    double ext[3], emax = 0.0, amax = 0.0;
    bool any = r[0] <= r[3];
    for (int k = 0; k < 3; ++k) {
        if (!any) r[k] = r[3 + k] = 0.0;                           // every face out of range: an empty 1-cell grid
        ext[k] = r[3 + k] - r[k];
        emax = fmax(emax, ext[k]);
        amax = fmax(amax, fmax(fabs(r[k]), fabs(r[3 + k])));
    }
    double h = kCellEdge * r[6] / (3.0 * F);
    if (!(h > 0.0) || !(h < 1e30)) h = emax > 0.0 ? emax / 16.0 : 1.0;
    double n[3] = {1.0, 1.0, 1.0};
    // (the host refuses the grid otherwise; an extent beyond the float32 range would overflow the differences of the query)
    bool fits = emax < 3.4028234663852886e38 && amax < 3.4028234663852886e38 && isfinite(h) && h > 0.0;
    // grow the cells until their number fits the cap: from the smallest positive h to the largest finite extent is < 900
    // steps of 1.25, so the bound below is never what ends the loop on finite input
    for (int it = 0; fits && it < 4096; ++it) {
        for (int k = 0; k < 3; ++k) n[k] = floor(ext[k] / h) + 1.0;
        if (n[0] * n[1] * n[2] <= (double)cap) break;
        h *= 1.25;
    }
    if (!fits || !(n[0] * n[1] * n[2] <= (double)cap)) {
        hdr->nonfinite = 1;
        h = 1.0;
        n[0] = n[1] = n[2] = 1.0;
        for (int k = 0; k < 3; ++k) r[k] = 0.0;
        emax = amax = 0.0;
    }
    const float hf = (float)h;
    hdr->h = hf;
    hdr->inv_h = 1.0f / hf;
    for (int k = 0; k < 3; ++k) {
        hdr->org[k] = (float)r[k];
        hdr->dims[k] = (int)n[k];
    }
    hdr->ncells = (int)(n[0] * n[1] * n[2]);
    // a point's float cell index differs from its geometric cell by a few ulps of (x - org) * inv_h (relative) and of the
    // coordinates themselves; the query's stopping bound gives that much away
    hdr->slack = (float)(16.0 * 1.1920928955078125e-07 * (emax + amax) + 1e-30);
    hdr->total = 0;
}

struct Cells { int x0, y0, z0, x1, y1, z1; };
__device__ __forceinline__ Cells tri_cells(const float4* __restrict__ tri, int f, const GridHdr& g) {
    const float4 t0 = tri[3 * (int64_t)f], t1 = tri[3 * (int64_t)f + 1], t2 = tri[3 * (int64_t)f + 2];
    const float lx = fminf(t0.x, fminf(t0.w, t1.z)), hx = fmaxf(t0.x, fmaxf(t0.w, t1.z));
    const float ly = fminf(t0.y, fminf(t1.x, t1.w)), hy = fmaxf(t0.y, fmaxf(t1.x, t1.w));
    const float lz = fminf(t0.z, fminf(t1.y, t2.x)), hz = fmaxf(t0.z, fmaxf(t1.y, t2.x));
    return {cell_of(lx, g.org[0], g.inv_h, g.dims[0]), cell_of(ly, g.org[1], g.inv_h, g.dims[1]),
            cell_of(lz, g.org[2], g.inv_h, g.dims[2]), cell_of(hx, g.org[0], g.inv_h, g.dims[0]),
            cell_of(hy, g.org[1], g.inv_h, g.dims[1]), cell_of(hz, g.org[2], g.inv_h, g.dims[2])};
}

__global__ __launch_bounds__(kThreads) void zero_kernel(int* __restrict__ p, long long n) {
    for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) p[i] = 0;
}

__global__ __launch_bounds__(kThreads) void count_kernel(int F, const float4* __restrict__ tri, const GridHdr* __restrict__ hdr,
                                                         int* __restrict__ cnt) {
    const GridHdr g = *hdr;
    for (int f = blockIdx.x * kThreads + threadIdx.x; f < F; f += gridDim.x * kThreads) {
        const Cells c = tri_cells(tri, f, g);
        for (int z = c.z0; z <= c.z1; ++z)
            for (int y = c.y0; y <= c.y1; ++y) {
                const int row = (z * g.dims[1] + y) * g.dims[0];
                for (int x = c.x0; x <= c.x1; ++x) atomicAdd(&cnt[row + x], 1);
            }
    }
}

// scan, phase 1: per tile of kTile cells, its sum
__global__ __launch_bounds__(kThreads) void scan_tiles_kernel(const int* __restrict__ cnt, const GridHdr* __restrict__ hdr,
                                                              long long* __restrict__ bsum) {
    __shared__ long long sm[kThreads / 64];
    const long long n = hdr->ncells, base = (long long)blockIdx.x * kTile + threadIdx.x * 8;
    long long s = 0;
    if (base < n)
        for (int k = 0; k < 8 && base + k < n; ++k) s += cnt[base + k];
    long long tot;
    block_excl_scan(s, sm, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// scan, phase 2 (one block): exclusive scan of the tile sums in place, the total into *total
__global__ __launch_bounds__(kThreads) void scan_blocks_kernel(long long nb, long long* __restrict__ bsum, long long* __restrict__ total) {
    __shared__ long long sm[kThreads / 64];
    long long carry = 0;
    for (long long b0 = 0; b0 < nb; b0 += kThreads) {
        const long long i = b0 + threadIdx.x;
        const long long v = i < nb ? bsum[i] : 0;
        long long tot;
        const long long e = block_excl_scan(v, sm, &tot);
        if (i < nb) bsum[i] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// scan, phase 3: offsets (int32, valid when total fits; the host checks before any reference is written) and the fill cursors
__global__ __launch_bounds__(kThreads) void scan_apply_kernel(int* __restrict__ cnt, const GridHdr* __restrict__ hdr,
                                                              const long long* __restrict__ bsum, const long long* __restrict__ total,
                                                              int* __restrict__ off) {
    __shared__ long long sm[kThreads / 64];
    const long long n = hdr->ncells, base = (long long)blockIdx.x * kTile + threadIdx.x * 8;
    int v[8];
    long long s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        v[k] = base + k < n ? cnt[base + k] : 0;
        s += v[k];
    }
    long long tot;
    long long e = bsum[blockIdx.x] + block_excl_scan(s, sm, &tot);
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (base + k < n) {
            off[base + k] = (int)e;
            cnt[base + k] = (int)e;
            e += v[k];
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) off[n] = (int)*total;   // (n may be the first index past the last tile)
}

__global__ __launch_bounds__(kThreads) void fill_kernel(int F, const float4* __restrict__ tri, const GridHdr* __restrict__ hdr,
                                                        int* __restrict__ cur, const int* __restrict__ off,
                                                        int* __restrict__ refs, long long max_refs) {
    const GridHdr g = *hdr;
    for (int f = blockIdx.x * kThreads + threadIdx.x; f < F; f += gridDim.x * kThreads) {
        const Cells c = tri_cells(tri, f, g);
        for (int z = c.z0; z <= c.z1; ++z)
            for (int y = c.y0; y <= c.y1; ++y) {
                const int row = (z * g.dims[1] + y) * g.dims[0];
                for (int x = c.x0; x <= c.x1; ++x) {
                    const int slot = atomicAdd(&cur[row + x], 1);
                    if (slot < off[row + x + 1] && slot < max_refs) refs[slot] = f;
                }
            }
    }
}

__global__ void ready_kernel(GridHdr* __restrict__ hdr) { hdr->ready = kReady; }

// --------------------------------------------------------------------------------------------------- query
__global__ __launch_bounds__(kThreads) void qcount_kernel(int Q, const float* __restrict__ pts, const GridHdr* __restrict__ hdr,
                                                          int* __restrict__ qcnt) {
    const GridHdr g = *hdr;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < Q; i += gridDim.x * kThreads) {
        const int x = cell_of(pts[3 * (int64_t)i], g.org[0], g.inv_h, g.dims[0]);
        const int y = cell_of(pts[3 * (int64_t)i + 1], g.org[1], g.inv_h, g.dims[1]);
        const int z = cell_of(pts[3 * (int64_t)i + 2], g.org[2], g.inv_h, g.dims[2]);
        atomicAdd(&qcnt[(z * g.dims[1] + y) * g.dims[0] + x], 1);
    }
}

__global__ __launch_bounds__(kThreads) void qscatter_kernel(int Q, const float* __restrict__ pts, const GridHdr* __restrict__ hdr,
                                                            int* __restrict__ cur, int* __restrict__ perm) {
    const GridHdr g = *hdr;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < Q; i += gridDim.x * kThreads) {
        const int x = cell_of(pts[3 * (int64_t)i], g.org[0], g.inv_h, g.dims[0]);
        const int y = cell_of(pts[3 * (int64_t)i + 1], g.org[1], g.inv_h, g.dims[1]);
        const int z = cell_of(pts[3 * (int64_t)i + 2], g.org[2], g.inv_h, g.dims[2]);
        const int slot = atomicAdd(&cur[(z * g.dims[1] + y) * g.dims[0] + x], 1);
        if (slot >= 0 && slot < Q) perm[slot] = i;
    }
}

__device__ __forceinline__ float scan_range(V3 p, const float4* __restrict__ tri, const int* __restrict__ refs, int b, int e,
                                            float best) {
    for (int k = b; k < e; ++k) {
        const int f = refs[k];
        const float4 t0 = tri[3 * (int64_t)f], t1 = tri[3 * (int64_t)f + 1], t2 = tri[3 * (int64_t)f + 2];
        best = fminf(best, point_tri_d2(p, {t0.x, t0.y, t0.z}, {t0.w, t1.x, t1.y}, {t1.z, t1.w, t2.x}));
    }
    return best;
}

// one lane per point (lanes of a wave search independently; perm: the counting-sorted order, or nullptr for index order)
__global__ __launch_bounds__(kThreads) void query_kernel(int Q, const float* __restrict__ pts, const int* __restrict__ perm,
                                                         const GridHdr* __restrict__ hdr, const float4* __restrict__ tri,
                                                         const int* __restrict__ off, const int* __restrict__ refs,
                                                         float max_dist, float* __restrict__ dist) {
    const GridHdr g = *hdr;
    const float md2 = max_dist > 0.f ? max_dist * max_dist : INFINITY;
    if (g.ready != kReady) {                                          // not a built grid
        for (int t = blockIdx.x * kThreads + threadIdx.x; t < Q; t += gridDim.x * kThreads) dist[t] = NAN;
        return;
    }
    for (int t = blockIdx.x * kThreads + threadIdx.x; t < Q; t += gridDim.x * kThreads) {
        const int i = perm ? perm[t] : t;
        const V3 p = {pts[3 * (int64_t)i], pts[3 * (int64_t)i + 1], pts[3 * (int64_t)i + 2]};
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) {     // no distance: NaN (and NaN statistics), never dropped
            dist[i] = NAN;
            continue;
        }
        const float pc[3] = {p.x, p.y, p.z};
        // distance from p to the grid box along each axis (0 inside): every closest point lies in the box
        float o[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float lo = g.org[k] - pc[k], hi = pc[k] - (g.org[k] + (float)g.dims[k] * g.h);
            o[k] = fmaxf(fmaxf(lo, hi) - g.slack, 0.f);
        }
        const int cx = cell_of(p.x, g.org[0], g.inv_h, g.dims[0]);
        const int cy = cell_of(p.y, g.org[1], g.inv_h, g.dims[1]);
        const int cz = cell_of(p.z, g.org[2], g.inv_h, g.dims[2]);
        float best = INFINITY;
        for (int r = 0;; ++r) {
            const int x0 = max(cx - r, 0), x1 = min(cx + r, g.dims[0] - 1);
            const int y0 = max(cy - r, 0), y1 = min(cy + r, g.dims[1] - 1);
            const int z0 = max(cz - r, 0), z1 = min(cz + r, g.dims[2] - 1);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int row = (z * g.dims[1] + y) * g.dims[0];
                    if (r == 0 || z == cz - r || z == cz + r || y == cy - r || y == cy + r) {
                        best = scan_range(p, tri, refs, off[row + x0], off[row + x1 + 1], best);   // the whole row of the shell
                    } else {
                        if (cx - r >= 0) best = scan_range(p, tri, refs, off[row + cx - r], off[row + cx - r + 1], best);
                        if (cx + r < g.dims[0]) best = scan_range(p, tri, refs, off[row + cx + r], off[row + cx + r + 1], best);
                    }
                }
            // Lower bound on the distance to every triangle not visited yet.  Its closest point q lies in the grid box and
            // outside the visited block, i.e. beyond one of the block's closed sides (a side that reaches the grid's boundary is
            // open: every cell beyond it clamps into the block).  Beyond the side on axis k: |p - q|^2 >= gap_k^2 + the squared
            // distances from p to the box along the two other axes -- which keeps points far outside the box from searching
            // the whole grid.
            float bound2 = INFINITY;
            const int cc[3] = {cx, cy, cz};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float rest = o[(k + 1) % 3] * o[(k + 1) % 3] + o[(k + 2) % 3] * o[(k + 2) % 3];
                if (cc[k] - r > 0) {
                    const float gap = fmaxf(pc[k] - (g.org[k] + (float)(cc[k] - r) * g.h) - g.slack, 0.f);
                    bound2 = fminf(bound2, gap * gap + rest);
                }
                if (cc[k] + r < g.dims[k] - 1) {
                    const float gap = fmaxf((g.org[k] + (float)(cc[k] + r + 1) * g.h) - pc[k] - g.slack, 0.f);
                    bound2 = fminf(bound2, gap * gap + rest);
                }
            }
            if (bound2 == INFINITY) break;                            // the block covers the grid
            if (fminf(best, md2) <= bound2) break;
        }
        dist[i] = best <= md2 ? sqrtf(best) : INFINITY;              // INFINITY: dropped (farther than max_dist)
    }
}

__global__ __launch_bounds__(kThreads) void stats_kernel(int Q, const float* __restrict__ dist, const float* __restrict__ pts,
                                                         double* __restrict__ part) {
    __shared__ double sm[kThreads / 64];
    double n = 0.0, s = 0.0, s2 = 0.0, mn = INFINITY, mx = -INFINITY, nd = 0.0;
    double bl[3] = {INFINITY, INFINITY, INFINITY}, bh[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < Q; i += kNB * kThreads) {
        const double d = dist[i];
        if (d == INFINITY) {
            nd += 1.0;
        } else {
            n += 1.0; s += d; s2 += d * d;
            mn = fmin(mn, d); mx = fmax(mx, d);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double x = pts[3 * (int64_t)i + k];
            bl[k] = fmin(bl[k], x); bh[k] = fmax(bh[k], x);
        }
    }
    double r[kStats] = {block_reduce(n, OpAdd(), sm), block_reduce(s, OpAdd(), sm), block_reduce(s2, OpAdd(), sm),
                        block_reduce(mn, OpMin(), sm), block_reduce(mx, OpMax(), sm), block_reduce(nd, OpAdd(), sm)};
    for (int k = 0; k < 3; ++k) {
        r[6 + k] = block_reduce(bl[k], OpMin(), sm);
        r[9 + k] = block_reduce(bh[k], OpMax(), sm);
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < kStats; ++k) part[kStats * blockIdx.x + k] = r[k];
}

__global__ __launch_bounds__(kThreads) void stats_final_kernel(const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sm[kThreads / 64];
    const double* q = part + kStats * threadIdx.x;                   // kThreads == kNB: one partial per thread
    double r[kStats] = {block_reduce(q[0], OpAdd(), sm), block_reduce(q[1], OpAdd(), sm), block_reduce(q[2], OpAdd(), sm),
                        block_reduce(q[3], OpMin(), sm), block_reduce(q[4], OpMax(), sm), block_reduce(q[5], OpAdd(), sm)};
    for (int k = 0; k < 3; ++k) {
        r[6 + k] = block_reduce(q[6 + k], OpMin(), sm);
        r[9 + k] = block_reduce(q[9 + k], OpMax(), sm);
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < kStats; ++k) out[k] = r[k];
}
static_assert(kThreads == kNB, "the final passes read one partial per thread");

inline int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, kThreads), 4096)); }
}  // namespace

extern "C" size_t ddmp_surfdist_grid_bytes(int64_t F, int64_t max_refs) {
    if (F <= 0 || F >= INT32_MAX / 3 || max_refs < 0 || max_refs >= INT32_MAX) return 0;
    return Layout(F, max_refs).end;
}

extern "C" int ddmp_surfdist_build(int64_t V, int64_t F, const float* pos, const int32_t* faces, void* grid, size_t grid_bytes,
                                   int64_t* refs_needed_host, ddmp_stream stream) {
    ARG_TRY(V > 0 && V < INT32_MAX / 3 && F > 0 && F < INT32_MAX / 3 && pos && faces && grid);
    const size_t fixed = Layout(F, 0).end;
    if (grid_bytes < fixed) return DDMP_EWORKSPACE;
    const int64_t max_refs = std::min<int64_t>((int64_t)((grid_bytes - fixed) / sizeof(int)), INT32_MAX - 1);
    const Layout L(F, max_refs);
    char* base = (char*)grid;
    GridHdr* hdr = (GridHdr*)base;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(hdr, 0, sizeof(GridHdr), st));
    hipLaunchKernelGGL(pack_kernel, dim3(kNB), dim3(kThreads), 0, st, (int)V, (int)F, pos, faces, (float4*)(base + L.tri),
                       (double*)(base + L.part), hdr);
    LAUNCH_TRY();
    hipLaunchKernelGGL(params_kernel, dim3(1), dim3(kThreads), 0, st, (int)F, (long long)L.cap, (const double*)(base + L.part), hdr);
    LAUNCH_TRY();
    hipLaunchKernelGGL(zero_kernel, dim3(grid_for(L.cap)), dim3(kThreads), 0, st, (int*)(base + L.cnt), (long long)L.cap);
    LAUNCH_TRY();
    hipLaunchKernelGGL(count_kernel, dim3(grid_for(F)), dim3(kThreads), 0, st, (int)F, (const float4*)(base + L.tri), hdr,
                       (int*)(base + L.cnt));
    LAUNCH_TRY();
    hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)L.nb), dim3(kThreads), 0, st, (const int*)(base + L.cnt), hdr,
                       (long long*)(base + L.bsum));
    LAUNCH_TRY();
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kThreads), 0, st, (long long)L.nb, (long long*)(base + L.bsum), &hdr->total);
    LAUNCH_TRY();
    // the reference count decides whether the workspace holds the grid: read it (and the index check) before any fill
    GridHdr h;
    HIP_TRY(hipMemcpyAsync(&h, hdr, sizeof(GridHdr), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (refs_needed_host) *refs_needed_host = (int64_t)h.total;
    if (h.bad) return DDMP_ERANGE;
    if (h.nonfinite) return DDMP_EINVAL;
    if (h.total > (long long)max_refs) return DDMP_EWORKSPACE;
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)L.nb), dim3(kThreads), 0, st, (int*)(base + L.cnt), hdr,
                       (const long long*)(base + L.bsum), &hdr->total, (int*)(base + L.off));
    LAUNCH_TRY();
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for(F)), dim3(kThreads), 0, st, (int)F, (const float4*)(base + L.tri), hdr,
                       (int*)(base + L.cnt), (const int*)(base + L.off), (int*)(base + L.refs), (long long)max_refs);
    LAUNCH_TRY();
    hipLaunchKernelGGL(ready_kernel, dim3(1), dim3(1), 0, st, hdr);
    LAUNCH_TRY();
    return DDMP_OK;
}

extern "C" size_t ddmp_surfdist_query_workspace_bytes(int64_t Q, int64_t F) {
    if (Q <= 0 || Q >= INT32_MAX / 3 || F <= 0 || F >= INT32_MAX / 3) return 0;
    return QLayout(Q, F).end;
}

extern "C" int ddmp_surfdist_query(int64_t F, const void* grid, size_t grid_bytes, int64_t Q, const float* points,
                                   float max_dist, int sort_queries, float* dist, double* stats, void* workspace,
                                   size_t workspace_bytes, ddmp_stream stream) {
    ARG_TRY(F > 0 && F < INT32_MAX / 3 && Q > 0 && Q < INT32_MAX / 3 && grid && points && stats);
    ARG_TRY(max_dist >= 0.f && max_dist < INFINITY && (sort_queries == 0 || sort_queries == 1));
    const Layout L(F, 0);
    if (grid_bytes < L.end) return DDMP_EINVAL;                   // not a grid of F faces
    const QLayout W(Q, F);
    if (!workspace || workspace_bytes < W.end) return DDMP_EWORKSPACE;
    const char* g = (const char*)grid;
    char* w = (char*)workspace;
    const GridHdr* hdr = (const GridHdr*)g;
    hipStream_t st = (hipStream_t)stream;
    float* d = dist ? dist : (float*)(w + W.dist);
    const int* perm = nullptr;
    if (sort_queries) {
        // counting sort of the queries by cell: the cell table of the target grid, scanned like the grid's own counts
        hipLaunchKernelGGL(zero_kernel, dim3(grid_for(W.cap)), dim3(kThreads), 0, st, (int*)(w + W.qcnt), (long long)W.cap);
        LAUNCH_TRY();
        hipLaunchKernelGGL(qcount_kernel, dim3(grid_for(Q)), dim3(kThreads), 0, st, (int)Q, points, hdr, (int*)(w + W.qcnt));
        LAUNCH_TRY();
        hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)W.nb), dim3(kThreads), 0, st, (const int*)(w + W.qcnt), hdr,
                           (long long*)(w + W.bsum));
        LAUNCH_TRY();
        long long* qtotal = (long long*)(w + W.total);
        hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kThreads), 0, st, (long long)W.nb, (long long*)(w + W.bsum), qtotal);
        LAUNCH_TRY();
        hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)W.nb), dim3(kThreads), 0, st, (int*)(w + W.qcnt), hdr,
                           (const long long*)(w + W.bsum), (const long long*)qtotal, (int*)(w + W.qoff));
        LAUNCH_TRY();
        hipLaunchKernelGGL(qscatter_kernel, dim3(grid_for(Q)), dim3(kThreads), 0, st, (int)Q, points, hdr, (int*)(w + W.qcnt),
                           (int*)(w + W.perm));
        LAUNCH_TRY();
        perm = (const int*)(w + W.perm);
    }
    hipLaunchKernelGGL(query_kernel, dim3(grid_for(Q)), dim3(kThreads), 0, st, (int)Q, points, perm, hdr,
                       (const float4*)(g + L.tri), (const int*)(g + L.off), (const int*)(g + L.refs), max_dist, d);
    LAUNCH_TRY();
    hipLaunchKernelGGL(stats_kernel, dim3(kNB), dim3(kThreads), 0, st, (int)Q, (const float*)d, points, (double*)(w + W.part));
    LAUNCH_TRY();
    hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)(w + W.part), stats);
    LAUNCH_TRY();
    return DDMP_OK;
}

// Graph handle: CSR of A + I with D^-1/2, built once (the reference recomputes gcn_norm on every
// GCNConv call, 24x per step, on a static mesh graph).  Host-side counting sort; one-off.
#include "ddmp_common.h"

#include <algorithm>
#include <new>
#include <vector>
#include <cmath>
#include <cstring>
#include <cstdlib>

extern "C" int ddmp_abi_version(void) { return DDMP_ABI_VERSION; }

extern "C" const char* ddmp_status_string(int status) {
    switch (status) {
        case DDMP_OK: return "ok";
        case DDMP_EINVAL: return "invalid argument";
        case DDMP_ERANGE: return "index out of range";
        case DDMP_ENOMEM: return "host allocation failed";
        case DDMP_EWORKSPACE: return "workspace too small";
        default: break;
    }
    if (status > 0) return hipGetErrorString((hipError_t)status);
    return "unknown status";
}

// self_loops: GCN's A + I (exactly one loop per node, dinv = (1 + in-degree)^-1/2) | ChebConv's A (none, dinv = in-degree^-1/2,
// 0 for a node without edges)
static int csr_build(int64_t n, int64_t nnz, const int64_t* ei, int32_t* rowptr, int32_t* col, float* dinv, int64_t* nnz_out,
                     bool self_loops) {
    ARG_TRY(n > 0 && nnz >= 0 && rowptr && col && dinv && nnz_out);
    ARG_TRY(nnz == 0 || ei);
    ARG_TRY(n < (int64_t)INT32_MAX && nnz + n < (int64_t)INT32_MAX);
    const int64_t* src = ei;
    const int64_t* dst = ei + nnz;
    std::vector<int32_t> cnt;
    try { cnt.assign((size_t)n + 1, 0); } catch (const std::bad_alloc&) { return DDMP_ENOMEM; }
    int64_t kept = 0;
    for (int64_t e = 0; e < nnz; ++e) {
        const int64_t s = src[e], d = dst[e];
        if (s < 0 || s >= n || d < 0 || d >= n) return DDMP_ERANGE;
        if (s == d) continue;                         // add_remaining_self_loops drops explicit loops
        cnt[(size_t)d + 1]++;
        kept++;
    }
    const int64_t used = kept + (self_loops ? n : 0);
    if (*nnz_out < used) return DDMP_EWORKSPACE;
    rowptr[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t deg = cnt[(size_t)i + 1] + (self_loops ? 1 : 0);
        rowptr[i + 1] = rowptr[i] + deg;
        dinv[i] = deg > 0 ? (float)(1.0 / std::sqrt((double)deg)) : 0.f;
    }
    // fill: cursor per row
    for (int64_t i = 0; i < n; ++i) cnt[(size_t)i] = rowptr[i];
    for (int64_t e = 0; e < nnz; ++e) {
        const int64_t s = src[e], d = dst[e];
        if (s == d) continue;
        col[cnt[(size_t)d]++] = (int32_t)s;
    }
    for (int64_t i = 0; i < n; ++i) {
        if (self_loops) col[cnt[(size_t)i]++] = (int32_t)i;
        std::sort(col + rowptr[i], col + rowptr[i + 1]);
    }
    *nnz_out = used;
    return DDMP_OK;
}

extern "C" int ddmp_csr_build_host(int64_t n, int64_t nnz, const int64_t* ei, int32_t* rowptr,
                                   int32_t* col, float* dinv, int64_t* nnz_out) {
    return csr_build(n, nnz, ei, rowptr, col, dinv, nnz_out, true);
}

extern "C" int ddmp_csr_build_sym_host(int64_t n, int64_t nnz, const int64_t* ei, int32_t* rowptr,
                                       int32_t* col, float* dinv, int64_t* nnz_out) {
    return csr_build(n, nnz, ei, rowptr, col, dinv, nnz_out, false);
}

extern "C" int ddmp_csr_bfs_order_host(int64_t n, const int32_t* rowptr, const int32_t* col,
                                       int32_t* order) {
    ARG_TRY(n > 0 && rowptr && col && order);
    std::vector<uint8_t> seen;
    try { seen.assign((size_t)n, 0); } catch (const std::bad_alloc&) { return DDMP_ENOMEM; }
    int64_t head = 0, tail = 0;
    for (int64_t seed = 0; seed < n; ++seed) {
        if (seen[(size_t)seed]) continue;
        seen[(size_t)seed] = 1;
        order[tail++] = (int32_t)seed;
        while (head < tail) {
            const int32_t u = order[head++];
            for (int32_t e = rowptr[u]; e < rowptr[u + 1]; ++e) {
                const int32_t v = col[e];
                if (v < 0 || v >= n) return DDMP_ERANGE;
                if (!seen[(size_t)v]) {
                    seen[(size_t)v] = 1;
                    order[tail++] = v;
                }
            }
        }
    }
    return DDMP_OK;
}

namespace {
struct RcbCtx {
    const double* p;
    int leaf;
};
void rcb_split(const RcbCtx& c, int32_t* idx, int64_t m) {
    while (m > c.leaf) {
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        for (int64_t i = 0; i < m; ++i)
            for (int a = 0; a < 3; ++a) {
                const double v = c.p[3 * (int64_t)idx[i] + a];
                lo[a] = std::min(lo[a], v);
                hi[a] = std::max(hi[a], v);
            }
        int ax = 0;
        for (int a = 1; a < 3; ++a)
            if (hi[a] - lo[a] > hi[ax] - lo[ax]) ax = a;
        const int64_t leaves = (m + c.leaf - 1) / c.leaf;
        const int64_t nl = (leaves / 2) * c.leaf;               // the left part: whole leaves
        const double* p = c.p;
        std::nth_element(idx, idx + nl, idx + m, [p, ax](int32_t u, int32_t v) {
            const double a = p[3 * (int64_t)u + ax], b = p[3 * (int64_t)v + ax];
            return a < b || (a == b && u < v);
        });
        rcb_split(c, idx, nl);                                  // (recursion depth <= log2(n / leaf))
        idx += nl;
        m -= nl;
    }
}
}  // namespace

extern "C" int ddmp_rcb_order_host(int64_t n, const double* xyz, int leaf, int32_t* order) {
    ARG_TRY(n > 0 && n < (int64_t)INT32_MAX && xyz && order && leaf > 0);
    for (int64_t i = 0; i < n; ++i) order[i] = (int32_t)i;
    for (int64_t i = 0; i < 3 * n; ++i)
        if (!(xyz[i] == xyz[i])) return DDMP_EINVAL;            // NaN coordinates have no order
    rcb_split(RcbCtx{xyz, leaf}, order, n);
    return DDMP_OK;
}

static int upload_graph(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* col,
                        const float* dinv, ddmp_graph** out, int64_t row0 = 0) {
    ddmp_graph* g = new (std::nothrow) ddmp_graph();
    if (!g) return DDMP_ENOMEM;
    std::memset(g, 0, sizeof(*g));
    g->n_rows = n_rows;
    g->n_cols = n_cols;
    g->nnz = rowptr[n_rows];
    int mx = 0;
    for (int64_t i = 0; i < n_rows; ++i) mx = std::max(mx, (int)(rowptr[i + 1] - rowptr[i]));
    g->max_row_nnz = mx;
    hipError_t e;
    if ((e = hipMalloc((void**)&g->rowptr, sizeof(int32_t) * (size_t)(n_rows + 1))) != hipSuccess) goto fail;
    if ((e = hipMalloc((void**)&g->col, sizeof(int32_t) * (size_t)std::max<int64_t>(g->nnz, 1))) != hipSuccess) goto fail;
    if ((e = hipMalloc((void**)&g->dinv, sizeof(float) * (size_t)n_cols)) != hipSuccess) goto fail;
    if ((e = hipMemcpy(g->rowptr, rowptr, sizeof(int32_t) * (size_t)(n_rows + 1), hipMemcpyHostToDevice)) != hipSuccess) goto fail;
    if (g->nnz > 0 &&
        (e = hipMemcpy(g->col, col, sizeof(int32_t) * (size_t)g->nnz, hipMemcpyHostToDevice)) != hipSuccess) goto fail;
    if ((e = hipMemcpy(g->dinv, dinv, sizeof(float) * (size_t)n_cols, hipMemcpyHostToDevice)) != hipSuccess) goto fail;
    g->dinv_r = g->dinv + row0;                                  // output row i is node row0 + i of the column numbering
    {   // the entries' weights dinv[col[e]] as the gather kernels stage them: no col -> dinv chain in a chunk's set-up
        std::vector<float> ew((size_t)std::max<int64_t>(g->nnz, 1), 0.f);
        for (int64_t e2 = 0; e2 < g->nnz; ++e2) ew[(size_t)e2] = dinv[col[e2]];
        if ((e = hipMalloc((void**)&g->ew, sizeof(float) * ew.size())) != hipSuccess) goto fail;
        if ((e = hipMemcpy(g->ew, ew.data(), sizeof(float) * ew.size(), hipMemcpyHostToDevice)) != hipSuccess) goto fail;
    }
    {   // patch tables (see ddmp_graph): skipped when the rows of a chunk fan out too far (unordered numbering)
        const int64_t n_chunks = (n_rows + ddmp::kChunkRows - 1) / ddmp::kChunkRows;
        // by default from 64k rows for graphs with at most 12 entries per row ON AVERAGE (mesh graphs: 4 and ~7; the LDS
        // tables of a chunk hold 16 per row); DDMP_SPMM_PATCH=1 every graph (A/B), =0 none.  Row lengths are NOT a condition
        // any more (round 5): long rows run their tail from LDS lists, oversized chunks go to the heavy list.
        const char* pe = getenv("DDMP_SPMM_PATCH");
        const int pm = pe ? atoi(pe) : 3;
        const int64_t min_rows = 65536;                          // (16384 measured no gain at 62,500 rows: profiles/r06_launch_bound_probes.txt)
        bool ok = g->nnz > 0 && (pm == 1 || (pm != 0 && g->nnz <= 12 * n_rows && n_rows >= min_rows));
        constexpr int kMaxE = ddmp::kChunkRows * 16, kMaxKd = 6;
        std::vector<int32_t> np_of, tmp;
        if (ok) {
            np_of.assign((size_t)n_chunks, 0);
            int64_t over = 0;                                    // chunks that cannot be taken even with the largest buffers
            for (int64_t c = 0; c < n_chunks; ++c) {
                const int64_t r0 = c * ddmp::kChunkRows, r1 = std::min<int64_t>(n_rows, r0 + ddmp::kChunkRows);
                const int64_t ne = rowptr[r1] - rowptr[r0];
                if (ne == 0 || ne > kMaxE) { np_of[(size_t)c] = ne == 0 ? 0 : INT32_MAX; over += ne != 0; continue; }
                tmp.assign(col + rowptr[r0], col + rowptr[r1]);
                std::sort(tmp.begin(), tmp.end());
                const int np = (int)(std::unique(tmp.begin(), tmp.end()) - tmp.begin());
                np_of[(size_t)c] = np;
                over += np > 32 * kMaxKd;
                if (c == 1023 && over > 512) { over = n_chunks; break; }     // an unordered numbering: stop counting
            }
            ok = over * 50 <= n_chunks;                          // more than 2 % oversized: not a graph for this kernel
        }
        if (ok) {
            int kd = 3;                                          // the smallest buffers that leave at most 1 % of the chunks heavy
            for (; kd < kMaxKd; ++kd) {
                int64_t heavy = 0;
                for (int64_t c = 0; c < n_chunks; ++c) heavy += np_of[(size_t)c] > 32 * kd;
                if (heavy * 100 <= n_chunks) break;
            }
            std::vector<int32_t> pl_ptr((size_t)n_chunks + 1, 0), pl_col, heavy, split((size_t)2 * n_chunks, 0);
            int n_split = 0;
            std::vector<uint16_t> lcol((size_t)std::max<int64_t>(g->nnz, 1), 0);
            int max_patch = 0;
            for (int64_t c = 0; c < n_chunks; ++c) {
                const int np = np_of[(size_t)c];
                const int64_t c0 = c * ddmp::kChunkRows, c1 = std::min<int64_t>(n_rows, c0 + ddmp::kChunkRows);
                int parts = 0;                                   // too large a patch: do its 2 halves (32 rows) or 4 quarters (16 rows) fit?
                if (np > 32 * kd && np != INT32_MAX) {
                    for (int nh = 2; nh <= 4 && !parts; nh *= 2) {
                        const int64_t rp = ddmp::kChunkRows / nh;
                        bool fit = c1 - c0 > rp * (nh - 1);      // (every part has rows)
                        for (int h = 0; h < nh && fit; ++h) {
                            const int64_t a0 = c0 + rp * h, a1 = std::min<int64_t>(c1, a0 + rp);
                            tmp.assign(col + rowptr[a0], col + rowptr[a1]);
                            std::sort(tmp.begin(), tmp.end());
                            const int64_t u = std::unique(tmp.begin(), tmp.end()) - tmp.begin();
                            fit = u > 0 && u <= 32 * kd;         // (a part without entries has no patch row to point at)
                        }
                        if (fit) parts = nh;
                    }
                }
                if (parts) {
                    const int64_t rp = ddmp::kChunkRows / parts;
                    g->max_chunk_nnz = std::max(g->max_chunk_nnz, (int)(rowptr[c1] - rowptr[c0]));
                    split[(size_t)2 * c] = (int32_t)split.size();            // this chunk's (patch start, record slot) pairs, parts 1 ..
                    split[(size_t)2 * c + 1] = parts;
                    for (int h = 0; h < parts; ++h) {
                        const int64_t a0 = c0 + rp * h, a1 = std::min<int64_t>(c1, a0 + rp);
                        tmp.assign(col + rowptr[a0], col + rowptr[a1]);
                        std::sort(tmp.begin(), tmp.end());
                        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
                        max_patch = std::max(max_patch, (int)tmp.size());
                        for (int64_t e2 = rowptr[a0]; e2 < rowptr[a1]; ++e2)
                            lcol[(size_t)e2] = (uint16_t)(std::lower_bound(tmp.begin(), tmp.end(), col[e2]) - tmp.begin());
                        if (h > 0) {
                            split.push_back((int32_t)pl_col.size());
                            split.push_back((int32_t)(n_chunks + n_split++));
                        }
                        pl_col.insert(pl_col.end(), tmp.begin(), tmp.end());
                    }
                } else if (np == 0 || np > 32 * kd) {
                    heavy.push_back((int32_t)c);
                } else {
                    const int64_t r0 = c * ddmp::kChunkRows, r1 = std::min<int64_t>(n_rows, r0 + ddmp::kChunkRows);
                    tmp.assign(col + rowptr[r0], col + rowptr[r1]);
                    std::sort(tmp.begin(), tmp.end());
                    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
                    max_patch = std::max(max_patch, (int)tmp.size());
                    g->max_chunk_nnz = std::max(g->max_chunk_nnz, (int)(rowptr[r1] - rowptr[r0]));
                    for (int64_t e2 = rowptr[r0]; e2 < rowptr[r1]; ++e2)
                        lcol[(size_t)e2] = (uint16_t)(std::lower_bound(tmp.begin(), tmp.end(), col[e2]) - tmp.begin());
                    pl_col.insert(pl_col.end(), tmp.begin(), tmp.end());
                }
                pl_ptr[(size_t)c + 1] = (int32_t)pl_col.size();
            }
            if (max_patch > 0) {
                if ((e = hipMalloc((void**)&g->pl_ptr, sizeof(int32_t) * pl_ptr.size())) != hipSuccess) goto fail;
                if ((e = hipMalloc((void**)&g->pl_col, sizeof(int32_t) * std::max<size_t>(pl_col.size(), 1))) != hipSuccess) goto fail;
                if ((e = hipMalloc((void**)&g->lcol, sizeof(uint16_t) * lcol.size())) != hipSuccess) goto fail;
                if ((e = hipMemcpy(g->pl_ptr, pl_ptr.data(), sizeof(int32_t) * pl_ptr.size(), hipMemcpyHostToDevice)) != hipSuccess) goto fail;
                if ((e = hipMemcpy(g->pl_col, pl_col.data(), sizeof(int32_t) * pl_col.size(), hipMemcpyHostToDevice)) != hipSuccess) goto fail;
                if ((e = hipMemcpy(g->lcol, lcol.data(), sizeof(uint16_t) * lcol.size(), hipMemcpyHostToDevice)) != hipSuccess) goto fail;
                if (n_split > 0) {
                    if ((e = hipMalloc((void**)&g->pl_split, sizeof(int32_t) * split.size())) != hipSuccess) goto fail;
                    if ((e = hipMemcpy(g->pl_split, split.data(), sizeof(int32_t) * split.size(), hipMemcpyHostToDevice)) != hipSuccess) goto fail;
                    g->n_split = n_split;
                }
                if (!heavy.empty()) {
                    if ((e = hipMalloc((void**)&g->heavy, sizeof(int32_t) * heavy.size())) != hipSuccess) goto fail;
                    if ((e = hipMemcpy(g->heavy, heavy.data(), sizeof(int32_t) * heavy.size(), hipMemcpyHostToDevice)) != hipSuccess) goto fail;
                }
                g->n_heavy = (int)heavy.size();
                g->max_patch = max_patch;
                g->patch_kd = kd;
            }
        }
    }
    *out = g;
    return DDMP_OK;
fail:
    ddmp_graph_destroy(g);
    return (int)e;
}

extern "C" int ddmp_graph_create_csr_host(int64_t n_rows, int64_t n_cols, const int32_t* rowptr,
                                          const int32_t* col, const float* dinv, ddmp_graph** out) {
    ARG_TRY(out && n_rows > 0 && n_cols >= n_rows && rowptr && col && dinv);
    ARG_TRY(rowptr[0] == 0);
    for (int64_t i = 0; i < n_rows; ++i) ARG_TRY(rowptr[i + 1] >= rowptr[i]);
    for (int64_t e = 0; e < rowptr[n_rows]; ++e)
        if (col[e] < 0 || col[e] >= n_cols) return DDMP_ERANGE;
    return upload_graph(n_rows, n_cols, rowptr, col, dinv, out);
}

// Rows [row0, row1) of a local CSR as a graph of their own (round 6: the interior / boundary halves of a partitioned graph,
// so that the halo exchange of a layer travels while the interior rows are aggregated -- dual-dmp_amd/dist.py): output row i
// is node row0 + i, the columns keep the numbering of the whole local graph (X is the same tensor, Y starts at row row0).
extern "C" int ddmp_graph_create_csr_rows_host(int64_t n_rows_all, int64_t n_cols, const int32_t* rowptr, const int32_t* col,
                                               const float* dinv, int64_t row0, int64_t row1, ddmp_graph** out) {
    ARG_TRY(out && n_rows_all > 0 && n_cols >= n_rows_all && rowptr && col && dinv && row0 >= 0 && row1 > row0 && row1 <= n_rows_all);
    ARG_TRY(rowptr[0] == 0);
    for (int64_t i = 0; i < n_rows_all; ++i) ARG_TRY(rowptr[i + 1] >= rowptr[i]);
    for (int64_t e = rowptr[row0]; e < rowptr[row1]; ++e)
        if (col[e] < 0 || col[e] >= n_cols) return DDMP_ERANGE;
    std::vector<int32_t> rp;
    try {
        rp.resize((size_t)(row1 - row0) + 1);
    } catch (const std::bad_alloc&) {
        return DDMP_ENOMEM;
    }
    for (int64_t i = row0; i <= row1; ++i) rp[(size_t)(i - row0)] = rowptr[i] - rowptr[row0];
    return upload_graph(row1 - row0, n_cols, rp.data(), col + rowptr[row0], dinv, out, row0);
}

static int graph_create(int64_t n, int64_t nnz, const int64_t* edge_index, int on_device, ddmp_graph** out, bool self_loops) {
    ARG_TRY(out && n > 0 && nnz >= 0 && (nnz == 0 || edge_index));
    std::vector<int64_t> host_ei;
    std::vector<int32_t> rowptr, col;
    std::vector<float> dinv;
    try {
        rowptr.resize((size_t)n + 1);
        col.resize((size_t)std::max<int64_t>(nnz + (self_loops ? n : 0), 1));
        dinv.resize((size_t)n);
        if (on_device && nnz > 0) host_ei.resize((size_t)(2 * nnz));
    } catch (const std::bad_alloc&) {
        return DDMP_ENOMEM;
    }
    const int64_t* ei = edge_index;
    if (on_device && nnz > 0) {
        HIP_TRY(hipMemcpy(host_ei.data(), edge_index, sizeof(int64_t) * (size_t)(2 * nnz), hipMemcpyDeviceToHost));
        ei = host_ei.data();
    }
    int64_t used = nnz + (self_loops ? n : 0);
    int st = csr_build(n, nnz, ei, rowptr.data(), col.data(), dinv.data(), &used, self_loops);
    if (st != DDMP_OK) return st;
    return upload_graph(n, n, rowptr.data(), col.data(), dinv.data(), out);
}

extern "C" int ddmp_graph_create(int64_t n, int64_t nnz, const int64_t* edge_index, int on_device,
                                 ddmp_graph** out) {
    return graph_create(n, nnz, edge_index, on_device, out, true);
}

// S = D^-1/2 A D^-1/2 without self loops (ChebConv, normalization = "sym"); rows without entries are legal in every gather
extern "C" int ddmp_graph_create_sym(int64_t n, int64_t nnz, const int64_t* edge_index, int on_device,
                                     ddmp_graph** out) {
    return graph_create(n, nnz, edge_index, on_device, out, false);
}

// ---------------------------------------------------------------------------------------- valued graphs
// Structure: coalesced CSR by target + the three maps.  Rows are sorted by (source, input position) so that an entry's input
// edges are listed in input order: the device sums them in that order, deterministically.
static int csr_build_valued(int64_t n, int64_t nnz, const int64_t* ei, int flags, int32_t* rowptr, int32_t* col, int32_t* ee_ptr,
                            int32_t* ee_idx, int32_t* eid, int32_t* mirror, int64_t* n_entries) {
    ARG_TRY(n > 0 && nnz >= 0 && rowptr && col && ee_ptr && ee_idx && eid && mirror && n_entries);
    ARG_TRY(nnz == 0 || ei);
    ARG_TRY(n < (int64_t)INT32_MAX && nnz + n < (int64_t)INT32_MAX);
    ARG_TRY(!(flags & ~(DDMP_GV_LOOPS | DDMP_GV_IMPROVED | DDMP_GV_NORMALIZE | DDMP_GV_DROP_LOOPS | DDMP_GV_REQUIRE_SYM)));
    ARG_TRY(!((flags & DDMP_GV_LOOPS) && (flags & DDMP_GV_DROP_LOOPS)));
    const bool loops = flags & DDMP_GV_LOOPS, drop = flags & DDMP_GV_DROP_LOOPS;
    const int64_t* src = ei;
    const int64_t* dst = ei + nnz;
    const int64_t cap = *n_entries;
    std::vector<int32_t> cnt, last_loop;
    std::vector<std::pair<int32_t, int32_t>> ent;                // per row: (source, input edge | -1 = the added loop)
    try {
        cnt.assign((size_t)n + 1, 0);
        if (loops) last_loop.assign((size_t)n, -1);
    } catch (const std::bad_alloc&) { return DDMP_ENOMEM; }
    for (int64_t k = 0; k < nnz; ++k) {
        const int64_t s = src[k], d = dst[k];
        if (s < 0 || s >= n || d < 0 || d >= n) return DDMP_ERANGE;
        eid[k] = -1;
        if (s == d && (loops || drop)) {
            if (loops) last_loop[(size_t)d] = (int32_t)k;        // add_remaining_self_loops: the last explicit loop's weight stays
            continue;
        }
        cnt[(size_t)d + 1]++;
    }
    if (loops) for (int64_t i = 0; i < n; ++i) cnt[(size_t)i + 1]++;
    for (int64_t i = 0; i < n; ++i) cnt[(size_t)i + 1] += cnt[(size_t)i];
    try { ent.resize((size_t)cnt[(size_t)n]); } catch (const std::bad_alloc&) { return DDMP_ENOMEM; }
    {
        std::vector<int32_t> cur(cnt.begin(), cnt.end() - 1);
        for (int64_t k = 0; k < nnz; ++k) {
            const int64_t s = src[k], d = dst[k];
            if (s == d && (loops || drop)) continue;
            ent[(size_t)cur[(size_t)d]++] = {(int32_t)s, (int32_t)k};
        }
        if (loops) for (int64_t i = 0; i < n; ++i) ent[(size_t)cur[(size_t)i]++] = {(int32_t)i, last_loop[(size_t)i]};
    }
    int64_t ne = 0, nee = 0;
    rowptr[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        auto b = ent.begin() + cnt[(size_t)i], e = ent.begin() + cnt[(size_t)i + 1];
        std::stable_sort(b, e, [](const std::pair<int32_t, int32_t>& x, const std::pair<int32_t, int32_t>& y) { return x.first < y.first; });
        for (auto it = b; it != e; ++it) {
            if (it == b || it->first != (it - 1)->first) {
                if (ne >= cap) return DDMP_EWORKSPACE;
                col[ne] = it->first;
                ee_ptr[ne] = (int32_t)nee;
                ++ne;
            }
            if (it->second >= 0) {
                ee_idx[nee++] = it->second;
                eid[it->second] = (int32_t)(ne - 1);
            }
        }
        rowptr[i + 1] = (int32_t)ne;
    }
    if (ne >= cap + 1) return DDMP_EWORKSPACE;
    ee_ptr[ne] = (int32_t)nee;
    for (int64_t i = 0; i < n; ++i)
        for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            const int32_t j = col[e];
            const int32_t* b = col + rowptr[j];
            const int32_t* t = col + rowptr[j + 1];
            const int32_t* p = std::lower_bound(b, t, (int32_t)i);
            if (p == t || *p != (int32_t)i) return DDMP_EINVAL;   // the edge structure is not symmetric
            mirror[e] = (int32_t)(p - col);
        }
    *n_entries = ne;
    return DDMP_OK;
}

extern "C" int ddmp_csr_build_valued_host(int64_t n, int64_t nnz, const int64_t* ei, int flags, int32_t* rowptr, int32_t* col,
                                          int32_t* ee_ptr, int32_t* ee_idx, int32_t* eid, int32_t* mirror, int64_t* n_entries) {
    return csr_build_valued(n, nnz, ei, flags, rowptr, col, ee_ptr, ee_idx, eid, mirror, n_entries);
}

namespace {
// one thread per row: the entries' coalesced weights (input order), the row's weighted degree (CSR order), s = deg^-1/2
__global__ __launch_bounds__(256) void gv_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ ee_ptr,
                                                      const int* __restrict__ ee_idx, const float* __restrict__ w, float* __restrict__ a,
                                                      float* __restrict__ s, int n, float fill, int normalize, int* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float deg = 0.f;
    int bad = 0;
    for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int t0 = ee_ptr[e], t1 = ee_ptr[e + 1];
        float v = t0 == t1 ? fill : 0.f;
        for (int t = t0; t < t1; ++t) v += w ? w[ee_idx[t]] : 1.f;
        a[e] = v;
        if (!(fabsf(v) <= 3.4028234664e38f)) bad |= DDMP_GV_ENONFINITE;
        deg += v;
    }
    if (!(fabsf(deg) <= 3.4028234664e38f)) bad |= DDMP_GV_ENONFINITE;
    if (normalize && deg < 0.f) bad |= DDMP_GV_ENEGDEG;
    s[i] = normalize ? (deg > 0.f ? (float)(1.0 / sqrt((double)deg)) : 0.f) : 1.f;
    if (bad) atomicOr(status, bad);
}
// one thread per entry: the gather's factors for A and A^T
__global__ __launch_bounds__(256) void gv_entries_kernel(const int* __restrict__ col, const int* __restrict__ mirror,
                                                         const float* __restrict__ a, const float* __restrict__ s, float* __restrict__ ew,
                                                         float* __restrict__ ew_t, int ne, int normalize, int require_sym,
                                                         int* __restrict__ status) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const float ae = a[e], am = a[mirror[e]];
    const float sj = normalize ? s[col[e]] : 1.f;
    ew[e] = normalize ? ae * sj : ae;
    if (ew_t != ew) ew_t[e] = normalize ? am * sj : am;
    if (require_sym && ae != am) atomicOr(status, DDMP_GV_ENOTSYM);
}
// one thread per row: r_i + c_i, then the entries' gradient
__global__ __launch_bounds__(256) void gv_grad_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const int* __restrict__ mirror, const float* __restrict__ ew,
                                                           const float* __restrict__ ew_t, const float* __restrict__ s,
                                                           const float* __restrict__ G, float* __restrict__ ge, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    float rc = 0.f;
    for (int e = e0; e < e1; ++e) rc += ew[e] * G[e] + ew_t[e] * G[mirror[e]];
    const float si = s[i];
    const float k = 0.5f * si * si * si * rc;
    for (int e = e0; e < e1; ++e) ge[e] = si * s[col[e]] * G[e] - k;
}
__global__ __launch_bounds__(256) void gv_grad_edges_kernel(const int* __restrict__ eid, const float* __restrict__ ge,
                                                            float* __restrict__ dw, int64_t nnz) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nnz) return;
    const int e = eid[k];
    dw[k] = e >= 0 ? ge[e] : 0.f;
}
}  // namespace

extern "C" int ddmp_graph_set_values(ddmp_graph* g, const float* w, ddmp_stream stream) {
    ARG_TRY(g && g->valued);
    hipStream_t st = (hipStream_t)stream;
    const int normalize = (g->valued & DDMP_GV_NORMALIZE) ? 1 : 0;
    const float fill = (g->valued & DDMP_GV_IMPROVED) ? 2.f : 1.f;
    HIP_TRY(hipMemsetAsync(g->vstatus, 0, sizeof(int), st));
    const int n = (int)g->n_rows, ne = (int)g->nnz;
    hipLaunchKernelGGL(gv_rows_kernel, dim3((unsigned)ddmp::cdiv(n, 256)), dim3(256), 0, st, g->rowptr, g->ee_ptr, g->ee_idx, w, g->a,
                       g->dinv, n, fill, normalize, g->vstatus);
    LAUNCH_TRY();
    if (ne > 0) {
        hipLaunchKernelGGL(gv_entries_kernel, dim3((unsigned)ddmp::cdiv(ne, 256)), dim3(256), 0, st, g->col, g->mirror, g->a, g->dinv,
                           g->ew, g->ew_t, ne, normalize, (g->valued & DDMP_GV_REQUIRE_SYM) ? 1 : 0, g->vstatus);
        LAUNCH_TRY();
    }
    return DDMP_OK;
}

extern "C" int ddmp_graph_values_status(const ddmp_graph* g, int* status_host, ddmp_stream stream) {
    ARG_TRY(g && g->valued && status_host);
    HIP_TRY(hipMemcpyAsync(status_host, g->vstatus, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return DDMP_OK;
}

extern "C" int ddmp_graph_export_values(const ddmp_graph* g, float* ew, float* ew_t, float* a, float* s, ddmp_stream stream) {
    ARG_TRY(g && g->valued);
    hipStream_t st = (hipStream_t)stream;
    const size_t eb = sizeof(float) * (size_t)g->nnz;
    if (ew && eb) HIP_TRY(hipMemcpyAsync(ew, g->ew, eb, hipMemcpyDeviceToDevice, st));
    if (ew_t && eb) HIP_TRY(hipMemcpyAsync(ew_t, g->ew_t, eb, hipMemcpyDeviceToDevice, st));
    if (a && eb) HIP_TRY(hipMemcpyAsync(a, g->a, eb, hipMemcpyDeviceToDevice, st));
    if (s) HIP_TRY(hipMemcpyAsync(s, g->dinv, sizeof(float) * (size_t)g->n_rows, hipMemcpyDeviceToDevice, st));
    return DDMP_OK;
}

extern "C" int ddmp_graph_weight_grad(const ddmp_graph* g, const float* G, float* dw, ddmp_stream stream) {
    ARG_TRY(g && g->valued && G && dw);
    hipStream_t st = (hipStream_t)stream;
    const float* ge = G;                                         // not normalising: g_e = G_e
    if (g->valued & DDMP_GV_NORMALIZE) {
        hipLaunchKernelGGL(gv_grad_rows_kernel, dim3((unsigned)ddmp::cdiv(g->n_rows, 256)), dim3(256), 0, st, g->rowptr, g->col, g->mirror,
                           g->ew, g->ew_t, g->dinv, G, g->ge, (int)g->n_rows);
        LAUNCH_TRY();
        ge = g->ge;
    }
    if (g->nnz_in > 0) {
        hipLaunchKernelGGL(gv_grad_edges_kernel, dim3((unsigned)ddmp::cdiv(g->nnz_in, 256)), dim3(256), 0, st, g->eid, ge, dw, g->nnz_in);
        LAUNCH_TRY();
    }
    return DDMP_OK;
}

extern "C" int ddmp_graph_create_valued(int64_t n, int64_t nnz, const int64_t* edge_index, int on_device, int flags, ddmp_graph** out) {
    ARG_TRY(out && n > 0 && nnz >= 0 && (nnz == 0 || edge_index));
    std::vector<int64_t> host_ei;
    std::vector<int32_t> rowptr, col, ee_ptr, ee_idx, eid, mirror;
    std::vector<float> dinv;
    const size_t cap = (size_t)(nnz + n);
    try {
        rowptr.resize((size_t)n + 1);
        col.resize(cap);
        ee_ptr.resize(cap + 1);
        mirror.resize(cap);
        ee_idx.resize((size_t)std::max<int64_t>(nnz, 1));
        eid.resize((size_t)std::max<int64_t>(nnz, 1));
        dinv.assign((size_t)n, 0.f);
        if (on_device && nnz > 0) host_ei.resize((size_t)(2 * nnz));
    } catch (const std::bad_alloc&) {
        return DDMP_ENOMEM;
    }
    const int64_t* ei = edge_index;
    if (on_device && nnz > 0) {
        HIP_TRY(hipMemcpy(host_ei.data(), edge_index, sizeof(int64_t) * (size_t)(2 * nnz), hipMemcpyDeviceToHost));
        ei = host_ei.data();
    }
    int64_t ne = (int64_t)cap;
    int st = csr_build_valued(n, nnz, ei, flags, rowptr.data(), col.data(), ee_ptr.data(), ee_idx.data(), eid.data(), mirror.data(), &ne);
    if (st != DDMP_OK) return st;
    ddmp_graph* g = nullptr;
    st = upload_graph(n, n, rowptr.data(), col.data(), dinv.data(), &g);
    if (st != DDMP_OK) return st;
    g->valued = DDMP_GV_VALUED | flags;
    g->nnz_in = nnz;
    hipError_t e;
    const size_t ne1 = (size_t)std::max<int64_t>(ne, 1), nz1 = (size_t)std::max<int64_t>(nnz, 1);
    auto up = [&](int32_t** dst, const int32_t* src_h, size_t cnt) {
        if ((e = hipMalloc((void**)dst, sizeof(int32_t) * cnt)) != hipSuccess) return false;
        return (e = hipMemcpy(*dst, src_h, sizeof(int32_t) * cnt, hipMemcpyHostToDevice)) == hipSuccess;
    };
    if (!up(&g->ee_ptr, ee_ptr.data(), (size_t)ne + 1) || !up(&g->ee_idx, ee_idx.data(), nz1) || !up(&g->eid, eid.data(), nz1) ||
        !up(&g->mirror, mirror.data(), ne1))
        goto fail;
    if ((e = hipMalloc((void**)&g->a, sizeof(float) * ne1)) != hipSuccess) goto fail;
    if ((e = hipMalloc((void**)&g->ge, sizeof(float) * ne1)) != hipSuccess) goto fail;
    if ((e = hipMalloc((void**)&g->vstatus, sizeof(int))) != hipSuccess) goto fail;
    if (flags & DDMP_GV_REQUIRE_SYM) g->ew_t = g->ew;            // symmetric values by contract: one array serves both operators
    else if ((e = hipMalloc((void**)&g->ew_t, sizeof(float) * ne1)) != hipSuccess) goto fail;
    st = ddmp_graph_set_values(g, nullptr, nullptr);             // the values of all-ones weights
    if (st == DDMP_OK && (e = hipDeviceSynchronize()) != hipSuccess) goto fail;
    if (st != DDMP_OK) { ddmp_graph_destroy(g); return st; }
    *out = g;
    return DDMP_OK;
fail:
    ddmp_graph_destroy(g);
    return (int)e;
}

extern "C" int ddmp_graph_destroy(ddmp_graph* g) {
    if (!g) return DDMP_OK;
    if (g->ee_ptr) (void)hipFree(g->ee_ptr);
    if (g->ee_idx) (void)hipFree(g->ee_idx);
    if (g->eid) (void)hipFree(g->eid);
    if (g->mirror) (void)hipFree(g->mirror);
    if (g->a) (void)hipFree(g->a);
    if (g->ge) (void)hipFree(g->ge);
    if (g->vstatus) (void)hipFree(g->vstatus);
    if (g->ew_t && g->ew_t != g->ew) (void)hipFree(g->ew_t);
    if (g->rowptr) (void)hipFree(g->rowptr);
    if (g->col) (void)hipFree(g->col);
    if (g->dinv) (void)hipFree(g->dinv);
    if (g->pl_ptr) (void)hipFree(g->pl_ptr);
    if (g->pl_col) (void)hipFree(g->pl_col);
    if (g->lcol) (void)hipFree(g->lcol);
    if (g->ew) (void)hipFree(g->ew);
    if (g->pl_split) (void)hipFree(g->pl_split);
    if (g->heavy) (void)hipFree(g->heavy);
    delete g;
    return DDMP_OK;
}

extern "C" int ddmp_graph_info(const ddmp_graph* g, int64_t* n_rows, int64_t* n_cols, int64_t* nnz,
                               int* max_row_nnz) {
    ARG_TRY(g);
    if (n_rows) *n_rows = g->n_rows;
    if (n_cols) *n_cols = g->n_cols;
    if (nnz) *nnz = g->nnz;
    if (max_row_nnz) *max_row_nnz = g->max_row_nnz;
    return DDMP_OK;
}

extern "C" int ddmp_graph_patch_info(const ddmp_graph* g, int* patch_kd, int* n_heavy, int* n_split) {
    ARG_TRY(g);
    if (patch_kd) *patch_kd = g->max_patch > 0 ? g->patch_kd : 0;
    if (n_heavy) *n_heavy = g->n_heavy;
    if (n_split) *n_split = g->n_split;
    return DDMP_OK;
}

extern "C" int ddmp_graph_tables(const ddmp_graph* g, const int32_t** rowptr, const int32_t** col,
                                 const float** dinv) {
    ARG_TRY(g);
    if (rowptr) *rowptr = g->rowptr;
    if (col) *col = g->col;
    if (dinv) *dinv = g->dinv;
    return DDMP_OK;
}

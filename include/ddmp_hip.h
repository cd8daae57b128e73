/* libddmp_hip -- C ABI of the MI355X (gfx950) dual-GCN mesh-denoising hot path.
 *
 * Drop-in boundary: the reference (astaka-pe/Dual-DMP) has no FFI layer;
 * its hot path calls the Python operator API of torch_geometric / torch at
 *   util/networks.py:15-26,51-62,76-87,112-123   GCNConv(in,out)(x, edge_index)
 *   util/networks.py:31-44,64-67,125-129         BatchNorm1d / LeakyReLU / Linear heads
 *   util/loss.py:16,37,55,86,140,261             the five losses + mad
 *   main.py:106-110                              backward, clip_grad_norm_, Adam.step
 * This library is what a ctypes/cffi binding for that path binds instead.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - matrices are row-major float32 with an explicit leading dimension (elements);
 *   - the library never allocates or frees caller-visible memory: outputs and workspaces are
 *     caller-owned (PyTorch tensors in the Python host side); only ddmp_graph owns device memory;
 *   - work is enqueued on the caller's hipStream_t (void* here so the header needs no HIP);
 *     nothing synchronises the stream except the *_host helpers and ddmp_graph_create;
 *   - return value: 0 = OK, < 0 = invalid argument (DDMP_E*), > 0 = hipError_t;
 *     nothing throws across the ABI.
 */
#ifndef DDMP_HIP_H
#define DDMP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points declared in this header are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define DDMP_OK 0
#define DDMP_EINVAL (-1)      /* bad argument (null pointer, negative size, unsupported width) */
#define DDMP_ERANGE (-2)      /* index out of range in an input table */
#define DDMP_ENOMEM (-3)      /* host allocation failed */
#define DDMP_EWORKSPACE (-4)  /* caller workspace too small */

#define DDMP_ABI_VERSION 3      /* 3: per-call options (ddmp_opts, the *_o entry points);
                                   2: ddmp_next_pending, ddmp_gemm_forget_planes; additions only otherwise (the *_bf16 and
                                   dtype-tagged entry points) */

typedef struct ddmp_graph ddmp_graph;
typedef void* ddmp_stream;    /* hipStream_t */

int ddmp_abi_version(void);
const char* ddmp_status_string(int status);

/* ------------------------------------------------------------------ graph (gcn_norm, once)
 * Replaces the per-call `gcn_norm` of PyG 2.2.0 GCNConv (cached=False: recomputed 24x per step
 * in the reference, util/networks.py:51-62).  edge_index is the reference's [2, nnz] int64
 * tensor (row 0 = source j, row 1 = target i; util/datamaker.py:90-92), no self loops needed:
 * explicit self loops are dropped and exactly one per node is added (add_remaining_self_loops),
 * multi-edges keep their multiplicity.  CSR row i lists the sources of i (ascending) plus i.
 * dinv[i] = (1 + in-degree(i))^-1/2.
 */
int ddmp_csr_build_host(int64_t n_nodes, int64_t nnz, const int64_t* edge_index_host,
                        int32_t* rowptr_host /*[n+1]*/, int32_t* col_host /*[nnz_out]*/,
                        float* dinv_host /*[n]*/, int64_t* nnz_out /*in: capacity, out: used*/);
/* breadth-first (Cuthill-McKee style) node order for gather locality: order[k] = old id */
int ddmp_csr_bfs_order_host(int64_t n_nodes, const int32_t* rowptr_host, const int32_t* col_host,
                            int32_t* order_host /*[n]*/);
/* recursive coordinate bisection of the node coordinates (xyz_host [n,3] float64) into leaves of exactly `leaf` nodes
 * (the last one may be shorter), every split along the longest axis of the subset's bounding box at a multiple of
 * `leaf`: order[k] = old id.  Consecutive ids form compact patches of the surface whose sizes are multiples of the
 * gather kernels' 64-row chunks (a chunk of a Morton order straddles several cells of the curve: 1.9 distinct
 * neighbour rows per output row on the vertex graph of a 1M-face mesh against 1.6 here). */
int ddmp_rcb_order_host(int64_t n_nodes, const double* xyz_host, int leaf, int32_t* order_host /*[n]*/);

int ddmp_graph_create(int64_t n_nodes, int64_t nnz, const int64_t* edge_index, int edge_index_on_device,
                      ddmp_graph** out);
/* from ready CSR tables on the host (partitioned graphs: n_rows owned rows, cols < n_cols) */
int ddmp_graph_create_csr_host(int64_t n_rows, int64_t n_cols, const int32_t* rowptr_host,
                               const int32_t* col_host, const float* dinv_host, ddmp_graph** out);
/* rows [row0, row1) of such tables as a graph of their own: output row i is node row0 + i, the columns keep the numbering of the
 * whole local graph (pass the same X, and Y + row0 * ldy).  The interior / boundary halves of a partitioned graph (SURVEY.md 8e:
 * the halo exchange of a layer travels while the rows that reference no halo row are aggregated -- dual-dmp_amd/dist.py) */
int ddmp_graph_create_csr_rows_host(int64_t n_rows_all, int64_t n_cols, const int32_t* rowptr_host, const int32_t* col_host,
                                    const float* dinv_host, int64_t row0, int64_t row1, ddmp_graph** out);
int ddmp_graph_destroy(ddmp_graph* g);
int ddmp_graph_info(const ddmp_graph* g, int64_t* n_rows, int64_t* n_cols, int64_t* nnz, int* max_row_nnz);
/* How the LDS-patch gather takes this graph's 64-row chunks: patch_kd = patch rows per LDS buffer / 32 (0: no patch tables,
 * every aggregation runs the lean gather), n_heavy = chunks that go to the lean gather in a second launch, n_split = the extra passes of the chunks walked
 * as 2 halves / 4 quarters inside the same launch (= their extra record slots).  Diagnostic (tests, DESIGN figures); any pointer may be NULL. */
int ddmp_graph_patch_info(const ddmp_graph* g, int* patch_kd, int* n_heavy, int* n_split);

/* ------------------------------------------------------------------ aggregation  Y = A_hat . f(X) (+ bias)
 * Replaces GCNConv.propagate (index_select * norm -> scatter_add) and the `+ bias`.
 * A_hat = D^-1/2 (A + I) D^-1/2 is symmetric for the reference's graphs, so the same call is
 * the backward aggregation.  Optional fused prologue f(x) = LeakyReLU(pro_scale[c]*x + pro_shift[c])
 * (the BatchNorm1d + LeakyReLU of the previous layer, util/networks.py:51-62) applied to every
 * gathered element; pass NULL/NULL for f = identity.  C must be > 0; the vector path needs
 * C % 4 == 0 and ldx, ldy % 4 == 0, other widths take a scalar path.
 */
int ddmp_spmm_f32(const ddmp_graph* g, const float* X, int64_t ldx, float* Y, int64_t ldy, int C,
                  const float* bias, const float* pro_scale, const float* pro_shift, float slope,
                  ddmp_stream stream);
/* 1: ddmp_spmm* runs its LDS-patch form for this graph and shape (graphs from 64k rows with <= 12 entries per row on average,
 * C >= 256; rows of any length -- the selection is per 64-row chunk since round 5, chunks the form cannot take go to the lean
 * gather; has_red: 0 | 1 the fused BatchNorm-backward reduction | 2 the fused statistics; dtype DDMP_BF16: plain, prologue and
 * statistics only): distinct rows of a chunk copied to LDS once, gathers from LDS -- csrc/spmm_patch.hip; same results either way */
int ddmp_spmm_patch_selected(const ddmp_graph* g, int C, int dtype, int has_pro, int has_red);
/* 1: where the LDS-patch form does not run, a C % 32 == 0 gather of this graph and these leading dimensions runs the lean gather;
 * 0: the slab kernel (DDMP_SPMM_LEAN=0, or offsets beyond the lean gather's 32 bits).  For tests that name a route. */
int ddmp_spmm_lean_selected(const ddmp_graph* g, int64_t ldx, int64_t ldy, int C);

/* ------------------------------------------------------------------ Chebyshev step (torch_geometric ChebConv, normalization="sym")
 * The second graph flavour: S = D^-1/2 A D^-1/2 WITHOUT self loops -- explicit self loops are dropped and none is added,
 * multi-edges keep their multiplicity, CSR row i lists the sources of i (ascending), dinv[i] = in-degree(i)^-1/2 and 0 for a node
 * without edges (PyG's inf -> 0), whose row is empty.  Only symmetric edge lists (both directions present, as every graph of
 * this project is) give the S that ChebConv means: the same handle then serves the backward pass.  The handle is an ordinary
 * ddmp_graph: every ddmp_spmm* entry point takes it.
 */
int ddmp_csr_build_sym_host(int64_t n_nodes, int64_t nnz, const int64_t* edge_index_host,
                            int32_t* rowptr_host /*[n+1]*/, int32_t* col_host /*[nnz_out]*/,
                            float* dinv_host /*[n]*/, int64_t* nnz_out /*in: capacity (nnz suffices), out: used*/);
int ddmp_graph_create_sym(int64_t n_nodes, int64_t nnz, const int64_t* edge_index, int edge_index_on_device,
                          ddmp_graph** out);
/* One step of a three-term recurrence per launch -- the gather with an affine epilogue, float32:
 *     Y[i,:] = a * (dinv_i * sum_{e in row i} dinv_{col e} * X[col e,:]) + b * X[i,:] + c * Z[i,:] + d * Z2[i,:]
 * (T_k = 2 L^ T_{k-1} - T_{k-2} with L^ = alpha S + beta I: a = 2 alpha, b = 2 beta, c = -1, Z = T_{k-2}; the Clenshaw backward
 * uses both addends).  Z, Z2 nullable (their coefficient is then ignored); b == 0 reads no X[i,:].  Y may alias Z or Z2 (an
 * output row reads only its own row of them); Y must not alias X (DDMP_EINVAL).  X needs n_cols >= n_rows rows.  A row without
 * entries gives b X + c Z + d Z2.  No atomics, the gather's fixed summation order.  Widths as ddmp_spmm_f32: the vector
 * kernels need C % 4 == 0, leading dimensions % 4 == 0 and 16-byte aligned pointers, anything else takes the scalar kernel. */
int ddmp_spmm_axpby_f32(const ddmp_graph* g, const float* X, int64_t ldx, float* Y, int64_t ldy, const float* Z /*nullable*/,
                        int64_t ldz, const float* Z2 /*nullable*/, int64_t ldz2, int C, float a, float b, float c, float d,
                        ddmp_stream stream);

/* ------------------------------------------------------------------ valued graphs (edge_weight of GCNConv / ChebConv)
 * A third graph flavour whose STRUCTURE is built once per edge_index and whose VALUES are set on the device per weight version.
 * The structure is coalesced: one CSR entry per (target, source) pair, columns ascending, duplicates merged; three maps stay on
 * the device: entry -> its input edges in input order, input edge -> entry, entry (i, j) -> entry (j, i) ("mirror").  The edge
 * structure must be symmetric: an entry without mirror is DDMP_EINVAL.  flags:
 *   DDMP_GV_LOOPS      PyG add_remaining_self_loops: explicit self loops leave the edge list, every node gets ONE loop entry whose
 *                      value is the weight of its LAST explicit loop in input order, or `fill` (1; 2 with DDMP_GV_IMPROVED)
 *   DDMP_GV_NORMALIZE  entry value s_i a_e s_j, s_i = (sum of a_e over row i)^-1/2 (0 where the sum is 0); without it: a_e
 *   DDMP_GV_DROP_LOOPS explicit self loops are dropped and none is added (ChebConv's S)
 *   DDMP_GV_REQUIRE_SYM  the coalesced values must be symmetric bit for bit (ChebConv); reported by ddmp_graph_values_status
 * Until ddmp_graph_set_values has run, a valued graph holds the values of all-ones weights. */
#define DDMP_GV_LOOPS 1
#define DDMP_GV_IMPROVED 2
#define DDMP_GV_NORMALIZE 4
#define DDMP_GV_DROP_LOOPS 8
#define DDMP_GV_REQUIRE_SYM 16
#define DDMP_GV_VALUED 256        /* (internal marker of the handle) */
/* ddmp_graph_values_status bits */
#define DDMP_GV_ENONFINITE 1      /* a weight (or a coalesced sum) is NaN or infinite */
#define DDMP_GV_ENEGDEG 2         /* a node's weighted degree is negative (PyG would produce NaN) */
#define DDMP_GV_ENOTSYM 4         /* DDMP_GV_REQUIRE_SYM and a_ij != a_ji */
/* Host structure builder (no GPU): capacity of col / ee_ptr / mirror = *n_entries on entry (nnz + n_nodes always suffices; ee_ptr
 * needs one more), ee_idx and eid hold nnz.  eid[k] = -1 for an input edge that has no entry (a dropped or overridden loop). */
int ddmp_csr_build_valued_host(int64_t n_nodes, int64_t nnz, const int64_t* edge_index_host, int flags,
                               int32_t* rowptr_host /*[n+1]*/, int32_t* col_host, int32_t* ee_ptr_host, int32_t* ee_idx_host,
                               int32_t* eid_host, int32_t* mirror_host, int64_t* n_entries /*in: capacity, out: used*/);
int ddmp_graph_create_valued(int64_t n_nodes, int64_t nnz, const int64_t* edge_index, int edge_index_on_device, int flags,
                             ddmp_graph** out);
/* Values of one weight version, on the device, no host round trip: a_e = sum of the entry's input weights in input order
 * (float32; `fill` for a loop entry without explicit loop), deg_i = sum of a_e in CSR order, s_i = (float)(1 / sqrt((double)deg_i)),
 * factors a_e s_j and a_mirror(e) s_j.  w: device float32 [nnz], NULL = all ones.  Asynchronous on `stream`. */
int ddmp_graph_set_values(ddmp_graph* g, const float* w /*nullable*/, ddmp_stream stream);
/* The validation bits of the last ddmp_graph_set_values (synchronises `stream`). */
int ddmp_graph_values_status(const ddmp_graph* g, int* status_host, ddmp_stream stream);
/* Copies of the value arrays into caller-owned device buffers (each nullable): ew, ew_t, a [entries], s [n] (ones when not
 * normalising). */
int ddmp_graph_export_values(const ddmp_graph* g, float* ew, float* ew_t, float* a, float* s, ddmp_stream stream);
/* The gather with the TRANSPOSED values on the same structure: Y = A^T X + bias where ddmp_spmm_f32 gives A X + bias. */
int ddmp_spmm_t_f32(const ddmp_graph* g, const float* X, int64_t ldx, float* Y, int64_t ldy, int C, const float* bias /*nullable*/,
                    ddmp_stream stream);
/* Per-entry gradient (SDDMM over the CSR): G[e] = sum_c dY[row(e), c] * H[col(e), c], float32 products and accumulation, fixed
 * summation order (bitwise reproducible, no atomics).  Any ddmp_graph; G has one float per CSR entry. */
int ddmp_sddmm_f32(const ddmp_graph* g, const float* dY, int64_t lddy, const float* H, int64_t ldh, int C, float* G,
                   ddmp_stream stream);
/* dL/dw of the input edges from G = dL/dA per entry (ddmp_sddmm_f32) through the normalisation of a valued graph:
 * g_e = s_i s_j G_e - 1/2 s_i^3 (r_i + c_i), r_i = sum_{e in row i} a_e s_j G_e, c_i = sum_{e in row i} a_m(e) s_j G_m(e)
 * (g_e = G_e when not normalising); dw[k] = g_eid[k], 0 for an edge without entry.  dw: device float32 [nnz].
 * NOT reentrant per handle: the entries' gradient passes through scratch the handle owns, as the values themselves do --
 * ddmp_graph_set_values, ddmp_graph_weight_grad and the gathers of ONE valued graph must be ordered on one stream (or by events). */
int ddmp_graph_weight_grad(const ddmp_graph* g, const float* G, float* dw, ddmp_stream stream);

/* ------------------------------------------------------------------ graph attention (torch_geometric GATConv)
 * float32.  Hf is the projected feature matrix [n, heads * C] (head-major columns: Hf[i, h * C + c]), any leading dimension.
 * The graph is a VALUED graph (ddmp_graph_create_valued with DDMP_GV_LOOPS or 0) left at its all-ones values: its a_e is the
 * multiplicity of the coalesced entry, and a softmax over a multiset of edges equals the softmax with a_e exp(z_e) terms.
 * Per-entry arrays (alpha, ds) are entry-major [entries, heads]; per-node arrays (s_src, s_dst, ds_src, ds_dst) are contiguous
 * [n, heads].  No atomics, fixed summation orders: two calls give the same bits.  The vector kernels need C % 4 == 0, leading
 * dimensions % 4 == 0 and 16-byte aligned matrices; anything else takes scalar kernels.  An unvalued graph is DDMP_EINVAL.
 *
 * scores:    s_src[i,h] = sum_c Hf[i,h,c] att_src[h,c], s_dst likewise (att_*: [heads, C] contiguous). */
int ddmp_gat_scores_f32(const float* Hf, int64_t ldh, int64_t n_rows, int heads, int C, const float* att_src, const float* att_dst,
                        float* s_src, float* s_dst, ddmp_stream stream);
/* forward:   z_e = leaky_relu(s_src[col e, h] + s_dst[row e, h], slope), alpha_e = a_e exp(z_e - max_row z) / sum_row a_e exp(..)
 *            (written to alpha, saved for the backward), Y[i,h,:] = sum_{e in row i} alpha_e Hf[col e, h, :] (+ bias[h * C + c],
 *            nullable).  One launch.  A row without entries gets the bias alone.  exp arguments are <= 0. */
int ddmp_gat_fwd_f32(const ddmp_graph* g, const float* Hf, int64_t ldh, int heads, int C, const float* s_src, const float* s_dst,
                     float slope, const float* bias /*nullable*/, float* alpha, float* Y, int64_t ldy, ddmp_stream stream);
/* backward, edge side:  dalpha_e = dOut[row e, h, :] . Hf[col e, h, :], delta = sum_row alpha_e dalpha_e,
 *            ds_e = alpha_e (dalpha_e - delta) leaky'(z_e) (z_e recomputed from the scores) -> ds [entries, heads];
 *            ds_dst[i,h] = sum_{e in row i} ds_e. */
int ddmp_gat_bwd_edge_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Hf, int64_t ldh, int heads, int C,
                          const float* s_src, const float* s_dst, float slope, const float* alpha, float* ds, float* ds_dst,
                          ddmp_stream stream);
/* backward, node side:  ds_src[j,h] = sum_{e' in row j} ds[mirror e', h] and
 *            dHf[j,h,:] = sum_{e' in row j} alpha[mirror e', h] dOut[col e', h, :] + ds_src[j,h] att_src[h,:] + ds_dst[j,h] att_dst[h,:]
 *            (the structure is symmetric: row j's own entries enumerate the targets j feeds).  Writes dHf completely. */
int ddmp_gat_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, int heads, int C, const float* alpha, const float* ds,
                          const float* ds_dst, const float* att_src, const float* att_dst, float* dHf, int64_t lddh, float* ds_src,
                          ddmp_stream stream);
/* attention-vector gradient:  datt_src[h,c] = sum_i ds_src[i,h] Hf[i,h,c], datt_dst likewise with ds_dst; two stages, per-chunk
 * partials in the caller's workspace. */
size_t ddmp_gat_datt_workspace_bytes(int64_t n_rows, int heads, int C);
int ddmp_gat_datt_f32(const float* Hf, int64_t ldh, int64_t n_rows, int heads, int C, const float* ds_src, const float* ds_dst,
                      float* datt_src, float* datt_dst, void* workspace, size_t workspace_bytes, ddmp_stream stream);

/* ------------------------------------------------------------------ dynamic graph attention (torch_geometric GATv2Conv;
 * DESIGN.md 4.12).  float32.  Xl = lin_l(x) and Xr = lin_r(x) are [n, heads * C] (head-major columns), each with its own pointer
 * and leading dimension: column blocks of one packed row buffer [Xl | Xr], or the same matrix twice (share_weights).  att is
 * [heads, C] contiguous.  The graph is the attention graph above: a VALUED graph left at its all-ones values, a_e = the entry's
 * multiplicity.  Per-entry arrays (alpha, dz) are entry-major [entries, heads].  No atomics, fixed summation orders: two calls
 * give the same bits.  The vector kernels need C % 4 == 0, leading dimensions % 4 == 0 and 16-byte aligned matrices; anything
 * else takes scalar kernels.  An unvalued graph is DDMP_EINVAL.
 *
 * forward:   u_e[h,c] = Xl[col e, h, c] + Xr[row e, h, c], z_e[h] = sum_c att[h,c] leaky_relu(u_e[h,c], slope),
 *            alpha_e = a_e exp(z_e - max_row z) / sum_row a_e exp(..) (written to alpha, saved for the backward; z_e passes
 *            through the same array), Y[i,h,:] = sum_{e in row i} alpha_e Xl[col e, h, :] (+ bias[h * C + c], nullable).  One
 *            launch.  A row without entries gets the bias alone and writes no alpha.  exp arguments are <= 0. */
int ddmp_gatv2_fwd_f32(const ddmp_graph* g, const float* Xl, int64_t ldl, const float* Xr, int64_t ldr, int heads, int C,
                       const float* att, float slope, const float* bias /*nullable*/, float* alpha, float* Y, int64_t ldy,
                       ddmp_stream stream);
/* backward, edge side (row i's side):  dalpha_e = dOut[row e, h, :] . Xl[col e, h, :], delta = sum_row alpha_e dalpha_e,
 *            dz_e = alpha_e (dalpha_e - delta) -> dz [entries, heads];
 *            dXr[i,h,c] = sum_{e in row i} dz_e att[h,c] leaky'(u_e[h,c]) (u recomputed from a second gather of Xl; written
 *            completely, zeros on a row without entries) and, part non-null,
 *            part[i,h,c] = sum_{e in row i} dz_e leaky_relu(u_e[h,c]): the row's share of datt, [n, heads * C] with leading
 *            dimension ldp, reduced by ddmp_gatv2_datt_f32. */
int ddmp_gatv2_bwd_edge_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Xl, int64_t ldl, const float* Xr,
                            int64_t ldr, int heads, int C, const float* att, float slope, const float* alpha, float* dz, float* dXr,
                            int64_t lddr, float* part /*nullable*/, int64_t ldp, ddmp_stream stream);
/* backward, node side (node j's side, through the mirror map):
 *            dXl[j,h,c] = sum_{e' in row j} ( alpha[mirror e', h] dOut[col e', h, c]
 *                                             + dz[mirror e', h] att[h,c] leaky'(Xl[j,h,c] + Xr[col e', h, c]) )
 *            (the structure is symmetric: row j's own entries enumerate the targets j feeds).  Writes dXl completely. */
int ddmp_gatv2_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Xl, int64_t ldl, const float* Xr,
                            int64_t ldr, int heads, int C, const float* att, float slope, const float* alpha, const float* dz,
                            float* dXl, int64_t lddl, ddmp_stream stream);
/* attention-vector gradient:  datt[h,c] = sum_i part[i,h,c]; two stages, per-chunk partials in the caller's workspace, fixed
 * order. */
size_t ddmp_gatv2_datt_workspace_bytes(int64_t n_rows, int heads, int C);
int ddmp_gatv2_datt_f32(const float* part, int64_t ldp, int64_t n_rows, int heads, int C, float* datt, void* workspace,
                        size_t workspace_bytes, ddmp_stream stream);

/* ------------------------------------------------------------------ graph transformer (torch_geometric TransformerConv;
 * DESIGN.md 4.13).  float32.  Q = lin_query(x), K = lin_key(x), V = lin_value(x) and the skip term are [n, heads * C] (head-major
 * columns), each with its own pointer and leading dimension: column blocks of one packed row buffer [Q | K | V | S].  K and V
 * may be the same matrix.  scale multiplies the dot product (1 / sqrt(C) in the operator).  The graph is the attention graph
 * above: a VALUED graph left at its all-ones values, a_e = the entry's multiplicity.  Per-entry arrays (alpha, dz) are entry-major
 * [entries, heads].  No atomics, fixed summation orders: two calls give the same bits.  The vector kernels need C % 4 == 0, leading
 * dimensions % 4 == 0 and 16-byte aligned matrices; anything else takes scalar kernels.  heads * C < 2^24.  No output may be one
 * of the inputs.  An unvalued graph is DDMP_EINVAL.
 *
 * forward:   z_e[h] = scale * Q[row e, h, :] . K[col e, h, :], alpha_e = a_e exp(z_e - max_row z) / sum_row a_e exp(..) (written
 *            to alpha, saved for the backward; z_e passes through the same array),
 *            Y[i,h,:] = sum_{e in row i} alpha_e V[col e, h, :] (+ skip[i,h,:], nullable, leading dimension lds).  One launch.  A
 *            row without entries gets its skip row (or zeros) and writes no alpha.  exp arguments are <= 0. */
int ddmp_tconv_fwd_f32(const ddmp_graph* g, const float* Q, int64_t ldq, const float* K, int64_t ldk, const float* V, int64_t ldv,
                       int heads, int C, float scale, const float* skip /*nullable*/, int64_t lds, float* alpha, float* Y,
                       int64_t ldy, ddmp_stream stream);
/* backward, edge side (row i's side):  dalpha_e = dOut[row e, h, :] . V[col e, h, :], delta = sum_row alpha_e dalpha_e,
 *            dz_e = alpha_e (dalpha_e - delta) -> dz [entries, heads] (the gradient w.r.t. z_e);
 *            dQ[i,h,:] = scale sum_{e in row i} dz_e K[col e, h, :] (written completely, zeros on a row without entries). */
int ddmp_tconv_bwd_edge_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* K, int64_t ldk, const float* V,
                            int64_t ldv, int heads, int C, float scale, const float* alpha, float* dz, float* dQ, int64_t lddq,
                            ddmp_stream stream);
/* backward, node side (node j's side, through the mirror map; one launch, both neighbour streams in flight together):
 *            dK[j,h,:] = scale sum_{e' in row j} dz[mirror e', h] Q[col e', h, :],
 *            dV[j,h,:] = sum_{e' in row j} alpha[mirror e', h] dOut[col e', h, :]
 *            (the structure is symmetric: row j's own entries enumerate the targets j feeds) and, dS non-null, the skip term's
 *            gradient dS[j,:] = dOut[j,:] ([n, heads * C], leading dimension ldds).  Writes dK, dV (and dS) completely. */
int ddmp_tconv_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Q, int64_t ldq, int heads, int C,
                            float scale, const float* alpha, const float* dz, float* dK, int64_t lddk, float* dV, int64_t lddv,
                            float* dS /*nullable*/, int64_t ldds, ddmp_stream stream);

/* ------------------------------------------------------------------ residual gated graph convolution (torch_geometric
 * ResGatedGraphConv).  float32.  K = lin_key(x), Q = lin_query(x), V = lin_value(x) and the skip term are [n, C],
 * each with its own pointer and leading dimension: column blocks of one packed row buffer [K | Q | V | S].  The graph is the
 * attention graph above: a VALUED graph left at its all-ones values, a_e = the entry's multiplicity.  The gate
 * g = sigma(K[row e, :] + Q[col e, :]) is PER CHANNEL and is stored nowhere: there is no per-entry array, the backward launches
 * recompute the gate from the same rows.  sigma(x) = 1 / (1 + exp(-x)) is finite for every finite x.  No atomics, fixed summation
 * orders: two calls give the same bits.  The vector kernels need C % 4 == 0, leading dimensions % 4 == 0 and 16-byte aligned
 * matrices (and bias); anything else takes scalar kernels.  C < 2^24.  No output may be one of the inputs or another output.  An
 * unvalued graph is DDMP_EINVAL.
 *
 * forward:   Y[i,:] = skip[i,:] + bias + sum_{e in row i} a_e g_e (.) V[col e, :]  (skip [n, C] with leading dimension lds and bias
 *            [C] are each nullable).  One launch.  A row without entries gets skip[i,:] + bias exactly. */
int ddmp_rgate_fwd_f32(const ddmp_graph* g, const float* K, int64_t ldk, const float* Q, int64_t ldq, const float* V, int64_t ldv,
                       int C, const float* skip /*nullable*/, int64_t lds, const float* bias /*nullable*/, float* Y, int64_t ldy,
                       ddmp_stream stream);
/* backward, row side (row i's side):  dK[i,:] = sum_{e in row i} a_e dOut[i,:] (.) V[col e, :] (.) g_e (1 - g_e) (written
 *            completely, zeros on a row without entries). */
int ddmp_rgate_bwd_row_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* K, int64_t ldk, const float* Q,
                           int64_t ldq, const float* V, int64_t ldv, int C, float* dK, int64_t lddk, ddmp_stream stream);
/* backward, node side (node j's side; row j's own entries e' enumerate the targets i = col e' that j feeds -- the structure is
 *            symmetric -- with a = the multiplicity of the mirrored entry (i, j) and g = sigma(K[i,:] + Q[j,:])):
 *            dQ[j,:] = sum_{e'} a dOut[i,:] (.) V[j,:] (.) g (1 - g),   dV[j,:] = sum_{e'} a dOut[i,:] (.) g
 *            and, dS non-null, the skip term's gradient dS[j,:] = dOut[j,:] ([n, C], leading dimension ldds).  Writes dQ, dV (and
 *            dS) completely. */
int ddmp_rgate_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* K, int64_t ldk, const float* Q,
                            int64_t ldq, const float* V, int64_t ldv, int C, float* dQ, int64_t lddq, float* dV, int64_t lddv,
                            float* dS /*nullable*/, int64_t ldds, ddmp_stream stream);

/* ------------------------------------------------------------------ feature-steered convolution (torch_geometric FeaStConv;
 * DESIGN.md 4.9).  float32.  Hf is the projected feature matrix [n, heads * C] (head-major columns), P = X u^T the steering
 * projection [n, heads], each with its own pointer and leading dimension (they may be column blocks of one row buffer); c is
 * [heads].  The graph is the attention graph above: a VALUED graph left at its all-ones values, a_e = the entry's multiplicity.
 * Per-entry arrays (beta, dz) are entry-major [entries, heads]; rs is contiguous [n, heads].  No atomics, fixed summation orders:
 * two calls give the same bits.  The vector kernels need C % 4 == 0, leading dimensions of the [.., C]-wide matrices % 4 == 0 and
 * 16-byte aligned matrices; anything else takes scalar kernels.  heads <= 256.  An unvalued graph is DDMP_EINVAL.
 *
 * forward:   q_e[h] = softmax over the HEADS h of (P[col e, h] - P[row e, h] + c[h]) (exp arguments <= 0),
 *            beta_e[h] = a_e q_e[h] / deg_i with deg_i = sum_{e in row i} a_e (written to beta, saved for the backward;
 *            sum_h beta_e[h] = a_e / deg_i =: m_e, so q_e = beta_e / m_e needs no degree table),
 *            Y[i,:] = sum_{e in row i} sum_h beta_e[h] Hf[col e, h, :] (+ bias[C], nullable).  Y is [n, C].  One launch.  A row
 *            without entries gets the bias alone. */
int ddmp_feast_fwd_f32(const ddmp_graph* g, const float* Hf, int64_t ldh, const float* P, int64_t ldp, int heads, int C,
                       const float* c, const float* bias /*nullable*/, float* beta, float* Y, int64_t ldy, ddmp_stream stream);
/* backward, edge side:  g_e[h] = dOut[row e, :] . Hf[col e, h, :], delta_e = sum_h beta_e[h] g_e[h] / m_e,
 *            dz_e[h] = beta_e[h] (g_e[h] - delta_e) -> dz [entries, heads]; rs[i,h] = sum_{e in row i} dz_e[h].  dOut is [n, C].
 *            With heads == 1, dz and rs are exactly zero. */
int ddmp_feast_bwd_edge_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Hf, int64_t ldh, int heads, int C,
                            const float* beta, float* dz, float* rs, ddmp_stream stream);
/* backward, node side:  dHf[j,h,:] = sum_{e' in row j} beta[mirror e', h] dOut[col e', :]  (written completely) and
 *            dP[j,h] = sum_{e' in row j} dz[mirror e', h] - rs[j,h]  (the structure is symmetric: row j's own entries enumerate
 *            the targets j feeds).  dHf [n, heads * C] and dP [n, heads] each have their own leading dimension. */
int ddmp_feast_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, int heads, int C, const float* beta,
                            const float* dz, const float* rs, float* dHf, int64_t lddh, float* dP, int64_t lddp,
                            ddmp_stream stream);
/* offset gradient:  dc[h] = sum_i rs[i,h]; two stages, per-chunk partials in the caller's workspace, fixed order. */
size_t ddmp_feast_dc_workspace_bytes(int64_t n_rows, int heads);
int ddmp_feast_dc_f32(const float* rs, int64_t n_rows, int heads, float* dc, void* workspace, size_t workspace_bytes,
                      ddmp_stream stream);

/* ------------------------------------------------------------------ Gaussian-mixture convolution (torch_geometric GMMConv, mean
 * aggregation, separate_gaussians=False).  float32.  Hf is the projected feature matrix [n, K * C] (component-major
 * columns); attr holds the pseudo-coordinates of the INPUT edges, contiguous [input edges, dim], in the order of the edge list the
 * graph was created from; mu and sigma are contiguous [K, dim].  The graph is the attention graph above created with flags 0 (no
 * loop handling: every input edge belongs to exactly one entry) and left at its all-ones values; any other graph is DDMP_EINVAL.
 * Per-entry arrays (w, ge) are entry-major [entries, K].  K * dim <= 128, so the [n, 2 K dim] partials fit ddmp_feast_dc_f32.
 * No atomics, fixed summation orders: two calls give the same bits.  The vector kernels need C % 4 == 0, leading dimensions % 4 == 0
 * and 16-byte aligned matrices; anything else takes scalar kernels.
 *
 * forward:   gamma_t[k] = exp(-1/2 sum_d (attr[t,d] - mu[k,d])^2 / (1e-15 + sigma[k,d]^2)) per input edge t (exp arguments <= 0),
 *            w_e[k] = (1 / deg_i) sum_{t in the edges of entry e, input order} gamma_t[k] with deg_i = sum_{e in row i} a_e (written
 *            to w, saved for the backward),
 *            Y[i,:] = sum_{e in row i} sum_k w_e[k] Hf[col e, k, :] (+ R[i,:], nullable, own leading dimension) (+ bias[C], nullable).
 *            Y is [n, C].  One launch.  A row without entries gets R[i,:] + bias. */
int ddmp_gmm_fwd_f32(const ddmp_graph* g, const float* Hf, int64_t ldh, const float* attr, int dim, const float* mu,
                     const float* sigma, int K, int C, const float* R /*nullable*/, int64_t ldr, const float* bias /*nullable*/,
                     float* w, float* Y, int64_t ldy, ddmp_stream stream);
/* backward, edge side:  G_e[k] = dOut[row e, :] . Hf[col e, k, :] -> ge [entries, K] (scratch of the call); with
 *            c_t[k] = gamma_t[k] G_e[k] / deg_i and inv[k,d] = 1 / (1e-15 + sigma[k,d]^2), per ROW the sums over its entries' edges
 *            parts[i, k dim + d]         = sum_t c_t[k] (attr[t,d] - mu[k,d]) inv[k,d]                      (the dmu terms)
 *            parts[i, K dim + k dim + d] = sum_t c_t[k] (attr[t,d] - mu[k,d])^2 sigma[k,d] inv[k,d]^2       (the dsigma terms)
 *            (an entry's edges in input order, the row's entries by a fixed xor tree per 8 in CSR order; a row without entries
 *            writes zeros; dmu / dsigma are the column sums: ddmp_feast_dc_f32 with heads = 2 K dim), and, dattr non-null,
 *            dattr[t,d] = - sum_k c_t[k] (attr[t,d] - mu[k,d]) inv[k,d] for every input edge ([input edges, dim]).  One launch. */
int ddmp_gmm_bwd_edge_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Hf, int64_t ldh, const float* attr,
                          int dim, const float* mu, const float* sigma, int K, int C, float* ge, float* parts,
                          float* dattr /*nullable*/, ddmp_stream stream);
/* backward, node side:  dHf[j,k,:] = sum_{e' in row j} w[mirror e', k] dOut[col e', :] (written completely) and, dR non-null,
 *            dR[j,:] = dOut[j,:] (the root block's gradient; dHf and dR are meant to be column blocks of one row buffer). */
int ddmp_gmm_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, int K, int C, const float* w, float* dHf,
                          int64_t lddh, float* dR /*nullable*/, int64_t lddr, ddmp_stream stream);

/* ------------------------------------------------------------------ B-spline convolution (torch_geometric SplineConv, degree 1,
 * mean or add aggregation).  float32.  Hf is the projected feature matrix [n, K * C] with K = prod(kernel_size)
 * blocks of C columns, block index = sum_d index_d * prod_{d' < d} kernel_size[d'] (the first coordinate varies fastest); attr holds
 * the pseudo-coordinates of the INPUT edges, contiguous [input edges, dim], in the order of the edge list the graph was created
 * from; kernel_size and is_open are HOST arrays of dim ints (kernel_size[d] >= 1, is_open[d] 0 or 1).  1 <= dim <= 5 and
 * K * C < 2^24; anything else is DDMP_EINVAL.  The graph is the one of the Gaussian-mixture kernels (flags 0, all-ones values).
 * With v_d = attr[t,d] (kernel_size[d] - is_open[d]), f_d = v_d - floor(v_d), s in [0, 2^dim) and s_d its bit d:
 *            b_{t,s} = prod_d (s_d ? f_d : 1 - f_d),  k_{t,s} = sum_d ((floor(v_d) + s_d) mod kernel_size[d]) prod_{d' < d} kernel_size[d']
 * (a true non-negative modulo, clamped into [0, kernel_size[d]): the block index is in range for EVERY attr value; the result for
 * pseudo-coordinates outside [0, 1] or non-finite is otherwise unspecified).  Nothing is stored per edge: both launches evaluate
 * the basis from attr.  No atomics, fixed summation orders: two calls give the same bits.  The vector kernels need C % 4 == 0,
 * leading dimensions % 4 == 0 and 16-byte aligned matrices; anything else takes scalar kernels.
 *
 * forward:   Y[i,:] = (1 / n_i) sum_{e in row i} sum_{t in the edges of e, input order} sum_s b_{t,s} Hf[col e, k_{t,s}, :]
 *                     (+ R[i,:], nullable, own leading dimension) (+ bias[C], nullable),
 *            n_i = the number of input edges into i (mean != 0) or 1 (mean == 0).  Only the 2^dim selected blocks of a gathered
 *            row are read.  Y is [n, C].  One launch.  A row without entries gets R[i,:] + bias. */
int ddmp_spline_fwd_f32(const ddmp_graph* g, const float* Hf, int64_t ldh, const float* attr, int dim, const int32_t* kernel_size,
                        const int32_t* is_open, int C, const float* R /*nullable*/, int64_t ldr, const float* bias /*nullable*/,
                        int mean, float* Y, int64_t ldy, ddmp_stream stream);
/* backward, node side:  dHf[j,k,:] = sum_{e' in row j} sum_{t in the edges of mirror e'} [sum_{s: k_{t,s} = k} b_{t,s}] dOut[col e', :] / n_{col e'}
 *            written completely (a block no edge selects is zero; the structure is symmetric: row j's own entries enumerate the
 *            targets j feeds, the mirrored entry holds the edges j -> col e') and, dR non-null, dR[j,:] = dOut[j,:] (the root
 *            block's gradient; dHf and dR are meant to be column blocks of one row buffer).  One launch. */
int ddmp_spline_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* attr, int dim,
                             const int32_t* kernel_size, const int32_t* is_open, int C, int mean, float* dHf, int64_t lddh,
                             float* dR /*nullable*/, int64_t lddr, ddmp_stream stream);

/* ------------------------------------------------------------------ max aggregation (torch_geometric EdgeConv with a Linear edge
 * function).  float32.  The graph is the attention graph above (a VALUED graph; its values are not read: the
 * structure is coalesced and a duplicate edge cannot change a maximum); an unvalued graph is DDMP_EINVAL.  Every matrix has its own
 * pointer and leading dimension (A and B, dA and dB are meant to be the column blocks of one row buffer).  No atomics, fixed orders:
 * two calls give the same bits.  The vector kernels need C % 4 == 0, leading dimensions % 4 == 0 and 16-byte aligned matrices;
 * anything else takes scalar kernels.
 *
 * forward:   Y[i,c] = A[i,c] + max_{e in row i} B[col e, c] (A nullable: 0), arg[i,c] = col e of the winning entry (int32
 *            [n, C]; nullable: not stored).  Ties go to the first entry in CSR order, i.e. the smallest source id (strict >
 *            from the row's first entry).  A row without entries gets Y = 0 (not A) and arg = -1.  One launch. */
int ddmp_gather_max_f32(const ddmp_graph* g, const float* B, int64_t ldb, const float* A /*nullable*/, int64_t lda, int C, float* Y,
                        int64_t ldy, int32_t* arg /*nullable*/, int64_t ldarg, ddmp_stream stream);
/* backward:  dA[j,:] = dG[j,:] for a row with entries, 0 for one without;
 *            dB[j,c] = sum_{e' in row j} (arg[col e', c] == j ? dG[col e', c] : 0) in CSR order (the structure is symmetric: row
 *            j's own entries enumerate the rows j feeds; arg holds node ids, so no mirror map is read).  dG is [n, C].  One launch. */
int ddmp_gather_max_bwd_f32(const ddmp_graph* g, const float* dG, int64_t lddg, const int32_t* arg, int64_t ldarg, int C, float* dA,
                            int64_t ldda, float* dB, int64_t lddb, ddmp_stream stream);

/* ------------------------------------------------------------------ max aggregation of an edge-conditioned message
 * (torch_geometric PPFConv with a Linear local_nn).  float32.  The graph is the attention graph above (a VALUED graph
 * with its mirror map); an unvalued graph is DDMP_EINVAL.  No atomics, no LDS, fixed orders: two calls give the same bits.  The
 * vector kernels need C % 4 == 0, leading dimensions % 4 == 0 and 16-byte aligned matrices; anything else takes scalar kernels.
 *
 * features:  F[e,:] = [ |d|, angle(n_i, d), angle(n_j, d), angle(n_i, n_j) ] for every COALESCED entry e = (i, j = col e), with
 *            d = pos[j] - pos[i] and angle(a, b) = atan2(|a x b|, a . b); the cross products are compensated differences of
 *            products.  An entry with j == i gets exactly 0.  pos, normal: [n, 3] with leading dimensions ldp, ldn >= 3; F:
 *            contiguous [entries, 4], 16-byte aligned.  One thread per entry, one launch. */
int ddmp_ppf_entries_f32(const ddmp_graph* g, const float* pos, int64_t ldp, const float* normal, int64_t ldn, float* F,
                         ddmp_stream stream);
/* forward:   Y[i,c] = max_{e in row i} (B[col e, c] + sum_d F[e,d] E[d,c]) (B nullable: 0; E: contiguous [4, C]), arg[i,c] = col e
 *            of the winning entry (int32 [n, C]; nullable: not stored).  The message is fma(F3, E3, fma(F2, E2, fma(F1, E1,
 *            F0 * E0))) + B, in that order.  Ties go to the first entry in CSR order (strict > from the row's first entry).  A row
 *            without entries gets Y = 0 and arg = -1.  One launch. */
int ddmp_gather_max_attr_f32(const ddmp_graph* g, const float* B /*nullable*/, int64_t ldb, const float* F, const float* E, int C,
                             float* Y, int64_t ldy, int32_t* arg /*nullable*/, int64_t ldarg, ddmp_stream stream);
/* backward:  dB[j,c] = sum_{e' in row j} (arg[col e', c] == j ? dG[col e', c] : 0) in CSR order (the structure is symmetric, as
 *            for ddmp_gather_max_bwd_f32) and, P non-null, the shares of dE[d,c] = sum_i dG[i,c] F[entry(i, arg[i,c]), d] of every
 *            8 consecutive rows: P contiguous [ceil(n / 8), 4, C]; its column sum (ddmp_gatv2_datt_f32 with heads = 4) is dE.
 *            One launch. */
int ddmp_gather_max_attr_bwd_f32(const ddmp_graph* g, const float* dG, int64_t lddg, const int32_t* arg, int64_t ldarg,
                                 const float* F, int C, float* dB, int64_t lddb, float* P /*nullable*/, ddmp_stream stream);

/* ------------------------------------------------------------------ neighbour statistics (torch_geometric SAGEConv with mean, add,
 * max and min aggregation, one of them or several at once).  float32.  The graph is the one of the Gaussian-mixture
 * kernels: the attention graph created with flags 0 (no loop handling, so a_e is the number of input edges of entry e) and left at
 * its all-ones values; an unvalued graph or one with loop handling is DDMP_EINVAL.  Every matrix has its own pointer and leading
 * dimension (the outputs are meant to be column blocks of one row buffer).  No atomics, fixed orders: two calls give the same bits,
 * and a block of a fused call has the bits of the same block requested alone.  The vector kernels need C % 4 == 0, leading
 * dimensions % 4 == 0 and 16-byte aligned matrices (bias included); anything else takes scalar kernels.
 *
 * forward:   every neighbour row X[col e, :] is loaded once and feeds any non-empty subset of three outputs (a null pointer: not
 *            requested; none at all is DDMP_EINVAL):
 *            S[i,c]  = w_i sum_{e in row i} a_e X[col e, c] in CSR order (+ R[i,c], nullable, own leading dimension) (+ bias[c],
 *                      nullable), w_i = 1 / deg_i (mean != 0) or 1, deg_i = sum_{e in row i} a_e = the number of input edges into
 *                      i (duplicates and explicit loops count).  A row without entries gets R[i,:] + bias, or zeros.  mean, R and
 *                      bias need S.
 *            Mx[i,c] = max_{e in row i} X[col e, c], argmx[i,c] = col e of the winning entry (int32 [n, C]; nullable: not stored).
 *                      Multiplicities are ignored.  Ties go to the first entry in CSR order, i.e. the smallest source id (strict >
 *                      from the row's first entry).  A row without entries gets 0 and -1.
 *            Mn, argmn: the same for the minimum, with a strict <.
 *            invdeg[i] (nullable, [n]) = 1 / deg_i, 0 for a row without entries: saved for the backward.
 *            Xcopy[i,:] (nullable, own leading dimension) = X[i,:]: the row's own features copied into a column block of the
 *                      output buffer.
 *            No output may alias X or another operand.  One launch. */
int ddmp_gather_stats_f32(const ddmp_graph* g, const float* X, int64_t ldx, int C, int mean, const float* R /*nullable*/, int64_t ldr,
                          const float* bias /*nullable*/, float* S /*nullable*/, int64_t lds, float* Mx /*nullable*/, int64_t ldmx,
                          int32_t* argmx /*nullable*/, int64_t ldamx, float* Mn /*nullable*/, int64_t ldmn,
                          int32_t* argmn /*nullable*/, int64_t ldamn, float* invdeg /*nullable*/, float* Xcopy /*nullable*/,
                          int64_t ldxc, ddmp_stream stream);
/* backward, node side (the structure is symmetric: row j's own entries e' enumerate the targets i = col e' that j feeds, the
 *            mirrored entry holds the multiplicity of j -> i, arg holds node ids):
 *            dX[j,c] = dX0[j,c] + sum_{e' in row j} ( a_{mirror e'} w_i dS[i,c] + (argmx[i,c] == j ? dMx[i,c] : 0)
 *                                                                              + (argmn[i,c] == j ? dMn[i,c] : 0) ) in CSR order,
 *            w_i = invdeg[i], or 1 with invdeg null (the sum).  Each of the three gradient streams is nullable (dMx comes with
 *            argmx, dMn with argmn; none at all is DDMP_EINVAL) and only the requested ones are loaded; dX0 (nullable) is the
 *            gradient that arrives through the Xcopy block.  dX is written completely: a row without entries gets dX0, or zeros.
 *            dR[j,:] = dS[j,:] (nullable; needs dS): the gradient of the forward's R block.  One launch. */
int ddmp_gather_stats_bwd_f32(const ddmp_graph* g, int C, const float* dS /*nullable*/, int64_t ldds,
                              const float* invdeg /*nullable*/, const float* dMx /*nullable*/, int64_t lddmx,
                              const int32_t* argmx /*nullable*/, int64_t ldamx, const float* dMn /*nullable*/, int64_t lddmn,
                              const int32_t* argmn /*nullable*/, int64_t ldamn, const float* dX0 /*nullable*/, int64_t lddx0,
                              float* dX, int64_t lddx, float* dR /*nullable*/, int64_t lddr, ddmp_stream stream);

/* ------------------------------------------------------------------ neighbour moments (PNAConv): mean-or-sum,
 * max, min and std-or-var of the neighbours' rows in one sweep, on the graph and with the rules of the neighbour statistics above
 * (same fma order, ONE multiplication for the mean, strict comparisons from the row's first entry: the smallest source id wins a
 * tie).  No atomics, fixed orders, every output written completely; a block of a fused call has the bits of the same block
 * requested alone, and without R and with tw == C the S, Mx, Mn blocks and the args have the bits of ddmp_gather_stats_f32.
 *
 * forward:   every neighbour row B[col e, :] is loaded once and feeds any non-empty subset of four blocks (a null pointer: not
 *            requested; none at all is DDMP_EINVAL):
 *            S       = w_i sum_e a_e B[col e, c], w_i = 1 / deg_i (mean != 0) or 1;
 *            Mx, argmx (nullable), Mn, argmn (nullable): as in ddmp_gather_stats_f32;
 *            V       = the second central moment of the row's entries, from sums SHIFTED by the row's first entry K = B[col rbase, c]:
 *                      d_e = B[col e, c] - K, m1 = sum a_e d_e, m2 = sum a_e d_e d_e, mu = K + m1 w, var = max(m2 w - (m1 w)^2, 0),
 *                      w = 1 / deg_i; V = var, or (as_std != 0) var > 1e-5 ? sqrt(var) : 0 (PyG 2.2.0's StdAggregation).  V comes
 *                      with mu [n, C] (the neighbour mean, saved for the backward; DDMP_EINVAL without it, or mu without V).
 *            R (nullable, [n, C]): on a row WITH entries R[i,c] is added to the mean, to Mx and to Mn (one unfused addition each)
 *                      and deg_i R[i,c] to the sum; never to V.  A row without entries gets 0 in every block whatever R is, -1
 *                      in the args, 0 in mu and invdeg.
 *            tw, tstride: column c of S, Mx, Mn, V lands at base + row * ld + (c / tw) * tstride + c % tw (tower-major: the row
 *                      buffer can be [tower][aggregator][tw]); tw must divide C; tw == C is the plain layout (tstride ignored).
 *                      The args, mu and invdeg (nullable, [n]: 1 / deg_i) are always plain.  The vector kernels need C, tw, tstride
 *                      and every leading dimension % 4 == 0 and 16-byte aligned matrices; anything else takes scalar kernels.
 *            No output may alias B, R or another output.  One launch. */
int ddmp_gather_moments_f32(const ddmp_graph* g, const float* B, int64_t ldb, int C, int mean, int as_std, const float* R /*nullable*/,
                            int64_t ldr, int tw, int64_t tstride, float* S /*nullable*/, int64_t lds, float* Mx /*nullable*/,
                            int64_t ldmx, int32_t* argmx /*nullable*/, int64_t ldamx, float* Mn /*nullable*/, int64_t ldmn,
                            int32_t* argmn /*nullable*/, int64_t ldamn, float* V /*nullable*/, int64_t ldv, float* mu /*nullable*/,
                            int64_t ldmu, float* invdeg /*nullable*/, ddmp_stream stream);
/* backward, node side (symmetric structure, as ddmp_gather_stats_bwd_f32):
 *            dB[j,c] = sum_{e' in row j} ( a w_i dS[i,c] + (argmx[i,c] == j ? dMx[i,c] : 0) + (argmn[i,c] == j ? dMn[i,c] : 0) )
 *                      + B[j,c] sum_{e' in row j} a w_i dQ[i,c],   i = col e', a = a_{mirror e'},
 *            w_i = invdeg[i], or 1 with invdeg null.  dQ (nullable; needs dS and B) is the second stream of the std / var chain
 *            rule: with G = dStd / std where std > 0 (else 0), or 2 dVar, the caller passes dQ = G and adds -G mu to dS.
 *            dB is written completely: a row without entries gets zeros.
 *            One launch. */
int ddmp_gather_moments_bwd_f32(const ddmp_graph* g, int C, const float* dS /*nullable*/, int64_t ldds, const float* dQ /*nullable*/,
                                int64_t lddq, const float* B /*nullable*/, int64_t ldb,
                                const float* invdeg /*nullable*/, const float* dMx /*nullable*/, int64_t lddmx,
                                const int32_t* argmx /*nullable*/, int64_t ldamx, const float* dMn /*nullable*/, int64_t lddmn,
                                const int32_t* argmn /*nullable*/, int64_t ldamn, float* dB, int64_t lddb, ddmp_stream stream);

/* ------------------------------------------------------------------ per-channel softmax aggregation (GENConv / PyG's
 * SoftmaxAggregation) on the graph of the neighbour statistics above.  The message is m_j[c] = max(H[j,c], 0) +
 * msg_eps with has_eps != 0 (msg_eps >= 0), else m_j[c] = H[j,c]; it is formed in registers and never written.  t: any finite float.
 *
 * forward:   per row i and channel c, over the row's entries e (a_e their multiplicities):
 *            p_e = a_e exp(t m_e - mx) / sum_e a_e exp(t m_e - mx), mx = max_e t m_e;
 *            Y[i,c] = R[i,c] + sum_e p_e m_e;   lse[i,c] = mx + log sum_e a_e exp(t m_e - mx).
 *            Every neighbour row is loaded once per sweep (the row's first one a second time ahead of it, for the shift; an L1
 *            hit); the running maximum, denominator and numerator of a channel stay in registers over
 *            all entries and are rescaled once per batch of 8 entries.  The sums run over m_e - (the row's first message), so a
 *            column with a large offset keeps Y to float32 rounding.  R (nullable, [n, C]; it may be a column block of the buffer H
 *            is a block of): one unfused addition.  A row without entries gets R's row bit for bit (0 without R) and lse = 0.
 *            lse (nullable): not stored when null (a forward without a backward).  No output may alias H, R or the other output.
 *            The vector kernels need C and every leading dimension % 4 == 0 and 16-byte aligned matrices; anything else takes
 *            scalar kernels.  One launch. */
int ddmp_gather_softmax_f32(const ddmp_graph* g, const float* H, int64_t ldh, int C, float t, int has_eps, float msg_eps,
                            const float* R /*nullable*/, int64_t ldr, float* Y, int64_t ldy, float* lse /*nullable*/, int64_t ldl,
                            ddmp_stream stream);
/* backward, node side (symmetric structure, as ddmp_gather_stats_bwd_f32), with i = col e', w = a_{mirror e'},
 *            p = exp(t m_j[c] - lse[i,c]) and Yp = Y without the R term (the caller passes it):
 *            s[j,c] = sum_{e' in row j} w p dOut[i,c],   r[j,c] = sum_{e' in row j} w p dOut[i,c] (m_j[c] - Yp[i,c]),
 *            dH[j,c] = (s + t r) (has_eps: times [H[j,c] > 0]),   dR[j,:] = dOut[j,:] (nullable: the root block of the same gradient
 *            row buffer),   dt_rows[j] = sum_c m_j[c] r[j,c] (nullable, [n]: the temperature's gradient is its sum).
 *            add_dout != 0: dH[j,c] += dOut[j,c], one unfused addition after the mask (a layer whose root term is H itself).
 *            dH is written completely: a row without entries gets zeros (dOut's row with add_dout).  No output may alias an input
 *            or another output.  One launch. */
int ddmp_gather_softmax_bwd_f32(const ddmp_graph* g, int C, const float* dOut, int64_t lddo, const float* H, int64_t ldh,
                                const float* Yp, int64_t ldyp, const float* lse, int64_t ldl, float t, int has_eps, float msg_eps,
                                int add_dout, float* dH, int64_t lddh, float* dR /*nullable*/, int64_t lddr,
                                float* dt_rows /*nullable*/, ddmp_stream stream);

/* ------------------------------------------------------------------ crystal graph convolution (torch_geometric CGConv; DESIGN.md
 * 4.19): two per-channel gates on every input edge t: j -> i, each with a learned term in the edge's attributes a_t [dim]:
 *   F_t = Af[i,:] + Bf[j,:] + Ef a_t,   S_t = As[i,:] + Bs[j,:] + Es a_t,   f = sigmoid(F_t),   s = softplus(S_t).
 * float32.  Af, As, Bf, Bs: [n, C] with their own leading dimensions (column blocks of one row buffer).  dim in [0, 8].
 * dim > 0: the graph of ddmp_graph_create_valued(flags = 0) left at all-ones values (an entry's input edges are its ee span, in
 * input order: duplicate edges with different attributes are exact); attr: contiguous [input edges, dim] in the order of the edge
 * list the graph was created from; EfT, EsT: the edge weights TRANSPOSED, contiguous [dim, C].  dim == 0: any attention graph; attr,
 * EfT and EsT are null, an entry counts with its multiplicity and the ee tables are not read.  mean != 0: w_i = 1 / (the number
 * of input edges into i) (1 for a row without any), else w_i = 1.  Nothing is stored per edge: the backward launches recompute
 * both gates.  softplus keeps its relative accuracy for S -> -inf; no NaN and no Inf for any finite operand.  No output may alias an
 * input or another output.  The vector kernels need C and every leading dimension % 4 == 0 and 16-byte aligned operands; anything
 * else takes scalar kernels.  No atomics, fixed order: bitwise reproducible.
 *
 * forward:   Y[i,:] = root[i,:] + w_i sum_{t -> i} f (.) s  (root [n, C] nullable: zeros).  A row without entries gets root[i,:]
 *            bit for bit.  One launch. */
int ddmp_cgate_fwd_f32(const ddmp_graph* g, const float* Af, int64_t ldaf, const float* As, int64_t ldas, const float* Bf,
                       int64_t ldbf, const float* Bs, int64_t ldbs, int C, const float* attr /*null iff dim == 0*/, int dim,
                       const float* EfT /*null iff dim == 0*/, const float* EsT /*null iff dim == 0*/, const float* root /*nullable*/,
                       int64_t ldr, int mean, float* Y, int64_t ldy, ddmp_stream stream);
/* backward, row side, with dF_t = dOut[i,:] (.) s (.) f (1 - f) and dS_t = dOut[i,:] (.) f (.) sigmoid(S_t):
 *            dAf[i,:] = w_i sum_{t -> i} dF_t,   dAs[i,:] = w_i sum_{t -> i} dS_t  (written completely) and, dim > 0 and P non-null,
 *            the per-row partials P[i] = w_i [sum_t dF_t (x) a_t | sum_t dS_t (x) a_t], contiguous [n, 2, dim, C]: their column sum
 *            is [dEfT | dEsT].  One launch. */
int ddmp_cgate_bwd_row_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Af, int64_t ldaf, const float* As,
                           int64_t ldas, const float* Bf, int64_t ldbf, const float* Bs, int64_t ldbs, int C,
                           const float* attr /*null iff dim == 0*/, int dim, const float* EfT, const float* EsT, int mean, float* dAf,
                           int64_t lddaf, float* dAs, int64_t lddas, float* P /*nullable*/, ddmp_stream stream);
/* backward, node side (row j's own entries e' enumerate the targets i = col e' that j feeds -- the structure is symmetric -- and
 *            the edges j -> i, or their count, are those of the mirrored entry):
 *            dBf[j,:] = sum_{t: j -> i} w_i dF_t,   dBs[j,:] = sum_{t: j -> i} w_i dS_t  (written completely) and, dS non-null, the
 *            root block's gradient dS[j,:] = dOut[j,:].  One launch. */
int ddmp_cgate_bwd_node_f32(const ddmp_graph* g, const float* dOut, int64_t lddo, const float* Af, int64_t ldaf, const float* As,
                            int64_t ldas, const float* Bf, int64_t ldbf, const float* Bs, int64_t ldbs, int C,
                            const float* attr /*null iff dim == 0*/, int dim, const float* EfT, const float* EsT, int mean, float* dBf,
                            int64_t lddbf, float* dBs, int64_t lddbs, float* dS /*nullable*/, int64_t ldds, ddmp_stream stream);

/* ------------------------------------------------------------------ dense steps (MFMA; float32 operands and results, the
 * arithmetic is ddmp_set_gemm_mode's: by default SPLIT-precision 16-bit MFMA products with f32 accumulation -- f32-class
 * accuracy, not bit-exact f32; mode 0 = f32-input MFMA, the strict one)
 * Replace GCNConv.lin (X.W^T, no bias) and its autograd (dX = dH.W, dW = dH^T.X).
 *   nt : Y[n,M] = f(A[n,K]) . W[M,K]^T (+ bias[M])       forward / dgrad with a transposed table
 *   nn : Y[n,K] =   A[n,M]  . W[M,K]                     dgrad
 *   tn : dW[M,K] = G[n,M]^T . f(Z[n,K])                  wgrad, split over rows; needs workspace
 * f as in ddmp_spmm_f32 (per column of A resp. Z).  K, lda, ldz must be multiples of 4.
 */
size_t ddmp_gemm_rows_workspace_bytes(int K, int M);   /* optional scratch of nt / nn: W pre-split into bf16 planes */
int ddmp_gemm_nt_f32(const float* A, int64_t lda, const float* W, int64_t ldw, float* Y, int64_t ldy,
                     int64_t n_rows, int K, int M, const float* bias,
                     const float* pro_scale, const float* pro_shift, float slope,
                     void* workspace /*nullable*/, size_t workspace_bytes, ddmp_stream stream);
size_t ddmp_gemm_tn_workspace_bytes(int64_t n_rows, int M, int K);
/* GEMM arithmetic (process-wide; the environment variable DDMP_GEMM_MODE sets the initial value):
 *   6  = bf16x6 split MFMA: every f32 operand is split into three bf16 terms, six bf16 MFMA products accumulated in
 *        f32 -- f32-class accuracy at 2.67x the f32-MFMA rate;
 *   13 = (default) f16x3 in the row-panel kernels (the wide layers of big meshes), bf16x6 everywhere else: the
 *        operand, scaled by a power of two, is split into two _Float16 terms (22-23 bits) and three f16 MFMA products
 *        are accumulated in f32 (the "3xTF32" scheme; csrc/gemm_f16s.inc) -- f32-class accuracy, half the MFMA work;
 *   3  = bf16x3 (three products, ~2^-16 relative);   0 = f32-input MFMA (v_mfma_f32_32x32x2_f32).
 * Mode 13's power of two comes from the operand's absolute maximum, kept in a "scale slot" (device float[4]: {maximum
 * in use, maximum seen by the last kernels, overflow flag, healed events}).  By default the library measures it in a pre-pass over
 * the operand.  A training loop avoids that pass: DDMP_OPT_SCALES of the *_o forms names persistent slots for THAT call
 * (slot_a: the row operand A / dZ / G; slot_b: Z of the tn forms; prime != 0: measure now
 * anyway, e.g. first iteration), the GEMM kernels record the maximum they see, and ddmp_gemm_scales_roll, once per
 * iteration, makes it the next iteration's scale (6 bits of head-room).  An operand that still outgrows its scale raises
 * the slot's flag ([2]) and is HEALED inside the same ddmp_gemm_* call: the kernel is launched a second time, returns at
 * once while the flag is clear and otherwise redoes the product with the maximum the first launch has just recorded
 * ([1]), overwriting the clamped result before the caller's next kernel sees it.  ddmp_gemm_scales_roll counts healed
 * events per slot in [3] (-1: the operand was not finite) and clears the flag. */
int ddmp_set_gemm_mode(int mode);
int ddmp_get_gemm_mode(void);
int ddmp_gemm_scales_roll(float* slots, int n_slots, ddmp_stream stream);

/* ------------------------------------------------------------------ BatchNorm1d (train mode) + LeakyReLU
 * Replace nn.BatchNorm1d(C) in train mode + nn.LeakyReLU() (util/networks.py:31-44,51-62): batch
 * statistics over all n rows, biased variance, running stats with `momentum`.  Statistics are
 * float64 column sums (sum, sumsq) so that several devices can add theirs before `prepare`.
 * The normalise+activate is expressed as z = LeakyReLU(scale[c]*y + shift[c]) and is applied by the
 * CONSUMER kernels (pro_scale / pro_shift arguments); ddmp_bn_lrelu_apply_f32 materialises it.
 * Widths: C a power of two in [8, 1024].  Workspace: ddmp_colreduce_workspace_bytes(n_rows, C).
 */
size_t ddmp_colreduce_workspace_bytes(int64_t n_rows, int C);
int ddmp_bn_stats_f32(const float* Y, int64_t ldy, int64_t n_rows, int C, double* sums /*[2C]*/,
                      void* workspace, size_t workspace_bytes, ddmp_stream stream);
int ddmp_bn_prepare_f32(const double* sums /*[2C]*/, double n_total, int C, const float* gamma,
                        const float* beta, float eps, float momentum, float* scale, float* shift,
                        float* mean, float* rstd, float* running_mean /*nullable*/,
                        float* running_var /*nullable*/, ddmp_stream stream);
int ddmp_bn_lrelu_apply_f32(const float* Y, int64_t ldy, float* Z, int64_t ldz, int64_t n_rows, int C,
                            const float* scale, const float* shift, float slope, ddmp_stream stream);
/* backward reductions sums2 = (sum g, sum g*yhat), g = dZ * LeakyReLU'(scale*y+shift), yhat = (y-mean)*rstd: ddmp_bn_bwd_reduce
 * (dtype-tagged, below) */
/* sums2 -> dgamma, dbeta and the two folded constants of dY = scale*g + c1*y + c0 */
int ddmp_bn_bwd_prepare_f32(const double* sums2, double n_total, int C, const float* scale, const float* mean,
                            const float* rstd, float* dgamma, float* dbeta, float* c1, float* c0,
                            ddmp_stream stream);
/* Tail-fused coefficients (round 3) and the other per-call options are arguments of the *_o entry points at the end of this header
 * (ABI 3).  ddmp_next_pending is the ABI's diagnostic for options "still recorded for this host thread": options travel with their
 * own call as arguments and are recorded nowhere, so it returns 0, always. */
int ddmp_next_pending(void);
/* dY (gradient w.r.t. the conv output) and its column sums (= gradient of the conv bias; dbias_sums NULL: dY only -- behind
 * a BatchNorm those sums are zero in exact arithmetic) */
int ddmp_colsum_f32(const float* X, int64_t ldx, int64_t n_rows, int C, double* sums /*[C]*/, void* workspace,
                    size_t workspace_bytes, ddmp_stream stream);
int ddmp_f64_to_f32(const double* in, float* out, int64_t n, ddmp_stream stream);

/* ------------------------------------------------------------------ output heads
 * Replace linear1 -> LeakyReLU -> linear2 (+ residual | tanh + row normalise), util/networks.py:64-67
 * (kind 0, PosNet: out = x_pos + u) and :125-129 (kind 1, NormalNet: out = tanh(u)/(|tanh(u)|+1e-12)).
 * Y is the conv12 output [n,32]; its BatchNorm+LeakyReLU is the scale/shift prologue.  W1 [16,32],
 * b1 [16], W2 [3,16], b2 [3]; out / dout [n,3] contiguous.  Backward writes dZ [n,32] (gradient w.r.t.
 * the activated conv12 features) and overwrites the four parameter gradients.
 */
size_t ddmp_head_bwd_workspace_bytes(int64_t n_rows);

/* ------------------------------------------------------------------ losses (util/loss.py)
 * Index tables are int32 device arrays: faces [F,3], f2f [F,3] (-1 padded, symmetric on valid entries),
 * vv_ptr/vv_idx = 1-ring CSR without self (util/mesh.py:189-197), vf_ptr/vf_corner = vertex -> incident
 * (3*face + corner).  Targets are float64 as in the reference (n_mesh.vs / n_mesh.fn are f64 numpy).
 * `partials` (ddmp_loss_partials_bytes()) collects per-block float64 sums of S1..S5 and sigma_c;
 * ddmp_loss_finalize turns them into
 *   lossbuf[0..4] = pos_rec (:16), laplacian (:37), norm_rec (:55), fn_bnf (:86, ungated), pos_norm (:140)
 *   lossbuf[5]    = k1*L1 + k2*L2 + k3*L3 + k4*gate4*L4 + k5*L5        (main.py:101-106)
 *   lossbuf[6..10]= gradient coefficients c1..c5 consumed by the *_bwd calls, lossbuf[11] = sigma_c.
 * The *_bwd calls take `coef` = device double[5] (c1..c5); a zero coefficient switches a term off.
 */
size_t ddmp_loss_partials_bytes(void);
int ddmp_loss_vertex_fwd(int64_t V, const float* pos, const double* real_pos, const int32_t* vv_ptr,
                         const int32_t* vv_idx, float* resid /*[V,3]*/, double* partials, ddmp_stream stream);
int ddmp_loss_face_fwd(int64_t F, const float* pos, const float* norm, const double* real_norm,
                       const int32_t* faces, float* fc /*[F,3]*/, float* fa /*[F]*/, float* pn_coef /*[F,3]*/,
                       float* pn_dn /*[F,3]*/, double* partials, ddmp_stream stream);
int ddmp_loss_bnf_fwd(int64_t F, const float* norm, const int32_t* f2f, const float* fc, const float* fa,
                      int loop, float* fcd /*[F,3]*/, float* bnf_n /*[loop+1,F,3]*/, float* bnf_A /*[loop,F,3]*/,
                      double* partials, ddmp_stream stream);
int ddmp_loss_finalize(const double* partials, int64_t V, int64_t F, const double* k_host /*[5]*/, double gate4,
                       double* lossbuf /*[12]*/, ddmp_stream stream);
int ddmp_loss_bnf_bwd(int64_t F, const int32_t* f2f, const float* fa, const float* fcd, int loop,
                      const float* bnf_n, const float* bnf_A, const double* partials, const double* coef,
                      float* G0 /*[F,3]*/, float* scratch /*[2,F,3]*/, ddmp_stream stream);
int ddmp_loss_face_bwd(int64_t F, const float* norm, const double* real_norm, const float* pn_dn,
                       const float* G0 /*nullable*/, const float* n_last /*with G0*/, const double* coef,
                       float* dnorm /*[F,3]*/, ddmp_stream stream);
int ddmp_loss_vertex_bwd(int64_t V, const float* pos, const double* real_pos, const float* resid,
                         const int32_t* vv_ptr, const int32_t* vv_idx, const int32_t* vf_ptr,
                         const int32_t* vf_corner, const float* pn_coef, const float* norm, const double* coef,
                         float* dpos /*[V,3]*/, ddmp_stream stream);

/* Sharded form of the same losses (one rank of a partitioned mesh).  The rank runs the kernels above on its
 * LOCAL sub-mesh = owned vertices / faces plus a ghost closure deep enough that every value an owned row's loss term or
 * gradient reads is computed locally (dist.LossShard: 2*loop+1 face rings, 2 vertex rings, the mesh's last face for the
 * "-1" slots): no exchange inside the losses.  What differs from the single-device calls:
 *   - `own` (uint8 per local row, nullable = all): partial sums count owned rows only; ghost rows are computed, not counted;
 *   - the caller all-reduces the partial sums across ranks -- the sigma_c slice between ddmp_loss_bnf_sigma and
 *     ddmp_loss_bnf_filter, the S1..S5 slices before ddmp_loss_finalize (which takes the GLOBAL V, F);
 *   - F_glob: sigma_c = sum / (3 F_glob) is a mean over all faces of the mesh; the local F still addresses the local
 *     "last face" (the caller places the mesh's last face at the end of its local numbering).
 * partials layout: 6 slices of ddmp_loss_partials_bytes() / 48 doubles: S1..S5, sigma_c. */
int ddmp_loss_vertex_fwd_part(int64_t V, const float* pos, const double* real_pos, const int32_t* vv_ptr,
                              const int32_t* vv_idx, float* resid, double* partials, const uint8_t* own, ddmp_stream stream);
int ddmp_loss_face_fwd_part(int64_t F, const float* pos, const float* norm, const double* real_norm, const int32_t* faces,
                            float* fc, float* fa, float* pn_coef, float* pn_dn, double* partials, const uint8_t* own,
                            ddmp_stream stream);
int ddmp_loss_bnf_sigma(int64_t F, const float* norm, const int32_t* f2f, const float* fc, float* fcd, float* bnf_n,
                        double* partials, const uint8_t* own, ddmp_stream stream);
int ddmp_loss_bnf_filter(int64_t F, int64_t F_glob, const int32_t* f2f, const float* fcd, const float* fa, int loop,
                         float* bnf_n, float* bnf_A, double* partials, const uint8_t* own, ddmp_stream stream);
int ddmp_loss_bnf_bwd_part(int64_t F, int64_t F_glob, const int32_t* f2f, const float* fa, const float* fcd, int loop,
                           const float* bnf_n, const float* bnf_A, const double* partials, const double* coef, float* G0,
                           float* scratch, ddmp_stream stream);

/* ------------------------------------------------------------------ clip_grad_norm_ + Adam (main.py:108-110)
 * One flat float32 arena per net for param / grad / exp_avg / exp_avg_sq.  clip: coefficient
 * min(1, max_norm / (sqrt(sumsq) + 1e-6)) (torch.nn.utils.clip_grad_norm_); Adam: torch defaults
 * (no weight decay, no amsgrad), `step` is 1-based.  Passing clip_sumsq to ddmp_adam_step_f32 applies
 * the clip on the fly (grad buffer left unscaled); ddmp_grad_clip_f32 scales it in place instead.
 */
size_t ddmp_sumsq_workspace_bytes(void);
int ddmp_grad_sumsq_f32(const float* g, int64_t n, double* out /*[1]*/, void* workspace, size_t workspace_bytes,
                        ddmp_stream stream);
int ddmp_grad_clip_f32(float* g, int64_t n, const double* sumsq, float max_norm, ddmp_stream stream);
int ddmp_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                       float beta2, float eps, int step, const double* clip_sumsq /*nullable*/, float max_norm,
                       ddmp_stream stream);
/* ddmp_spmm_bnred (dtype-tagged, below; + ddmp_spmm_bnred_ws_bytes): the aggregation (no bias, no prologue) whose output Y is a
 * gradient dZ consumed next by a BatchNorm+LeakyReLU backward also returns that layer's column reductions sums2 =
 * ddmp_bn_bwd_reduce(Y, Yp, scale, shift, mean, rstd) from the kernel's epilogue (float32 partials per 64-row chunk, summed in
 * float64); other widths run the two calls one after the other. */
/* GCNConv.propagate of a transform-first layer (forward) that also returns the BatchNorm statistics of its output
 * (float64 [2C]: column sums of Y and of Y^2 = ddmp_bn_stats_f32(Y)) from the gather kernel's epilogue (round 3).  `ref`
 * [C]: a per-column reference near the column means (the caller's previous batch means; zeros are valid): the kernel
 * sums (y - ref) and (y - ref)^2 in float32 over 16 rows at a time and in float64 from there on, and the shift is undone
 * exactly -- around ref those partial sums are well conditioned whatever mean / std is (float32-class statistics, as
 * nn.BatchNorm1d computes them).  Workspace: ddmp_spmm_bnred_ws_bytes(n_rows, C, DDMP_F32).  Where the fused kernel does not
 * apply (C % 32, misaligned, ref NULL) it runs ddmp_spmm_f32 + the column reduction of ddmp_bn_stats_f32, at any width, leading
 * dimension and alignment (a scalar first stage where that entry point's own kernel does not apply); ddmp_spmm_bnred likewise. */
int ddmp_spmm_stats_supported(int C);
int ddmp_spmm_stats_f32(const ddmp_graph* g, const float* X, int64_t ldx, float* Y, int64_t ldy, int C,
                        const float* bias /*nullable*/, const float* pro_scale /*nullable*/,
                        const float* pro_shift /*nullable*/, float slope, const float* ref /*[C], nullable*/,
                        double* sums2 /*[2C]*/, void* workspace, size_t workspace_bytes, ddmp_stream stream);
/* dtype-tagged form; workspace >= max(ddmp_spmm_bnred_ws_bytes, ddmp_colreduce_workspace_bytes) */
int ddmp_spmm_stats(const ddmp_graph* g, const void* X, int64_t ldx, void* Y, int64_t ldy, int C, int dtype,
                    const float* bias, const float* pro_scale, const float* pro_shift, float slope, const float* ref,
                    double* sums2, void* workspace, size_t workspace_bytes, ddmp_stream stream);
/* backward of GCNConv.propagate of a transform-first layer, with the backward of the BatchNorm1d+LeakyReLU behind it
 * (util/networks.py:51-62 under autograd) rebuilt on the gather: out = A_hat . dY,
 * dY = a * dZ * lrelu'(a * Yb + b) + c1 * Yb + c0 per column (what ddmp_bn_bwd_apply_f32 would have written and this
 * kernel read back).  C % 32 == 0 (ddmp_spmm_bnbwd_supported). */
int ddmp_spmm_bnbwd_supported(int C);
int ddmp_spmm_bnbwd_f32(const ddmp_graph* g, const float* dZ, int64_t lddz, const float* Yb, int64_t ldyb,
                        float* out, int64_t ld_out, int C, const float* a, const float* b, const float* c1,
                        const float* c0, float slope, ddmp_stream stream);


/* ddmp_gemm_nt_f32 that also returns the BatchNorm statistics of its output (float64 [2M]: column sums of Y and of
 * Y^2 over the n_rows rows = what ddmp_bn_stats_f32(Y) returns; GCNConv -> BatchNorm1d, util/networks.py:52-53).  The
 * row-panel kernel produces them in its epilogue (float64 partials per 64 rows); other shapes run
 * the GEMM followed by ddmp_bn_stats_f32. */
size_t ddmp_gemm_nt_stats_workspace_bytes(int64_t n_rows, int M);
int ddmp_gemm_nt_stats_f32(const float* A, int64_t lda, const float* W, int64_t ldw, float* Y, int64_t ldy,
                           int64_t n_rows, int K, int M, const float* bias /*nullable*/,
                           const float* pro_scale /*nullable*/, const float* pro_shift /*nullable*/, float slope,
                           double* sums2 /*[2M]*/, void* workspace, size_t workspace_bytes, void* stats_ws,
                           size_t stats_ws_bytes, ddmp_stream stream);

/* BatchNorm+LeakyReLU backward fused into the operand load of the GEMMs that consume dY (agg-first layers of the
 * engine; replaces ddmp_bn_bwd_apply_f32 + ddmp_gemm_nn_f32 + ddmp_gemm_tn_f32 of util/networks.py's autograd chain):
 *     dY = a * dZ * lrelu'(a * Yb + b) + c1 * Yb + c0        (a, b, c1, c0 per column, from ddmp_bn_bwd_prepare_f32)
 * ddmp_gemm_bnbwd_supported(cout, cin, n_rows) says whether BOTH fused GEMMs exist for a layer of that shape and row
 * count in the current GEMM mode (the panel kernels they live in are used from ~30k rows); the conv-bias gradient (column sums of dY) is exactly zero in exact arithmetic and is written as 0. */
/* dgrad of a transform-first layer with the NEXT BatchNorm-backward column reductions from its epilogue (round 3, row-register
 * kernel): out[n,K] = A[n,M] . W[M,K] and sums2[2K] = what ddmp_bn_bwd_reduce_f32(out, Yp, scale, shift, mean, rstd) returns,
 * Yp [n,K] = the previous layer's conv output; stats_ws >= ddmp_gemm_nt_stats_workspace_bytes(n_rows, K) */
/* Weights prepared once per iteration (round 3).  Every ddmp_gemm_nt* / ddmp_gemm_nn* call splits its weight matrix into
 * 16-bit planes in its workspace before the product (absolute maximum + split: 2-3 launches per call).
 * ddmp_gemm_prepare_weights does that for n <= 24 matrices in two launches, into caller-owned buffers planes[i] (>=
 * ddmp_gemm_rows_workspace_bytes(K[i], M[i]) bytes, 16-byte aligned), in the layout the product over n_rows rows will want:
 * W[i] is [M[i], K[i]] float32 with leading dimension ldw[i]; form[i] 0 = forward (ddmp_gemm_nt*: Y[n,M] = f(A[n,K]) . W^T,
 * has_pro[i] = with a prologue), 1 = dgrad (ddmp_gemm_nn*: Y[n,K] = A[n,M] . W).  scratch: 8 n floats.
 * A GEMM call then passes planes[i] as its `workspace` and says so with DDMP_OPT_PREPARED (the *_o entry points below): it
 * skips its own split if the buffer was prepared for exactly this matrix, shape and route, and splits as before otherwise.
 * The caller re-prepares whenever the weights change. */
int ddmp_gemm_prepare_weights(int n, const float* const* W, const int64_t* ldw, const int* M, const int* K, const int* form,
                              const int* has_pro /*nullable*/, void* const* planes, const size_t* planes_bytes,
                              int64_t n_rows, float* scratch, ddmp_stream stream);
/* the owner of a plane buffer is about to free it: drop what this thread recorded for it (NULL: everything) */
int ddmp_gemm_forget_planes(const void* planes);
int ddmp_gemm_tn_bnbwd_supported(int cout, int cin, int64_t n_rows);   /* the fused wgrad alone (a first layer has no dgrad) */
int ddmp_gemm_nn_bnred_supported(int M, int K, int64_t n_rows);
int ddmp_gemm_nn_bnred_f32(const float* A, int64_t lda, const float* W, int64_t ldw, float* out, int64_t ld_out,
                           int64_t n_rows, int M, int K, const float* Yp, int64_t ldyp, const float* scale,
                           const float* shift, const float* mean, const float* rstd, float slope, double* sums2,
                           void* workspace, size_t workspace_bytes, void* stats_ws, size_t stats_ws_bytes,
                           ddmp_stream stream);
int ddmp_gemm_bnbwd_supported(int cout, int cin, int64_t n_rows);
int ddmp_gemm_nn_bnbwd_f32(const float* dZ, int64_t lddz, const float* Yb, int64_t ldyb, const float* W, int64_t ldw,
                           float* out, int64_t ld_out, int64_t n_rows, int M, int K, const float* a, const float* b,
                           const float* c1, const float* c0, float slope, void* workspace, size_t workspace_bytes,
                           ddmp_stream stream);
int ddmp_gemm_tn_bnbwd_f32(const float* dZ, int64_t lddz, const float* Yb, int64_t ldyb, const float* Z, int64_t ldz,
                           float* dW, int64_t lddw, int64_t n_rows, int M, int K, const float* a, const float* b,
                           const float* c1, const float* c0, const float* pro_scale /*nullable*/,
                           const float* pro_shift /*nullable*/, float slope, void* workspace, size_t workspace_bytes,
                           ddmp_stream stream);
/* For tests that name a route (host only, nothing is launched; the current GEMM mode and the DDMP_* switches apply).
 * ddmp_gemm_row_route: the kernel family of a row product Y[n, MD] = f(A[n, KD]) . B with a fitting workspace -- 1 f16x3 row panel,
 *   2 bf16 row panel, 3 tiled, 4 presplit, 5 plain -- + 256 where the row-register kernel runs the f16x3 family.  lda2 > 0: the
 *   (dZ, Yb) operand pair of ddmp_gemm_nn_bnbwd_f32 (0 otherwise); y_misaligned != 0: Y is not on 16 bytes.
 * ddmp_gemm_tn_route: the wgrad kernel -- 1 f16x3 row-major, 2 bf16 panel, 3 bf16 tiled, 4 f32 tiled -- for operands of small
 *   leading dimensions; ld_ok: every leading dimension a multiple of 4 and every base on 16 bytes; dual: the _bnbwd form;
 *   plan4: T (1 | 2 tiles of 64 T, 4 = panels), tm, tk (panel edges, 0 for tiles), n_splits */
int ddmp_gemm_row_route(int64_t n_rows, int KD, int MD, int has_pro, int64_t lda, int64_t lda2, int64_t ldy, int y_misaligned);
int ddmp_gemm_tn_route(int64_t n_rows, int M, int K, int dual, int ld_ok, int* plan4 /*[4], nullable*/);

/* graph-replay form: the step count lives on the device.  ddmp_adam_prepare does ++(*step_counter) and writes
 * coef = { lr / (1 - beta1^t), sqrt(1 - beta2^t) }; ddmp_adam_step_dev_f32 reads coef instead of host values. */
int ddmp_adam_prepare(int32_t* step_counter, float lr, float beta1, float beta2, float* coef /*[2]*/,
                      ddmp_stream stream);
int ddmp_adam_step_dev_f32(float* p, const float* g, float* m, float* v, int64_t n, float beta1, float beta2,
                           float eps, const float* coef /*[2]*/, const double* clip_sumsq /*nullable*/,
                           float max_norm, ddmp_stream stream);

/* ------------------------------------------------------------------ evaluation block (main.py:117-123)
 * Face normals of predicted positions (util/mesh.py:87-92; float32 like the reference's float32 `new_pos`)
 * and MAD = mean over faces of deg(arccos(clip(n1.n2, -1, 1))) in float64 (util/loss.py:261-272).
 */
int ddmp_face_normals_f32(int64_t F, const float* pos, const int32_t* faces, float* fn /*[F,3]*/,
                          float* fa /*[F] nullable*/, ddmp_stream stream);
/* vertex update from predicted normals (util/models.py:31-44): `loop` sweeps of
 * p_v += mean_{f in F(v)} ((c_f - p_v).n_f) n_f, in place; fc_scratch [F,3] (holds (c_f - p_fk).n_f per corner, formed
 * from edge vectors so that the result does not depend on where the mesh sits) */
int ddmp_vertex_update_f32(int64_t V, int64_t F, float* pos, const float* norm, const int32_t* faces,
                           const int32_t* vf_ptr, const int32_t* vf_corner, float* fc_scratch, int loop,
                           ddmp_stream stream);
/* the same with the positions kept as a float32 pair pos + lo_scratch [V,3] between sweeps (lo_scratch is zeroed here and
 * holds the rounding remainder afterwards; `pos` is the pair's sum rounded once): several sweeps of a mesh whose coordinates
 * are much larger than its edges stay within 1e-7 of an edge of float64, where one float32 per coordinate loses an ulp of
 * the coordinate per sweep */
int ddmp_vertex_update_pair_f32(int64_t V, int64_t F, float* pos, const float* norm, const int32_t* faces,
                                const int32_t* vf_ptr, const int32_t* vf_corner, float* corner_scratch /*[F,3]*/,
                                float* lo_scratch /*[V,3]*/, int loop, ddmp_stream stream);
size_t ddmp_mad_workspace_bytes(void);
int ddmp_mad_f64(int64_t F, const float* n1 /*[F,3] f32*/, const double* n2 /*[F,3] f64*/, double* out /*[1]*/,
                 void* workspace, size_t workspace_bytes, ddmp_stream stream);

/* ------------------------------------------------------------------ point-to-surface distance (check/hausdorff_checker.py)
 * A uniform grid over the triangles of a target mesh, built on the device, and the exact distance from query points to
 * that surface (closest point by Voronoi region, f32).  The grid is one caller-owned buffer:
 *   ddmp_surfdist_grid_bytes(F, max_refs): bytes for F faces and up to max_refs cell references (0 on bad sizes);
 *   ddmp_surfdist_build: packs the triangles, sizes the cells (about the mean edge length, grown until the cell count is
 *     at most 4F), lists every face in every cell its bounding box overlaps.  SYNCHRONISES the stream once, to read the
 *     reference count: DDMP_EWORKSPACE when it exceeds the buffer (*refs_needed_host then says how many are needed),
 *     DDMP_ERANGE for a face index outside [0, V), DDMP_EINVAL for a non-finite coordinate of a face's vertex or an extent
 *     beyond the float32 range (no grid is built then).  Nothing is written past grid_bytes.
 *   ddmp_surfdist_query: one distance per point, stats[12] (f64) = count, sum, sum of squares, min, max of the kept
 *     distances, number dropped, bbox min xyz and bbox max xyz of the points.  max_dist > 0: points farther than max_dist
 *     from the surface are dropped (dist = +inf); 0 keeps all.  sort_queries = 1 orders the points by grid cell first
 *     (same results).  dist may be null (the workspace holds them).  A non-finite point gets dist = NaN and makes the
 *     sum NaN (it is not dropped).  Deterministic: no float atomics. */
size_t ddmp_surfdist_grid_bytes(int64_t F, int64_t max_refs);
int ddmp_surfdist_build(int64_t V, int64_t F, const float* pos /*[V,3]*/, const int32_t* faces /*[F,3]*/, void* grid,
                        size_t grid_bytes, int64_t* refs_needed_host /*nullable*/, ddmp_stream stream);
size_t ddmp_surfdist_query_workspace_bytes(int64_t Q, int64_t F);
int ddmp_surfdist_query(int64_t F, const void* grid, size_t grid_bytes, int64_t Q, const float* points /*[Q,3]*/,
                        float max_dist, int sort_queries, float* dist /*[Q] nullable*/, double* stats /*[12]*/,
                        void* workspace, size_t workspace_bytes, ddmp_stream stream);

/* ------------------------------------------------------------------ bfloat16-feature mode (SURVEY.md §8b `dtype`)
 * BASELINE.json configs[1] ("bf16 features"): node features, saved activations and activation gradients [N, C] are
 * bfloat16 in HBM (raw uint16_t bits here; rows 16-byte aligned: C and every leading dimension a multiple of 8);
 * kernels unpack to float32, accumulate in float32 (BatchNorm statistics in float64) and round to nearest-even once on
 * the store.  Parameters, parameter gradients, optimizer state, coefficients (bias, scale, shift, c1, c0 ...) and the
 * [n,3] outputs / loss gradients stay float32.  The GEMMs run ONE v_mfma_f32_32x32x16_bf16 product per step (the float32
 * weights are converted to bf16 planes per call: workspace), no operand splitting and no scale slots.
 * Each *_bf16 entry point mirrors its *_f32 namesake argument for argument; the dtype-tagged forms
 * ddmp_spmm / ddmp_gemm_nt / ... below take `void*` features and dispatch on `dtype`.
 */
#define DDMP_F32 0
#define DDMP_BF16 1

/* bfloat16 features, plain GEMMs: through the dtype-tagged ddmp_gemm_nt / _nn / _tn below (nt / nn: K resp. M -- the contraction -- a
 * multiple of 32, nt also K = 8 | 16: the first layer; outputs <= 512 columns; workspace >= ddmp_gemm_rows_ws_bytes(K, M, DDMP_BF16)
 * holds the bf16 weight planes) */
/* Fused forms on the row-register kernel (csrc/gemm_rr_b16.inc; round 3): the streaming BatchNorm passes of the bf16 step
 * folded into the GEMMs, as the *_f32 namesakes do for float32 features.
 *   ddmp_gemm_fused_bf16_supported  bit 0: ddmp_gemm_nt_stats_bf16, bit 1: the two *_bnbwd_bf16 forms exist AND pay for a
 *                                   layer cin -> cout over n_rows rows (measured thresholds, csrc/gemm_b16.hip)
 *   ddmp_gemm_nt_stats_bf16         ddmp_gemm_nt_bf16 + sums2[2M] (float64) = column sums of Y and Y^2 as STORED (bf16),
 *                                   i.e. ddmp_bn_stats_bf16(Y), from the epilogue; stats_ws >= ..._stats_bf16_workspace_bytes
 *   ddmp_gemm_nn_bnbwd_bf16         out[n,K] = dY . W[M,K], dY = bf16(a dZ lrelu'(a Yb + b) + c1 Yb + c0) rebuilt on the operand
 *                                   load: what ddmp_bn_bwd_apply_bf16 would have written, never stored
 *   ddmp_gemm_tn_bnbwd_bf16         dW[M,K] = dY^T . f(Z), the same dY (reference op: GCNConv.lin backward behind
 *                                   BatchNorm1d + LeakyReLU, util/networks.py:31-44,51-62)
 *   (round 5's ddmp_gemm_nn_bnred_bf16 -- measured no gain inside the step -- left the library in round 6: experiments/r05/) */
int ddmp_gemm_fused_bf16_supported(int cout, int cin, int64_t n_rows);
size_t ddmp_gemm_nt_stats_bf16_workspace_bytes(int64_t n_rows, int M);
int ddmp_gemm_nt_stats_bf16(const uint16_t* A, int64_t lda, const float* W, int64_t ldw, uint16_t* Y, int64_t ldy,
                            int64_t n_rows, int K, int M, const float* bias, const float* pro_scale,
                            const float* pro_shift, float slope, double* sums2, void* workspace, size_t workspace_bytes,
                            void* stats_ws, size_t stats_ws_bytes, ddmp_stream stream);
int ddmp_gemm_nn_bnbwd_bf16(const uint16_t* dZ, int64_t lddz, const uint16_t* Yb, int64_t ldyb, const float* W,
                            int64_t ldw, uint16_t* out, int64_t ld_out, int64_t n_rows, int M, int K, const float* a,
                            const float* b, const float* c1, const float* c0, float slope, void* workspace,
                            size_t workspace_bytes, ddmp_stream stream);
int ddmp_gemm_tn_bnbwd_bf16(const uint16_t* dZ, int64_t lddz, const uint16_t* Yb, int64_t ldyb, const uint16_t* Z,
                            int64_t ldz, float* dW, int64_t lddw, int64_t n_rows, int M, int K, const float* a,
                            const float* b, const float* c1, const float* c0, const float* pro_scale,
                            const float* pro_shift, float slope, void* workspace, size_t workspace_bytes,
                            ddmp_stream stream);
/* BatchNorm passes: C a power of two in [16, 1024]; workspace = ddmp_colreduce_workspace_bytes(n_rows, C) */
int ddmp_bn_stats_bf16(const uint16_t* Y, int64_t ldy, int64_t n_rows, int C, double* sums /*[2C]*/, void* workspace,
                       size_t workspace_bytes, ddmp_stream stream);
int ddmp_bn_lrelu_apply_bf16(const uint16_t* Y, int64_t ldy, uint16_t* Z, int64_t ldz, int64_t n_rows, int C,
                             const float* scale, const float* shift, float slope, ddmp_stream stream);
int ddmp_bn_bwd_reduce_bf16(const uint16_t* dZ, int64_t lddz, const uint16_t* Y, int64_t ldy, int64_t n_rows, int C,
                            const float* scale, const float* shift, const float* mean, const float* rstd, float slope,
                            double* sums2 /*[2C]*/, void* workspace, size_t workspace_bytes, ddmp_stream stream);
int ddmp_bn_bwd_apply_bf16(const uint16_t* dZ, int64_t lddz, const uint16_t* Y, int64_t ldy, uint16_t* dY, int64_t lddy,
                           int64_t n_rows, int C, const float* scale, const float* shift, const float* c1,
                           const float* c0, float slope, double* dbias_sums /*[C]*/, void* workspace,
                           size_t workspace_bytes, ddmp_stream stream);
/* Multi-device halo packing (the reference is single-device, main.py:51): dst[r,:] = src[idx[r],:]
 * (scatter = 0: the boundary rows a rank sends, in the order of its halo plan) or dst[idx[r],:] = src[r,:] (scatter = 1);
 * idx int64 on the device; rows of C elements with C * element size a multiple of 16 bytes. */
int ddmp_rows_gather(const void* src, int64_t ld_src, const int64_t* idx, int64_t n, int C, int dtype, void* dst,
                     int64_t ld_dst, int scatter, ddmp_stream stream);
/* Communicator + halo plan + exchange on the caller's stream (csrc/comm.hip): one process per GPU, RCCL over xGMI.
 *   ddmp_comm_unique_id    rank 0 draws the 128-byte id, the host side distributes it (any out-of-band channel)
 *   ddmp_comm_create       ncclCommInitRank; status 1000 + ncclResult_t on RCCL errors
 *   ddmp_halo_plan_create  send_idx_host [sum send_counts]: LOCAL owned row of every boundary row, grouped by destination
 *                          rank in the order the receiver stores its halo; recv_counts per source rank (sum = n_cols - n_rows)
 *   ddmp_halo_exchange     rows [0, n_rows) of T are owned, rows [n_rows, n_cols) the halo (grouped by source rank): packs the
 *                          boundary rows (kernel), then ONE ncclGroup of send/recv pairs that lands the halo rows in place
 *                          (ld == C) and, when sums != NULL, the all-reduce of `n_sums` float64 BatchNorm column sums
 *   ddmp_comm_allreduce_sum / ddmp_comm_allgather   gradient arena, loss inputs */
typedef struct ddmp_comm ddmp_comm;
typedef struct ddmp_halo_plan ddmp_halo_plan;
int ddmp_comm_unique_id(char* id128_host);
int ddmp_comm_create(int rank, int world, const char* id128_host, ddmp_comm** out);
int ddmp_comm_destroy(ddmp_comm* comm);
int ddmp_halo_plan_create(int world, int rank, int64_t n_rows, int64_t n_cols, const int64_t* send_idx_host,
                          const int64_t* send_counts_host, const int64_t* recv_counts_host, ddmp_halo_plan** out);
int ddmp_halo_plan_destroy(ddmp_halo_plan* plan);
size_t ddmp_halo_pack_bytes(const ddmp_halo_plan* plan, int C, int dtype);
int ddmp_halo_exchange(ddmp_comm* comm, const ddmp_halo_plan* plan, void* T, int64_t ld, int C, int dtype, void* pack_ws,
                       size_t ws_bytes, double* sums /*nullable*/, int n_sums, ddmp_stream stream);
int ddmp_comm_allreduce_sum(ddmp_comm* comm, void* buf, int64_t n, int is_f64, ddmp_stream stream);
int ddmp_comm_allgather(ddmp_comm* comm, const void* send, void* recv, int64_t bytes_per_rank, ddmp_stream stream);
/* a one-thread kernel named ddmp_trace_marker_kernel: brackets a region in a rocprofv3 kernel trace (measurement aid) */
int ddmp_trace_marker(ddmp_stream stream);
/* 0 for the product library; a bit mask of the timing-only ablation macros a diagnostic build was compiled with (such builds
 * compute WRONG results: scripts/build_ablation*.sh).  The Python host side refuses a non-zero library unless it was named
 * explicitly through DDMP_LIB. */
int ddmp_build_ablation_flags(void);
/* measurement aid (bench.py's copy yardstick): a streaming device copy of `bytes` (multiple of 16, both pointers 16-byte
 * aligned) written like the library's HBM-bound kernels; mode 0 plain, 1 nontemporal loads / stores */
int ddmp_copy_probe(const void* src, void* dst, int64_t bytes, int mode, ddmp_stream stream);
/* ... and the same copy in the gather's access pattern: 64-row chunks of a row-major [n_rows, row_bytes] matrix walked one
 * 128-byte slab at a time (row_bytes a multiple of 128): the ceiling of that pattern, whatever the graph */
int ddmp_copy_probe_rows(const void* src, void* dst, int64_t n_rows, int row_bytes, ddmp_stream stream);
/* float32 -> bfloat16 (round to nearest even) of n contiguous elements */
int ddmp_f32_to_bf16(const float* in, uint16_t* out, int64_t n, ddmp_stream stream);

/* dtype-tagged forms (dtype = DDMP_F32 | DDMP_BF16): what a binding of the reference's GCNConv / BatchNorm1d / Linear
 * call sites (util/networks.py:15-26,31-44,51-67) uses when the feature dtype is a run-time choice */
int ddmp_spmm(const ddmp_graph* g, const void* X, int64_t ldx, void* Y, int64_t ldy, int C, int dtype, const float* bias,
              const float* pro_scale, const float* pro_shift, float slope, ddmp_stream stream);
size_t ddmp_spmm_bnred_ws_bytes(int64_t n_rows, int C, int dtype);
int ddmp_spmm_bnred(const ddmp_graph* g, const void* X, int64_t ldx, void* Y, int64_t ldy, int C, int dtype,
                    const void* Yp, int64_t ldyp, const float* scale, const float* shift, const float* mean,
                    const float* rstd, float slope, double* sums2, void* workspace, size_t workspace_bytes,
                    ddmp_stream stream);
int ddmp_spmm_bnbwd(const ddmp_graph* g, const void* dZ, int64_t lddz, const void* Yb, int64_t ldyb, void* out,
                    int64_t ld_out, int C, int dtype, const float* a, const float* b, const float* c1, const float* c0,
                    float slope, ddmp_stream stream);
size_t ddmp_gemm_rows_ws_bytes(int K, int M, int dtype);
int ddmp_gemm_nt(const void* A, int64_t lda, const float* W, int64_t ldw, void* Y, int64_t ldy, int64_t n_rows, int K,
                 int M, int dtype, const float* bias, const float* pro_scale, const float* pro_shift, float slope,
                 void* workspace, size_t workspace_bytes, ddmp_stream stream);
int ddmp_gemm_nn(const void* A, int64_t lda, const float* W, int64_t ldw, void* Y, int64_t ldy, int64_t n_rows, int M,
                 int K, int dtype, void* workspace, size_t workspace_bytes, ddmp_stream stream);
size_t ddmp_gemm_tn_ws_bytes(int64_t n_rows, int M, int K, int dtype);
int ddmp_gemm_tn(const void* G, int64_t ldg, const void* Z, int64_t ldz, float* dW, int64_t lddw, int64_t n_rows, int M,
                 int K, int dtype, const float* pro_scale, const float* pro_shift, float slope, void* workspace,
                 size_t workspace_bytes, ddmp_stream stream);
int ddmp_bn_stats(const void* Y, int64_t ldy, int64_t n_rows, int C, int dtype, double* sums, void* workspace,
                  size_t workspace_bytes, ddmp_stream stream);
int ddmp_bn_bwd_reduce(const void* dZ, int64_t lddz, const void* Y, int64_t ldy, int64_t n_rows, int C, int dtype,
                       const float* scale, const float* shift, const float* mean, const float* rstd, float slope,
                       double* sums2, void* workspace, size_t workspace_bytes, ddmp_stream stream);
int ddmp_bn_bwd_apply(const void* dZ, int64_t lddz, const void* Y, int64_t ldy, void* dY, int64_t lddy, int64_t n_rows,
                      int C, int dtype, const float* scale, const float* shift, const float* c1, const float* c0,
                      float slope, double* dbias_sums, void* workspace, size_t workspace_bytes, ddmp_stream stream);
int ddmp_head_fwd(const void* Y, int64_t ldy, int64_t n_rows, int dtype, const float* scale, const float* shift,
                  float slope, const float* W1, const float* b1, const float* W2, const float* b2, int kind,
                  const float* x_pos, float* out, ddmp_stream stream);
int ddmp_head_bwd(const void* Y, int64_t ldy, int64_t n_rows, int dtype, const float* scale, const float* shift,
                  float slope, const float* W1, const float* b1, const float* W2, const float* b2, int kind,
                  const float* dout, void* dZ, int64_t lddz, float* dW1, float* db1, float* dW2, float* db2,
                  void* workspace, size_t workspace_bytes, ddmp_stream stream);


/* ------------------------------------------------------------------ ABI 3: per-call options
 * What a call can be asked for beyond its own arguments is an explicit, nullable last argument of the call itself:
 * `name_o(<the arguments of name>, const ddmp_opts* opts)`.  The options apply to THAT call and to nothing else (whatever it
 * returns); opts == NULL is the plain call.  A malformed block is DDMP_EINVAL before any device work; so are BatchNorm
 * coefficients asked of a call that has no float64 column reduction, or whose reduction is not bn_C columns wide.  A call that
 * fails writes no coefficients.
 *   DDMP_OPT_BN_FWD   the call's float64 [2C] reduction (sum y, sum y^2) also yields what ddmp_bn_prepare_f32 would write:
 *                     bn_in = {gamma, beta}, bn_out = {scale, shift, mean, rstd, running_mean | NULL, running_var | NULL}
 *   DDMP_OPT_BN_BWD   ... (sum g, sum g yhat) also yields what ddmp_bn_bwd_prepare_f32 would write:
 *                     bn_in = {scale, mean, rstd}, bn_out = {dgamma, dbeta, c1, c0}
 *                     (bn_C must be the reduction's width, bn_n_total the row count of the whole batch)
 *   DDMP_OPT_SCALES   f16x3 GEMM mode: persistent scale slots of the operands (slot_a: the row operand A / dZ / G, slot_b:
 *                     Z of the tn forms, either may be NULL); prime != 0: measure now (first iteration)
 *   DDMP_OPT_PREPARED `workspace` holds weight planes written by ddmp_gemm_prepare_weights for exactly this product */
#define DDMP_OPT_BN_FWD 1u
#define DDMP_OPT_BN_BWD 2u
#define DDMP_OPT_SCALES 4u
#define DDMP_OPT_PREPARED 8u
typedef struct ddmp_opts {
    uint32_t struct_size; /* sizeof(ddmp_opts) of the caller's header */
    uint32_t flags;       /* DDMP_OPT_* */
    double bn_n_total;
    int32_t bn_C;
    float bn_eps, bn_momentum;
    int32_t prime;
    const float* bn_in[3];
    float* bn_out[6];
    float* slot_a;
    float* slot_b;
} ddmp_opts;
int ddmp_bn_stats_o(const void* Y, int64_t ldy, int64_t n_rows, int C, int dtype, double* sums, void* workspace,
    size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts);
int ddmp_bn_bwd_reduce_o(const void* dZ, int64_t lddz, const void* Y, int64_t ldy, int64_t n_rows, int C, int dtype,
    const float* scale, const float* shift, const float* mean, const float* rstd, float slope, double* sums2,
    void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts);
int ddmp_spmm_stats_o(const ddmp_graph* g, const void* X, int64_t ldx, void* Y, int64_t ldy, int C, int dtype,
    const float* bias, const float* pro_scale, const float* pro_shift, float slope, const float* ref, double* sums2,
    void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts);
int ddmp_spmm_bnred_o(const ddmp_graph* g, const void* X, int64_t ldx, void* Y, int64_t ldy, int C, int dtype,
    const void* Yp, int64_t ldyp, const float* scale, const float* shift, const float* mean, const float* rstd,
    float slope, double* sums2, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts);
int ddmp_gemm_nt_o(const void* A, int64_t lda, const float* W, int64_t ldw, void* Y, int64_t ldy, int64_t n_rows,
    int K, int M, int dtype, const float* bias, const float* pro_scale, const float* pro_shift, float slope,
    void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts);
int ddmp_gemm_nn_o(const void* A, int64_t lda, const float* W, int64_t ldw, void* Y, int64_t ldy, int64_t n_rows,
    int M, int K, int dtype, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts);
int ddmp_gemm_tn_o(const void* G, int64_t ldg, const void* Z, int64_t ldz, float* dW, int64_t lddw, int64_t n_rows,
    int M, int K, int dtype, const float* pro_scale, const float* pro_shift, float slope, void* workspace,
    size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts);
int ddmp_gemm_nt_stats_f32_o(const float* A, int64_t lda, const float* W, int64_t ldw, float* Y, int64_t ldy,
    int64_t n_rows, int K, int M, const float* bias , const float* pro_scale , const float* pro_shift , float slope,
    double* sums2 , void* workspace, size_t workspace_bytes, void* stats_ws, size_t stats_ws_bytes, ddmp_stream stream,
    const ddmp_opts* opts);
int ddmp_gemm_nt_stats_bf16_o(const uint16_t* A, int64_t lda, const float* W, int64_t ldw, uint16_t* Y, int64_t ldy,
    int64_t n_rows, int K, int M, const float* bias, const float* pro_scale, const float* pro_shift, float slope,
    double* sums2, void* workspace, size_t workspace_bytes, void* stats_ws, size_t stats_ws_bytes, ddmp_stream stream,
    const ddmp_opts* opts);
int ddmp_gemm_nn_bnred_f32_o(const float* A, int64_t lda, const float* W, int64_t ldw, float* out, int64_t ld_out,
    int64_t n_rows, int M, int K, const float* Yp, int64_t ldyp, const float* scale, const float* shift,
    const float* mean, const float* rstd, float slope, double* sums2, void* workspace, size_t workspace_bytes,
    void* stats_ws, size_t stats_ws_bytes, ddmp_stream stream, const ddmp_opts* opts);
int ddmp_gemm_nn_bnbwd_f32_o(const float* dZ, int64_t lddz, const float* Yb, int64_t ldyb, const float* W, int64_t ldw,
    float* out, int64_t ld_out, int64_t n_rows, int M, int K, const float* a, const float* b, const float* c1,
    const float* c0, float slope, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts);
int ddmp_gemm_tn_bnbwd_f32_o(const float* dZ, int64_t lddz, const float* Yb, int64_t ldyb, const float* Z, int64_t ldz,
    float* dW, int64_t lddw, int64_t n_rows, int M, int K, const float* a, const float* b, const float* c1,
    const float* c0, const float* pro_scale , const float* pro_shift , float slope, void* workspace,
    size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DDMP_HIP_H */

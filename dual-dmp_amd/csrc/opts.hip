// ABI 3: the *_o entry points -- per-call options (include/ddmp_hip.h, ddmp_opts).  An _o form validates its options into a
// CallCtx of its own (finalize.h), passes it to the context-taking form of the call it wraps (ddmp_internal.h) and runs the one
// epilogue below: nothing an _o call is given can reach another call.
#include "ddmp_common.h"
#include "finalize.h"

namespace {
using ddmp::FinalizeArgs;

// `sums`, `width`: the float64 [2 * width] column reduction of the wrapped call (none: nullptr, 0) -- BatchNorm coefficients can
// only be asked of a call that has one, of exactly bn_C columns
struct OptCall {
    int err = DDMP_OK;
    ddmp::CallCtx ctx;
    const double* sums;
    ddmp_stream stream;
    OptCall(const ddmp_opts* o, ddmp_stream stream_, const double* sums_ = nullptr, int width = 0) : sums(sums_), stream(stream_) {
        if (o) err = fill(*o, width);
    }
    int fill(const ddmp_opts& o, int width) {
        ARG_TRY(o.struct_size >= sizeof(ddmp_opts));
        ARG_TRY(!(o.flags & ~(DDMP_OPT_BN_FWD | DDMP_OPT_BN_BWD | DDMP_OPT_SCALES | DDMP_OPT_PREPARED)));
        ARG_TRY(!((o.flags & DDMP_OPT_BN_FWD) && (o.flags & DDMP_OPT_BN_BWD)));
        if (o.flags & (DDMP_OPT_BN_FWD | DDMP_OPT_BN_BWD)) {
            FinalizeArgs& f = ctx.fin;
            f.kind = (o.flags & DDMP_OPT_BN_FWD) ? 1 : 2;
            f.C = o.bn_C; f.n_total = o.bn_n_total; f.eps = o.bn_eps; f.momentum = o.bn_momentum;
            for (int i = 0; i < 3; ++i) f.in[i] = o.bn_in[i];
            for (int i = 0; i < 6; ++i) f.out[i] = o.bn_out[i];
            ARG_TRY(sums && f.C == width && f.n_total > 0 && f.C > 0 && f.in[0] && f.in[1] && f.out[0] && f.out[1] && f.out[2] && f.out[3]);
            if (f.kind == 1) ARG_TRY((f.out[4] == nullptr) == (f.out[5] == nullptr));
            else ARG_TRY(f.in[2]);
        }
        if (o.flags & DDMP_OPT_SCALES) {
            ctx.slot_a = o.slot_a; ctx.slot_b = o.slot_b; ctx.prime = o.prime;
        }
        ctx.prepared = (o.flags & DDMP_OPT_PREPARED) != 0;
        return DDMP_OK;
    }
    // behind the wrapped call: it succeeded, coefficients were requested and no second stage wrote them (a route without
    // one) -> the stand-alone kernel over the call's sums
    int finish(int rc) {
        const FinalizeArgs& f = ctx.fin;
        if (rc != DDMP_OK || f.kind == 0 || ctx.fin_done) return rc;
        if (f.kind == 1)
            return ddmp_bn_prepare_f32(sums, f.n_total, f.C, f.in[0], f.in[1], f.eps, f.momentum, f.out[0], f.out[1], f.out[2],
                                       f.out[3], f.out[4], f.out[5], stream);
        return ddmp_bn_bwd_prepare_f32(sums, f.n_total, f.C, f.in[0], f.in[1], f.in[2], f.out[0], f.out[1], f.out[2], f.out[3], stream);
    }
};
}  // namespace

extern "C" int ddmp_bn_stats_o(const void* Y, int64_t ldy, int64_t n_rows, int C, int dtype, double* sums, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream, sums, C);
    if (c.err) return c.err;
    return c.finish(ddmp_bn_stats(Y, ldy, n_rows, C, dtype, sums, workspace, workspace_bytes, stream, c.ctx));
}

extern "C" int ddmp_bn_bwd_reduce_o(const void* dZ, int64_t lddz, const void* Y, int64_t ldy, int64_t n_rows, int C, int dtype, const float* scale, const float* shift, const float* mean, const float* rstd, float slope, double* sums2, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream, sums2, C);
    if (c.err) return c.err;
    return c.finish(ddmp_bn_bwd_reduce(dZ, lddz, Y, ldy, n_rows, C, dtype, scale, shift, mean, rstd, slope, sums2, workspace, workspace_bytes, stream, c.ctx));
}

extern "C" int ddmp_spmm_stats_o(const ddmp_graph* g, const void* X, int64_t ldx, void* Y, int64_t ldy, int C, int dtype, const float* bias, const float* pro_scale, const float* pro_shift, float slope, const float* ref, double* sums2, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream, sums2, C);
    if (c.err) return c.err;
    return c.finish(ddmp_spmm_stats(g, X, ldx, Y, ldy, C, dtype, bias, pro_scale, pro_shift, slope, ref, sums2, workspace, workspace_bytes, stream, c.ctx));
}

extern "C" int ddmp_spmm_bnred_o(const ddmp_graph* g, const void* X, int64_t ldx, void* Y, int64_t ldy, int C, int dtype, const void* Yp, int64_t ldyp, const float* scale, const float* shift, const float* mean, const float* rstd, float slope, double* sums2, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream, sums2, C);
    if (c.err) return c.err;
    return c.finish(ddmp_spmm_bnred(g, X, ldx, Y, ldy, C, dtype, Yp, ldyp, scale, shift, mean, rstd, slope, sums2, workspace, workspace_bytes, stream, c.ctx));
}

extern "C" int ddmp_gemm_nt_o(const void* A, int64_t lda, const float* W, int64_t ldw, void* Y, int64_t ldy, int64_t n_rows, int K, int M, int dtype, const float* bias, const float* pro_scale, const float* pro_shift, float slope, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream);
    if (c.err) return c.err;
    return c.finish(ddmp_gemm_nt(A, lda, W, ldw, Y, ldy, n_rows, K, M, dtype, bias, pro_scale, pro_shift, slope, workspace, workspace_bytes, stream, c.ctx));
}

extern "C" int ddmp_gemm_nn_o(const void* A, int64_t lda, const float* W, int64_t ldw, void* Y, int64_t ldy, int64_t n_rows, int M, int K, int dtype, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream);
    if (c.err) return c.err;
    return c.finish(ddmp_gemm_nn(A, lda, W, ldw, Y, ldy, n_rows, M, K, dtype, workspace, workspace_bytes, stream, c.ctx));
}

extern "C" int ddmp_gemm_tn_o(const void* G, int64_t ldg, const void* Z, int64_t ldz, float* dW, int64_t lddw, int64_t n_rows, int M, int K, int dtype, const float* pro_scale, const float* pro_shift, float slope, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream);
    if (c.err) return c.err;
    return c.finish(ddmp_gemm_tn(G, ldg, Z, ldz, dW, lddw, n_rows, M, K, dtype, pro_scale, pro_shift, slope, workspace, workspace_bytes, stream, c.ctx));
}

extern "C" int ddmp_gemm_nt_stats_f32_o(const float* A, int64_t lda, const float* W, int64_t ldw, float* Y, int64_t ldy, int64_t n_rows, int K, int M, const float* bias , const float* pro_scale , const float* pro_shift , float slope, double* sums2 , void* workspace, size_t workspace_bytes, void* stats_ws, size_t stats_ws_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream, sums2, M);
    if (c.err) return c.err;
    return c.finish(ddmp_gemm_nt_stats_f32(A, lda, W, ldw, Y, ldy, n_rows, K, M, bias, pro_scale, pro_shift, slope, sums2, workspace, workspace_bytes, stats_ws, stats_ws_bytes, stream, c.ctx));
}

extern "C" int ddmp_gemm_nt_stats_bf16_o(const uint16_t* A, int64_t lda, const float* W, int64_t ldw, uint16_t* Y, int64_t ldy, int64_t n_rows, int K, int M, const float* bias, const float* pro_scale, const float* pro_shift, float slope, double* sums2, void* workspace, size_t workspace_bytes, void* stats_ws, size_t stats_ws_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream, sums2, M);
    if (c.err) return c.err;
    return c.finish(ddmp_gemm_nt_stats_bf16(A, lda, W, ldw, Y, ldy, n_rows, K, M, bias, pro_scale, pro_shift, slope, sums2, workspace, workspace_bytes, stats_ws, stats_ws_bytes, stream, c.ctx));
}

extern "C" int ddmp_gemm_nn_bnred_f32_o(const float* A, int64_t lda, const float* W, int64_t ldw, float* out, int64_t ld_out, int64_t n_rows, int M, int K, const float* Yp, int64_t ldyp, const float* scale, const float* shift, const float* mean, const float* rstd, float slope, double* sums2, void* workspace, size_t workspace_bytes, void* stats_ws, size_t stats_ws_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream, sums2, K);
    if (c.err) return c.err;
    return c.finish(ddmp_gemm_nn_bnred_f32(A, lda, W, ldw, out, ld_out, n_rows, M, K, Yp, ldyp, scale, shift, mean, rstd, slope, sums2, workspace, workspace_bytes, stats_ws, stats_ws_bytes, stream, c.ctx));
}

extern "C" int ddmp_gemm_nn_bnbwd_f32_o(const float* dZ, int64_t lddz, const float* Yb, int64_t ldyb, const float* W, int64_t ldw, float* out, int64_t ld_out, int64_t n_rows, int M, int K, const float* a, const float* b, const float* c1, const float* c0, float slope, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream);
    if (c.err) return c.err;
    return c.finish(ddmp_gemm_nn_bnbwd_f32(dZ, lddz, Yb, ldyb, W, ldw, out, ld_out, n_rows, M, K, a, b, c1, c0, slope, workspace, workspace_bytes, stream, c.ctx));
}

extern "C" int ddmp_gemm_tn_bnbwd_f32_o(const float* dZ, int64_t lddz, const float* Yb, int64_t ldyb, const float* Z, int64_t ldz, float* dW, int64_t lddw, int64_t n_rows, int M, int K, const float* a, const float* b, const float* c1, const float* c0, const float* pro_scale , const float* pro_shift , float slope, void* workspace, size_t workspace_bytes, ddmp_stream stream, const ddmp_opts* opts) {
    OptCall c(opts, stream);
    if (c.err) return c.err;
    return c.finish(ddmp_gemm_tn_bnbwd_f32(dZ, lddz, Yb, ldyb, Z, ldz, dW, lddw, n_rows, M, K, a, b, c1, c0, pro_scale, pro_shift, slope, workspace, workspace_bytes, stream, c.ctx));
}

// Tail-fused finalisation of the column reductions, and the per-call context that carries it.
//
// Every BatchNorm of the path turns a float64 [2C] result of a column reduction into float32 per-column coefficients:
// forward (sum y, sum y^2) -> scale / shift / mean / rstd (+ running statistics); backward (sum g, sum g*yhat) -> dgamma,
// dbeta, c1, c0.  As a kernel of its own behind the reduction's second stage that is 48 launches of ~3 us per iteration, 11 %
// of the launches of a 13k-face mesh.  A reducing call that is given DDMP_OPT_BN_FWD / DDMP_OPT_BN_BWD (include/ddmp_hip.h,
// ddmp_opts) has its second-stage kernel (one thread holds both sums of a column) write the coefficients too, with the
// arithmetic of bn_prepare_kernel / bn_bwd_prepare_kernel (same device function: bitwise the same values).  On a route
// without a second stage the _o entry point runs the stand-alone kernel behind the call (opts.hip), so "requested => the
// coefficients exist when the call returns DDMP_OK" holds on every route.
#pragma once
#include "ddmp_common.h"

namespace ddmp {

struct FinalizeArgs {
    int kind = 0;                  // 0 nothing | 1 BatchNorm forward coefficients | 2 BatchNorm backward coefficients
    int C = 0;
    double n_total = 0.0;
    const float* in[3] = {nullptr, nullptr, nullptr};   // 1: gamma, beta, -          2: scale, mean, rstd
    float* out[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    //                                1: scale, shift, mean, rstd, running_mean, running_var      2: dgamma, dbeta, c1, c0
    float eps = 0.f, momentum = 0.f;
};

// column c: s0 = sums[c], s1 = sums[C + c]
__device__ __forceinline__ void finalize_column(const FinalizeArgs& f, int c, double s0, double s1) {
    if (f.kind == 1) {
        const double mu = s0 / f.n_total;
        double var = s1 / f.n_total - mu * mu;                   // biased
        if (var < 0.0) var = 0.0;
        const float muf = (float)mu;
        const float rs = (float)(1.0 / sqrt(var + (double)f.eps));
        const float a = f.in[0][c] * rs;
        f.out[0][c] = a;
        f.out[1][c] = fmaf(-muf, a, f.in[1][c]);
        f.out[2][c] = muf;
        f.out[3][c] = rs;
        if (f.out[4]) {
            const double unb = f.n_total > 1.0 ? var * f.n_total / (f.n_total - 1.0) : var;
            f.out[4][c] = (1.f - f.momentum) * f.out[4][c] + f.momentum * muf;
            f.out[5][c] = (1.f - f.momentum) * f.out[5][c] + f.momentum * (float)unb;
        }
    } else if (f.kind == 2) {
        const double db = s0, dg = s1;
        f.out[1][c] = (float)db;
        f.out[0][c] = (float)dg;
        const double a = f.in[0][c], r = f.in[2][c], mu = f.in[1][c];
        const double k1 = -a * r * dg / f.n_total;
        f.out[2][c] = (float)k1;
        f.out[3][c] = (float)(-a * db / f.n_total - k1 * mu);
    }
}

// One call's options (ddmp_opts, validated by the _o entry point: opts.hip), passed by reference from that entry point down
// to the launch helper that consumes them.  An exported entry point without options runs on an empty one.
struct CallCtx {
    FinalizeArgs fin;                                            // kind 0: no BatchNorm coefficients requested
    bool fin_done = false;                                       // a second-stage kernel of this call has written them
    float* slot_a = nullptr;                                     // DDMP_OPT_SCALES: f16 split mode (gemm_f16s.inc), the
    float* slot_b = nullptr;                                     // operands' persistent scale slots
    int prime = 0;
    bool prepared = false;                                       // DDMP_OPT_PREPARED
    // second stage of a reduction over C columns: the coefficients it writes as well (kind 0: none), marked as written
    FinalizeArgs take_fin(int C) {
        if (fin.kind == 0 || fin_done || fin.C != C) return FinalizeArgs();
        fin_done = true;
        return fin;
    }
};

}  // namespace ddmp

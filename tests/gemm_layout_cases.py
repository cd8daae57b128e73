"""The cases of tests/test_gpu_gemm_layouts.py and tests/test_gemm_routes_cpu.py: one GEMM shape per kernel family at the smallest
row counts inside the family (default thresholds: row-register 10000, row panels 20000, wgrad panels 30000), with the family
each case exists for in every GEMM mode it is run in.  tests/test_gemm_routes_cpu.py asserts the table against the library's
route queries (host only), so a moved threshold fails there instead of silently emptying a GPU test.

Row products are named by their contraction and output width, whatever the entry point: out[n, MD] = f(a[n, KD]) . B with
B = w[MD, KD]^T (gemm_nt, gemm_nt_stats) or B = w[KD, MD] (gemm_nn, gemm_nn_bnred, gemm_nn_bnbwd).  Weight gradients:
out[M, K] = g[n, M]^T . f(z[n, K])."""
from collections import namedtuple

# families / kernels as ops.ROW_FAMILIES and ops.TN_KERNELS name them
F16, B16, TILED, PRE, PLAIN = "f16x3-panel", "bf16-panel", "tiled", "presplit", "plain"
TN_F16, TN_PANEL, TN_TILED, TN_F32 = "f16x3-rowmajor", "bf16-panel", "bf16-tiled", "f32-tiled"

# eps: the entry points run on the shape ("nt_pro": gemm_nt with the BatchNorm+LeakyReLU prologue, "nt_stats_pro" likewise).
# fam: mode -> (family, row-register kernel) without a prologue; pro_fam: the same with one, where it differs.
# odd: mode -> the family an output with ldy % 4 != 0 falls to, where it differs.
RowCase = namedtuple("RowCase", "n KD MD eps fam pro_fam odd")


def _row(n, KD, MD, eps, fam, pro_fam=None, odd=None):
    return RowCase(n, KD, MD, tuple(eps.split()), fam, pro_fam or {}, odd or {})


ROW_CASES = [
    # row-register f16x3; the first with padded MP = 256 beside live neighbour columns
    _row(10003, 64, 132, "nt nt_pro nt_stats nt_stats_pro nn nn_bnred", {13: (F16, True)}),
    _row(12289, 256, 512, "nt nt_pro nt_stats nt_stats_pro nn nn_bnred", {13: (F16, True)}),
    # f16x3 row panel, not row-register (KD > 512); with a prologue the f32-input MFMA (KD > kMaxProK)
    _row(20003, 544, 256, "nt nt_pro nn", {13: (F16, False)}, pro_fam={13: (PLAIN, False)}),
    # bf16 row panels, NJ = 1 / 4 / 4, padded and full
    _row(20003, 32, 16, "nt nt_pro nt_stats nn", {13: (B16, False)}),
    _row(20003, 64, 100, "nt nt_stats nn", {13: (B16, False), 6: (B16, False), 3: (B16, False)}),
    _row(20003, 256, 128, "nt nt_stats nn nn_bnred", {13: (B16, False)}),
    # BatchNorm-backward dgrads: panel (dual, MP > kRRCols), row-register, narrow panel
    _row(30003, 512, 512, "nn_bnbwd", {13: (F16, False)}),
    _row(30003, 512, 256, "nn_bnbwd", {13: (F16, True)}),
    _row(30003, 128, 64, "nn_bnbwd", {13: (B16, False), 6: (B16, False), 3: (B16, False), 0: (PLAIN, False)}),
    # tiled; an output the float4 stores cannot reach makes it presplit
    _row(777, 96, 260, "nt nt_pro nn", {13: (TILED, False)}, odd={13: (PRE, False)}),
    _row(513, 256, 128, "nt nn", {13: (TILED, False), 6: (TILED, False), 3: (TILED, False), 0: (PLAIN, False)},
         odd={13: (PRE, False), 6: (PRE, False), 3: (PRE, False)}),
    # presplit
    _row(513, 40, 36, "nt nt_pro nn", {13: (PRE, False), 6: (PRE, False), 3: (PRE, False)}),
    _row(130, 8, 32, "nt nn", {13: (PRE, False)}),
    # plain (the split kernels' tile-by-tile form: KD % 8 != 0)
    _row(50, 12, 20, "nt nt_pro nn", {13: (PLAIN, False), 6: (PLAIN, False), 3: (PLAIN, False), 0: (PLAIN, False)}),
    _row(50, 12, 3, "nt", {13: (PLAIN, False)}),
]

# fam: mode -> (kernel, T, tm, tk); odd: the same for operands the float4 loads cannot reach (gemm_tn_bnbwd only: "odd-in")
TnCase = namedtuple("TnCase", "n M K eps fam odd")


def _tn(n, M, K, eps, fam, odd=None):
    return TnCase(n, M, K, tuple(eps.split()), fam, odd or {})


TN_CASES = [
    _tn(1000, 64, 32, "tn tn_pro", {13: (TN_TILED, 1, 0, 0), 6: (TN_TILED, 1, 0, 0), 3: (TN_TILED, 1, 0, 0), 0: (TN_F32, 1, 0, 0)}),
    _tn(1000, 128, 256, "tn tn_pro", {13: (TN_TILED, 2, 0, 0)}),
    # f16x3 row-major: wide, both narrow panels, one partial panel
    _tn(30003, 256, 256, "tn tn_pro tn_bnbwd tn_bnbwd_pro",
        {13: (TN_F16, 4, 256, 256), 6: (TN_PANEL, 4, 256, 256), 3: (TN_PANEL, 4, 256, 256), 0: (TN_F32, 2, 0, 0)},
        odd={13: (TN_PANEL, 4, 256, 256)}),
    _tn(30003, 256, 128, "tn tn_bnbwd", {13: (TN_F16, 4, 256, 128)}),
    _tn(30003, 128, 256, "tn tn_bnbwd", {13: (TN_F16, 4, 128, 256)}),
    _tn(30003, 320, 128, "tn tn_bnbwd", {13: (TN_F16, 4, 256, 128)}),
    # first-layer tiled dual
    _tn(30003, 32, 16, "tn_bnbwd", {13: (TN_TILED, 1, 0, 0), 6: (TN_TILED, 1, 0, 0), 3: (TN_TILED, 1, 0, 0)}),
    _tn(30003, 64, 32, "tn_bnbwd", {13: (TN_TILED, 1, 0, 0)}, odd={13: (TN_TILED, 1, 0, 0)}),
]

# bfloat16 features: (n, KD, MD) of the row products / (n, M, K) = (n, MD, KD) of the weight gradient
BF16_CASES = [(12289, 256, 512), (20003, 64, 128), (30003, 256, 256)]

# the large-offset case: n_rows * lda * 4 just exceeds 2^32, beyond the row-register kernel's 32-bit lane offsets
BIG = RowCase(10003, 64, 132, ("nt", "nn_bnred"), {13: (F16, False)}, {}, {})
BIG_LDA = 107400


def row_id(c):
    return "%dx%dx%d" % (c.n, c.KD, c.MD)


def tn_id(c):
    return "%dx%dx%d" % (c.n, c.M, c.K)


def layout(name, widths, out_index, d=1):
    """-> [(ld, off)] per operand (widths in call order; out_index: the output operand).
    block: ld = width + 4, off = 4; mixed: (width + 4, 4) | (2 width, 12) | (width + 8, 8) in turn (2 width: at least
    width + 12, so that the block fits); odd-out: as block, the output with ld = width + d, off = 1."""
    if name == "mixed":
        pick = [lambda w: (w + 4, 4), lambda w: (max(2 * w, w + 12), 12), lambda w: (w + 8, 8)]
        return [pick[i % 3](w) for i, w in enumerate(widths)]
    out = [(w + 4, 4) for w in widths]
    if name == "odd-out":
        out[out_index] = (widths[out_index] + d, 1)
    return out

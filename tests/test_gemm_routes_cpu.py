"""The route queries ddmp_gemm_row_route / ddmp_gemm_tn_route (host only: no GPU) against the table of tests/gemm_layout_cases.py:
every case of tests/test_gpu_gemm_layouts.py lands on the kernel family it exists for, in every GEMM mode it is run in, for the
contiguous call and for each layout; the leading dimensions and alignments that move a call to another family do so."""
import os

import pytest

import gemm_layout_cases as gc

DEFAULT_CONFIG = not any(k.startswith("DDMP_") and k != "DDMP_LIB" for k in os.environ)
pytestmark = pytest.mark.skipif(not DEFAULT_CONFIG, reason="the table is written for the default thresholds and switches")


@pytest.fixture
def ops():
    from dual_dmp_amd import ops
    old = ops.get_gemm_mode()
    yield ops
    ops.set_gemm_mode(old)


def test_the_queries_are_declared_and_exported():
    from dual_dmp_amd import _lib
    protos = _lib.parse_header()
    L = _lib.lib()
    assert len(protos["ddmp_gemm_row_route"][1]) == 8 and len(protos["ddmp_gemm_tn_route"][1]) == 6
    assert L.ddmp_abi_version() == 3
    assert L.ddmp_gemm_row_route(0, 32, 32, 0, 32, 0, 32, 0) == -1 and L.ddmp_gemm_tn_route(10, 0, 32, 0, 1, None) == -1


@pytest.mark.parametrize("case", gc.ROW_CASES, ids=gc.row_id)
def test_row_cases_land_on_their_family(ops, case):
    n, KD, MD = case.n, case.KD, case.MD
    dual = "nn_bnbwd" in case.eps
    for mode, want in case.fam.items():
        ops.set_gemm_mode(mode)
        for name in ("contiguous", "block", "mixed"):
            (lda, _), (ldy, _) = ((KD, 0), (MD, 0)) if name == "contiguous" else gc.layout(name, [KD, MD], 1)
            lda2 = (2 * KD if name == "mixed" else lda) if dual else 0
            assert ops.gemm_row_route(n, KD, MD, False, lda, lda2, ldy) == want, (mode, name)
            if any(e.endswith("_pro") for e in case.eps):
                assert ops.gemm_row_route(n, KD, MD, True, lda, 0, ldy) == case.pro_fam.get(mode, want), (mode, name, "pro")
        # an output the float4 stores cannot reach: only the tiled family minds
        for d in (1, 2, 3):
            got = ops.gemm_row_route(n, KD, MD, False, KD + 4, KD + 4 if dual else 0, MD + d, True)
            assert got == case.odd.get(mode, want), (mode, "odd-out", d)
        got = ops.gemm_row_route(n, KD, MD, False, KD + 4, KD + 4 if dual else 0, MD + 4, True)
        assert got == case.odd.get(mode, want), (mode, "Y off 16 bytes")
        if "nn_bnred" in case.eps:
            assert ops.gemm_nn_bnred_supported(KD, MD, n), mode
        if dual:
            assert ops.gemm_bnbwd_supported(KD, MD, n) == (mode != 0), mode
    if 13 in case.fam and case.fam[13] == (gc.F16, True):
        ops.set_gemm_mode(13)
        # 32-bit lane offsets: the row-register kernel up to n_rows * lda * 4 < 2^32, the row-panel kernel beyond
        edge = (1 << 30) // n // 4 * 4
        assert ops.gemm_row_route(n, KD, MD, False, edge, 0, MD) == (gc.F16, True)
        assert ops.gemm_row_route(n, KD, MD, False, edge + 4, 0, MD) == (gc.F16, False)


def test_the_large_offset_case_leaves_the_row_register_kernel(ops):
    ops.set_gemm_mode(13)
    c = gc.BIG
    assert (1 << 32) < (c.n - 1) * gc.BIG_LDA * 4 < 1.001 * (1 << 32)      # the last rows lie just beyond 4 GiB
    assert ops.gemm_row_route(c.n, c.KD, c.MD, False, gc.BIG_LDA, 0, c.MD) == c.fam[13]
    assert ops.gemm_row_route(c.n, c.KD, c.MD, False, c.KD, 0, c.MD) == (gc.F16, True)


@pytest.mark.parametrize("case", gc.TN_CASES, ids=gc.tn_id)
def test_wgrad_cases_land_on_their_kernel(ops, case):
    n, M, K = case.n, case.M, case.K
    for mode, want in case.fam.items():
        ops.set_gemm_mode(mode)
        for ep in case.eps:
            dual = ep.startswith("tn_bnbwd")
            if dual and mode == 0:                                 # no f32-input kernel for the dual form: refused before
                assert not ops.gemm_tn_bnbwd_supported(M, K, n)
                continue
            got = ops.gemm_tn_route(n, M, K, dual)
            assert got[:4] == want and got[4] >= 8, (mode, ep, got)         # (several splits: reduce_splits_kernel adds them)
            if dual:
                assert ops.gemm_tn_bnbwd_supported(M, K, n), (mode, ep)
    for mode, want in case.odd.items():
        ops.set_gemm_mode(mode)
        assert ops.gemm_tn_route(n, M, K, True, ld_ok=False)[:4] == want, (mode, "odd-in")


def test_every_family_and_kernel_is_reached(ops):
    fams = {(m, f) for c in gc.ROW_CASES for m, f in list(c.fam.items()) + list(c.pro_fam.items()) + list(c.odd.items())}
    assert {f for m, f in fams if m == 13} == {(gc.F16, True), (gc.F16, False), (gc.B16, False), (gc.TILED, False), (gc.PRE, False),
                                                 (gc.PLAIN, False)}
    for mode in (6, 3):
        assert {f[0] for m, f in fams if m == mode} == {gc.B16, gc.TILED, gc.PRE, gc.PLAIN}
    kernels = {(m, f[0]) for c in gc.TN_CASES for m, f in list(c.fam.items()) + list(c.odd.items())}
    assert {k for m, k in kernels if m == 13} == {gc.TN_F16, gc.TN_PANEL, gc.TN_TILED}
    assert (0, gc.TN_F32) in kernels and (6, gc.TN_PANEL) in kernels and (3, gc.TN_TILED) in kernels

"""Every GEMM route (csrc/gemm.hip, csrc/gemm_b16.hip) on operands that are column blocks of wider buffers, with n_rows below
the buffers' rows -- what the multi-device path and any caller of the C ABI hand the library, and no other GPU test does.

Every operand of a call is a column block [off, off + width) of a [rows + 3, ld] buffer (layouts: tests/gemm_layout_cases.py).
Input buffers are hostile outside the operand -- NaN in one run, 3.0e38 in another (fmaxf drops a NaN, so only a large finite
value shows an absolute-maximum pre-pass that looked outside its operand) -- and must be bit-identical after the call; output
buffers start as the sentinel -7.25 and must still be that bit pattern outside [0, n) x [off, off + width).

Per case: the contiguous call within the project's bound of the float64 product (GEMM_TOL / 3e-6 of tests/test_gpu_kernels.py);
where the route query names the same kernel family for the laid-out call, the block is bitwise the contiguous result (and so
are the float64 sums); where it names another (an output the tiled kernel's float4 stores cannot reach, wgrad operands its
float4 loads cannot reach), the family it fell to is asserted and the result compared with float64 at the same bound.

One line per layout is printed (`pytest -s`): entry point, shape, mode, family, layout, fill, rel-L2 against float64."""
import os

import pytest
import torch

import gemm_layout_cases as gc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEFAULT_CONFIG = not any(k.startswith("DDMP_") and k != "DDMP_LIB" for k in os.environ)
SENT = -7.25
HOSTILE = {"nan": float("nan"), "huge": 3.0e38}
GEMM_TOL = {6: 2e-6, 3: 3e-5, 0: 2e-6, 13: 2e-6}                 # tests/test_gpu_kernels.py
BNBWD_TOL = 3e-6                                                 # the *_bnbwd forms there (run in the f32-class default mode only)


def tolerance(mode, bnbwd):
    """rel-L2 bound against float64.  The *_bnbwd forms: 3e-6 in the f32-class modes, as tests/test_gpu_kernels.py asks of them in the
    default mode.  Mode 3 (bf16x3) leaves out the cross terms of relative size 2^-16 in every product, whatever feeds the operand
    load: there the arithmetic's own bound GEMM_TOL[3] holds, as tests/test_gpu_bn.py has it for these same fused routes
    (K_GEMM x 10).  Measured in mode 3: gemm_nn_bnbwd 30003 x 128 -> 64 4.5e-6."""
    return max(BNBWD_TOL, GEMM_TOL[mode]) if bnbwd else GEMM_TOL[mode]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture
def in_mode(request):
    """The GEMM arithmetic named by the test's `mode` parameter (13 where it has none), the previous one put back afterwards."""
    from dual_dmp_amd import ops
    old = ops.get_gemm_mode()
    mode = request.node.callspec.params.get("mode", 13) if hasattr(request.node, "callspec") else 13
    ops.set_gemm_mode(mode)
    yield mode
    ops.set_gemm_mode(old)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def supported(answer, what):
    """A `*_supported` predicate answering no: a failure in the default configuration, a skip under a switch."""
    if not answer:
        assert not DEFAULT_CONFIG, "%s refused in the default configuration" % what
        pytest.skip("%s switched off in this configuration" % what)


def relerr(y, ref):
    return float((y.double() - ref).norm() / ref.norm())


def lrelu(x, slope):
    return torch.where(x > 0, x, slope * x)


def dy64(dz, yb, bn4, c10, slope):
    a, b, k1, k0 = bn4[0].double(), bn4[1].double(), c10[0].double(), c10[1].double()
    y = yb.double()
    return a * dz.double() * torch.where(y * a + b > 0, 1.0, slope) + k1 * y + k0


def _blocked(t, ld, off, fill):
    """A [rows + 3, ld] buffer of `fill` whose column block [off, off + width) holds t in its first rows -> (buffer, block)."""
    buf = torch.full((t.shape[0] + 3, ld), fill, dtype=t.dtype, device=t.device)
    blk = buf[:, off:off + t.shape[1]]
    blk[:t.shape[0]].copy_(t)
    return buf, blk


def _out(rows, width, ld, off, dev, dtype=torch.float32):
    buf = torch.full((rows + 3, ld), SENT, dtype=dtype, device=dev)
    return buf, buf[:, off:off + width]


def _untouched(buf, n, C, off):
    """Everything outside rows [0, n) x columns [off, off + C) is still the sentinel, bit for bit."""
    s = bits(torch.full((1,), SENT, dtype=buf.dtype, device=buf.device))[0]
    b = bits(buf)
    return bool((b[n:] == s).all() and (b[:n, :off] == s).all() and (b[:n, off + C:] == s).all())


def _same(buf, keep):
    return torch.equal(bits(buf), bits(keep))


def _views(operands, T, lay, fill, n):
    """The input operands as blocks of hostile buffers -> (views by name, [(buffer, copy before the call)], leading dimensions)."""
    v, held, lds = {}, [], {}
    for (name, key), (ld, off) in zip(operands, lay):
        buf, blk = _blocked(T[key], ld, off, fill)
        held.append((buf, buf.clone()))
        v[name] = blk if name != "w" else blk[:T[key].shape[0]]
        lds[name] = ld
    return v, held, lds


_DATA = {}


def data(dev, kind, n, c0, c1):
    """Operands of one shape on the device (randn: only the layout is hard here); the last shape is kept for the tests that share it."""
    key = (kind, n, c0, c1)
    if key not in _DATA:
        _DATA.clear()
        g = torch.Generator(device=dev)
        g.manual_seed(n + c0 + c1)

        def rn(*s):
            return torch.randn(*s, device=dev, generator=g)

        def ru(*s):
            return torch.rand(*s, device=dev, generator=g)
        if kind == "row":                                          # c0 = KD, c1 = MD
            T = dict(a=rn(n, c0), w=rn(c1, c0) / c0 ** 0.5, wt=rn(c0, c1) / c0 ** 0.5, bias=rn(c1), sc=ru(c0) + 0.5, sh=rn(c0),
                     yb=rn(n, c0) * 2 + 0.5, bn4=torch.stack([ru(c0) + 0.5, rn(c0), rn(c0), ru(c0) + 0.5]),
                     c10=torch.stack([rn(c0) * 0.1, rn(c0) * 0.1]), yp=rn(n, c1) * 2 + 0.3,
                     rbn4=torch.stack([ru(c1) + 0.5, rn(c1), rn(c1) * 0.1 + 0.3, ru(c1) + 0.5]))
        else:                                                      # c0 = M, c1 = K
            T = dict(g=rn(n, c0), z=rn(n, c1), yb=rn(n, c0) * 2 + 0.5, bn4=torch.stack([ru(c0) + 0.5, rn(c0), rn(c0), ru(c0) + 0.5]),
                     c10=torch.stack([rn(c0) * 0.1, rn(c0) * 0.1]), sc=ru(c1) + 0.5, sh=rn(c1))
        _DATA[key] = T
    return _DATA[key]


# ------------------------------------------------------------------------------------------------ row products
ROW_OPERANDS = {"nt": [("a", "a"), ("w", "w")], "nn": [("a", "a"), ("w", "wt")],
                "nn_bnred": [("a", "a"), ("w", "wt"), ("yp", "yp")], "nn_bnbwd": [("a", "a"), ("yb", "yb"), ("w", "wt")]}
for _e in ("nt_pro", "nt_stats", "nt_stats_pro"):
    ROW_OPERANDS[_e] = ROW_OPERANDS["nt"]
HAS_SUMS = ("nt_stats", "nt_stats_pro", "nn_bnred")


def row_call(ops, ep, T, v, n, sums=None, **kw):
    kw.update(out=v["y"], n_rows=n)
    pro = (T["sc"], T["sh"])
    if ep == "nt":
        return ops.gemm_nt(v["a"], v["w"], bias=v["bias"], **kw)
    if ep == "nt_pro":
        return ops.gemm_nt(v["a"], v["w"], pro=pro, **kw)
    if ep == "nt_stats":
        return ops.gemm_nt_stats(v["a"], v["w"], sums, bias=v["bias"], **kw)
    if ep == "nt_stats_pro":
        return ops.gemm_nt_stats(v["a"], v["w"], sums, pro=pro, **kw)
    if ep == "nn":
        return ops.gemm_nn(v["a"], v["w"], **kw)
    if ep == "nn_bnred":
        return ops.gemm_nn_bnred(v["a"], v["w"], v["yp"], T["rbn4"], sums, **kw)
    assert ep == "nn_bnbwd"
    return ops.gemm_nn_bnbwd(v["a"], v["yb"], v["w"], T["bn4"], T["c10"], **kw)


def row_reference(ep, T, slope):
    A = T["a"].double()
    if ep in ("nt", "nt_stats"):
        return A @ T["w"].double().t() + T["bias"].double()
    if ep in ("nt_pro", "nt_stats_pro"):
        return lrelu(A * T["sc"].double() + T["sh"].double(), slope) @ T["w"].double().t()
    if ep in ("nn", "nn_bnred"):
        return A @ T["wt"].double()
    return dy64(T["a"], T["yb"], T["bn4"], T["c10"], slope) @ T["wt"].double()


def _bias_view(T, fill):
    """The bias as a view at a 4-byte offset of a longer, otherwise hostile vector."""
    vec = torch.full((T["bias"].numel() + 2,), fill, device=T["bias"].device)
    vec[1:-1] = T["bias"]
    return vec[1:-1]


def row_contiguous(ops, ep, T, n, MD, dev, **kw):
    v = {name: T[key] for name, key in ROW_OPERANDS[ep]}
    v["bias"], v["y"] = T["bias"], torch.full((n, MD), SENT, device=dev)
    sums = torch.zeros(2 * MD, dtype=torch.float64, device=dev) if ep in HAS_SUMS else None
    row_call(ops, ep, T, v, n, sums, **kw)
    return v["y"], sums


def row_laid_out(ops, ep, T, n, MD, lay, fill, dev, pro, **kw):
    """One call on blocked operands -> (output block, sums, route named by the query); the buffers are checked here."""
    operands = ROW_OPERANDS[ep]
    v, held, lds = _views(operands, T, lay, fill, n)
    v["bias"] = _bias_view(T, fill)
    ldy, offy = lay[-1]
    ybuf, v["y"] = _out(n, MD, ldy, offy, dev)
    sums = torch.zeros(2 * MD, dtype=torch.float64, device=dev) if ep in HAS_SUMS else None
    route = ops.gemm_row_route(n, T["a"].shape[1], MD, pro, lds["a"], lds.get("yb", 0), ldy, v["y"].data_ptr() % 16 != 0)
    row_call(ops, ep, T, v, n, sums, **kw)
    assert _untouched(ybuf, n, MD, offy), "written outside the output block"
    for buf, keep in held:
        assert _same(buf, keep), "an input buffer changed"
    return v["y"][:n], sums, route


ROW_LAYOUTS = [("block", 0, "nan"), ("block", 0, "huge"), ("mixed", 0, "nan"), ("mixed", 0, "huge"),
               ("odd-out", 1, "nan"), ("odd-out", 2, "huge"), ("odd-out", 3, "nan")]
ROW_PARAMS = [pytest.param(c, ep, mode, id="%s-%s-m%d" % (gc.row_id(c), ep, mode)) for c in gc.ROW_CASES for ep in c.eps for mode in c.fam]


@pytest.mark.parametrize("case,ep,mode", ROW_PARAMS)
def test_row_products_on_blocked_operands(dev, in_mode, case, ep, mode):
    from dual_dmp_amd import ops
    n, KD, MD = case.n, case.KD, case.MD
    T = data(dev, "row", n, KD, MD)
    pro, dual = ep.endswith("_pro"), ep == "nn_bnbwd"
    tol = tolerance(mode, dual)
    want = case.pro_fam.get(mode, case.fam[mode]) if pro else case.fam[mode]
    route_c = ops.gemm_row_route(n, KD, MD, pro, KD, KD if dual else 0, MD)
    if DEFAULT_CONFIG:
        assert route_c == want
    if dual and mode == 0:                                         # no f32-input kernel rebuilds dY on the load: refused, nothing written
        assert not ops.gemm_bnbwd_supported(KD, MD, n)
        with pytest.raises(ops.DdmpError, match="status -1 "):
            y, _ = row_contiguous(ops, ep, T, n, MD, dev)
        lay = gc.layout("block", [KD, KD, MD, MD], 3)
        v, held, lds = _views(ROW_OPERANDS[ep], T, lay, HOSTILE["nan"], n)
        ybuf, v["y"] = _out(n, MD, *lay[-1], dev)
        with pytest.raises(ops.DdmpError, match="status -1 "):
            row_call(ops, ep, T, v, n)
        assert _untouched(ybuf, 0, 0, 0)
        return
    if dual:
        supported(ops.gemm_bnbwd_supported(KD, MD, n), "gemm_nn_bnbwd %d <- %d" % (MD, KD))
    if ep == "nn_bnred":
        supported(ops.gemm_nn_bnred_supported(KD, MD, n), "gemm_nn_bnred %d <- %d" % (MD, KD))
    yc, sums_c = row_contiguous(ops, ep, T, n, MD, dev)
    ref = row_reference(ep, T, ops.SLOPE)
    err_c = relerr(yc, ref)
    print("GEMMLAYOUT %s %s mode %d %s contiguous rel-L2 %.2e" % (ep, gc.row_id(case), mode, route_c, err_c))
    assert err_c < tol
    if ep in ("nt_stats", "nt_stats_pro"):                         # the sums are those of the stored output
        yd = yc.double()
        assert relerr(sums_c[:MD], yd.sum(0)) < 1e-6 and relerr(sums_c[MD:], (yd * yd).sum(0)) < 1e-6
    widths = [T[key].shape[1] for _, key in ROW_OPERANDS[ep]] + [MD]
    for name, d, fname in (ROW_LAYOUTS if mode == 13 else ROW_LAYOUTS[:2]):
        lay = gc.layout(name, widths, len(widths) - 1, d)
        y, sums, route = row_laid_out(ops, ep, T, n, MD, lay, HOSTILE[fname], dev, pro)
        err = relerr(y, ref)
        print("GEMMLAYOUT %s %s mode %d %s %s%s %s rel-L2 %.2e" % (ep, gc.row_id(case), mode, route, name, "+%d" % d if d else "", fname, err))
        if route == route_c:
            assert torch.equal(bits(y), bits(yc)), (name, d, fname, "not bitwise the contiguous result")
            if sums is not None:
                assert torch.equal(sums, sums_c), (name, d, fname, "sums")
        else:
            assert name == "odd-out"
            if DEFAULT_CONFIG:
                assert route == case.odd[mode]
            assert err < tol, (name, d, fname, err)
    if route_c[0] == gc.F16 and ep in ("nt", "nn"):
        # caller scale slots: the measured maximum is that of the block alone, and the product is the one the call's own slot gives
        slot = torch.zeros(1, 4, device=dev)
        y, _, _ = row_laid_out(ops, ep, T, n, MD, gc.layout("block", widths, len(widths) - 1), HOSTILE["huge"], dev, pro,
                               scales=(slot[0], None, True))
        amax = float(T["a"].abs().max())
        assert float(slot[0, 0]) == amax and float(slot[0, 1]) == amax, (slot.tolist(), amax)
        assert torch.equal(bits(y), bits(yc))


# ------------------------------------------------------------------------------------------------ weight gradients
TN_OPERANDS = {"tn": [("g", "g"), ("z", "z")], "tn_bnbwd": [("g", "g"), ("yb", "yb"), ("z", "z")]}
TN_OPERANDS["tn_pro"], TN_OPERANDS["tn_bnbwd_pro"] = TN_OPERANDS["tn"], TN_OPERANDS["tn_bnbwd"]


def tn_call(ops, ep, T, v, n, **kw):
    kw.update(out=v["dw"], n_rows=n, pro=(T["sc"], T["sh"]) if ep.endswith("_pro") else None)
    if ep.startswith("tn_bnbwd"):
        return ops.gemm_tn_bnbwd(v["g"], v["yb"], v["z"], T["bn4"], T["c10"], **kw)
    return ops.gemm_tn(v["g"], v["z"], **kw)


def tn_reference(ep, T, slope):
    G = dy64(T["g"], T["yb"], T["bn4"], T["c10"], slope) if ep.startswith("tn_bnbwd") else T["g"].double()
    Z = T["z"].double()
    if ep.endswith("_pro"):
        Z = lrelu(Z * T["sc"].double() + T["sh"].double(), slope)
    return G.t() @ Z


def tn_laid_out(ops, ep, T, n, M, K, lay, fill, dev, **kw):
    dual = ep.startswith("tn_bnbwd")
    v, held, lds = _views(TN_OPERANDS[ep], T, lay, fill, n)
    ld_ok = all(ld % 4 == 0 for ld in lds.values()) and all(t.data_ptr() % 16 == 0 for t in v.values())
    lddw, offw = lay[-1]
    wbuf, blk = _out(M, K, lddw, offw, dev)
    v["dw"] = blk[:M]
    route = ops.gemm_tn_route(n, M, K, dual, ld_ok)
    assert ld_ok or route[0] != gc.TN_F16, "the f16x3 route on operands its float4 loads cannot reach"
    tn_call(ops, ep, T, v, n, **kw)
    assert _untouched(wbuf, M, K, offw), "written outside the dW block"
    for buf, keep in held:
        assert _same(buf, keep), "an input buffer changed"
    return v["dw"], route


TN_LAYOUTS = ROW_LAYOUTS + [("odd-in", 0, "nan"), ("odd-in", 0, "huge")]
TN_PARAMS = [pytest.param(c, ep, mode, id="%s-%s-m%d" % (gc.tn_id(c), ep, mode)) for c in gc.TN_CASES for ep in c.eps for mode in c.fam]


@pytest.mark.parametrize("case,ep,mode", TN_PARAMS)
def test_weight_gradients_on_blocked_operands(dev, in_mode, case, ep, mode):
    from dual_dmp_amd import ops
    n, M, K = case.n, case.M, case.K
    T = data(dev, "tn", n, M, K)
    dual = ep.startswith("tn_bnbwd")
    tol = tolerance(mode, dual)
    widths = [T[key].shape[1] for _, key in TN_OPERANDS[ep]] + [K]

    def contiguous():
        v = {name: T[key] for name, key in TN_OPERANDS[ep]}
        v["dw"] = torch.full((M, K), SENT, device=dev)
        tn_call(ops, ep, T, v, n)
        return v["dw"]
    if dual and mode == 0:                                         # refused, nothing written
        assert not ops.gemm_tn_bnbwd_supported(M, K, n)
        with pytest.raises(ops.DdmpError, match="status -1 "):
            contiguous()
        lay = gc.layout("block", widths, len(widths) - 1)
        v, held, lds = _views(TN_OPERANDS[ep], T, lay, HOSTILE["nan"], n)
        wbuf, blk = _out(M, K, *lay[-1], dev)
        v["dw"] = blk[:M]
        with pytest.raises(ops.DdmpError, match="status -1 "):
            tn_call(ops, ep, T, v, n)
        assert _untouched(wbuf, 0, 0, 0)
        return
    if dual:
        supported(ops.gemm_tn_bnbwd_supported(M, K, n), "gemm_tn_bnbwd %d x %d" % (M, K))
    route_c = ops.gemm_tn_route(n, M, K, dual, True)
    if DEFAULT_CONFIG:
        assert route_c[:4] == case.fam[mode]
    dwc = contiguous()
    ref = tn_reference(ep, T, ops.SLOPE)
    err_c = relerr(dwc, ref)
    print("GEMMLAYOUT %s %s mode %d %s contiguous rel-L2 %.2e" % (ep, gc.tn_id(case), mode, route_c, err_c))
    assert err_c < tol
    for name, d, fname in (TN_LAYOUTS if mode == 13 else TN_LAYOUTS[:2]):
        if name == "odd-in":
            if not (dual and mode in case.odd):
                continue
            # leading dimensions that are no multiples of 4, one base (z) off 16 bytes: accepted on purpose by this entry point
            lay = [(M + 5, 4), (M + 6, 4), (K + 7, 1), (K + 4, 4)]
        else:
            lay = gc.layout(name, widths, len(widths) - 1, d)
        dw, route = tn_laid_out(ops, ep, T, n, M, K, lay, HOSTILE[fname], dev)
        err = relerr(dw, ref)
        print("GEMMLAYOUT %s %s mode %d %s %s%s %s rel-L2 %.2e" % (ep, gc.tn_id(case), mode, route, name, "+%d" % d if d else "", fname, err))
        if name != "odd-in":
            assert route == route_c
            assert torch.equal(bits(dw), bits(dwc)), (name, d, fname, "not bitwise the contiguous result")
        else:
            if DEFAULT_CONFIG:
                assert route[:4] == case.odd[mode]
            assert err < tol, (name, fname, err)
    if route_c[0] == gc.TN_F16 and ep == "tn":                     # both caller slots: the maxima of the blocks alone
        slots = torch.zeros(2, 4, device=dev)
        dw, _ = tn_laid_out(ops, ep, T, n, M, K, gc.layout("block", widths, len(widths) - 1), HOSTILE["huge"], dev,
                            scales=(slots[0], slots[1], True))
        assert float(slots[0, 0]) == float(T["g"].abs().max()) and float(slots[1, 0]) == float(T["z"].abs().max()), slots.tolist()
        assert torch.equal(bits(dw), bits(dwc))


# ------------------------------------------------------------------------------------------------ W as a block; prepared planes
@pytest.mark.parametrize("n,KD,MD,ep", [(10003, 64, 132, "nt"), (10003, 64, 132, "nn"), (20003, 64, 100, "nt"), (20003, 64, 100, "nn"),
                                        (513, 256, 128, "nt"), (513, 40, 36, "nn")])
def test_prepared_planes_of_a_weight_block(dev, in_mode, n, KD, MD, ep):
    """W as a block (ldw = width + 4) of a hostile buffer, its planes made by gemm_prepare_weights from that same view: bitwise the
    contiguous call with its own split -- and the planes are what the call reads (W zeroed afterwards changes nothing)."""
    from dual_dmp_amd import ops
    T = data(dev, "row", n, KD, MD)
    yc, _ = row_contiguous(ops, ep, T, n, MD, dev)
    src = T["w"] if ep == "nt" else T["wt"]
    route = ops.gemm_row_route(n, KD, MD, False, KD, 0, MD)
    assert route[0] != gc.PLAIN or not DEFAULT_CONFIG              # (the plain family keeps no planes)
    for fname, fill in HOSTILE.items():
        wbuf, blk = _blocked(src, src.shape[1] + 4, 4, fill)
        w = blk[:src.shape[0]]
        planes = torch.zeros(ops.gemm_rows_workspace_bytes(KD, MD), dtype=torch.uint8, device=dev)
        ops.gemm_prepare_weights([(w, 0 if ep == "nt" else 1, False, planes)], n, torch.zeros(8, device=dev))
        keep = wbuf.clone()
        for zeroed in (False, True):
            if zeroed:
                w.zero_()
            v = dict(a=T["a"], w=w, bias=T["bias"], y=torch.full((n, MD), SENT, device=dev))
            row_call(ops, ep, T, v, n, wplanes=planes)
            assert torch.equal(bits(v["y"]), bits(yc)), (fname, zeroed)
            if not zeroed:
                assert _same(wbuf, keep)
        ops.gemm_forget_planes(planes)
        print("GEMMLAYOUT prepared %s %dx%dx%d %s ldw %d %s bitwise" % (ep, n, KD, MD, route, src.shape[1] + 4, fname))


# ------------------------------------------------------------------------------------------------ bfloat16 features
def _bf16_layout(name, widths, dtypes):
    out = []
    for i, (w, dt) in enumerate(zip(widths, dtypes)):
        if dt != BF:                                               # the float32 operands (W, dW) by the float32 rule
            out.append((w + 4, 4))
        elif name == "block":
            out.append((w + 8, 8))
        else:
            out.append([(w + 8, 8), (max(2 * w, w + 16), 16), (w + 16, 8)][i % 3])
    return out


@pytest.mark.parametrize("ep", ["nt", "nt_stats", "nn", "nn_bnbwd", "tn", "tn_bnbwd"])
@pytest.mark.parametrize("n,KD,MD", gc.BF16_CASES, ids=lambda v: str(v))
def test_bf16_features_on_blocked_operands(dev, n, KD, MD, ep):
    """bfloat16 features: ld = width + 8 | 2 width | width + 16, offsets multiples of 8; bitwise the contiguous call, nothing
    outside touched.  Where ddmp_gemm_fused_bf16_supported says a fused form does not exist for the shape, the statistics come from
    the separate pass (gemm_nt_stats) or the call is refused and writes nothing (gemm_nn_bnbwd)."""
    from dual_dmp_amd import ops
    wg = ep in ("tn", "tn_bnbwd")
    T32 = data(dev, "tn" if wg else "row", n, MD if wg else KD, KD if wg else MD)
    T = {k: (t.to(BF) if k in ("a", "yb", "yp", "g", "z") else t) for k, t in T32.items()}
    operands = TN_OPERANDS[ep] if wg else ROW_OPERANDS[ep]
    rows_out, width_out, out_dt = (MD, KD, torch.float32) if wg else (n, MD, BF)
    call = tn_call if wg else row_call
    oname = "dw" if wg else "y"
    refused = ep == "nn_bnbwd" and not ops.gemm_bnbwd_supported(KD, MD, n, BF)

    def run(v, sums):
        if wg:
            return call(ops, ep, T, v, n)
        return call(ops, ep, T, v, n, sums)
    v = {name: T[key] for name, key in operands}
    v["bias"] = T.get("bias")
    v[oname] = torch.full((rows_out, width_out), SENT, dtype=out_dt, device=dev)
    sums_c = torch.zeros(2 * MD, dtype=torch.float64, device=dev) if ep == "nt_stats" else None
    if refused:
        with pytest.raises(ops.DdmpError, match="status -1 "):
            run(v, sums_c)
        assert bool((v[oname] == SENT).all())
    else:
        run(v, sums_c)
    yc = v[oname]
    widths = [T[key].shape[1] for _, key in operands] + [width_out]
    dtypes = [T[key].dtype for _, key in operands] + [out_dt]
    for name in ("block", "mixed"):
        for fname, fill in HOSTILE.items():
            lay = _bf16_layout(name, widths, dtypes)
            v, held, lds = _views(operands, T, lay, fill, n)
            v["bias"] = T.get("bias")
            obuf, blk = _out(rows_out, width_out, *lay[-1], dev, out_dt)
            v[oname] = blk[:rows_out] if wg else blk
            sums = torch.zeros(2 * MD, dtype=torch.float64, device=dev) if ep == "nt_stats" else None
            if refused:
                with pytest.raises(ops.DdmpError, match="status -1 "):
                    run(v, sums)
                assert _untouched(obuf, 0, 0, 0)
                continue
            run(v, sums)
            assert _untouched(obuf, rows_out, width_out, lay[-1][1]), (name, fname)
            for buf, keep in held:
                assert _same(buf, keep), (name, fname)
            assert torch.equal(bits(blk[:rows_out]), bits(yc)), (name, fname, "not bitwise the contiguous result")
            if sums is not None:
                assert torch.equal(sums, sums_c), (name, fname)
            print("GEMMLAYOUT bf16 %s %dx%dx%d %s %s %s" % (ep, n, KD, MD, name, fname, "refused" if refused else "bitwise"))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_the_argument_error_and_write_nothing(dev, in_mode):
    """What each entry point's argument checks state: a leading dimension that is no multiple of 4 (bfloat16: of 8), an A or W base
    off 16 bytes, lda < K, ldw < K, ldy < M -> DDMP_EINVAL (-1), outputs untouched.  Each entry point is first called with good
    arguments of the same shape (status 0), so that the refusal is the argument's.  ddmp_gemm_tn_bnbwd_f32 takes leading
    dimensions that are no multiples of 4 and bases off 16 bytes on purpose (the odd-in cases above): only its `<` refusals."""
    from dual_dmp_amd import ops, _lib
    L = _lib.lib()
    n, C, ld = 30003, 256, 264
    st, slope = ops._stream(), 0.01
    A = torch.full((n + 1, ld), 0.5, device=dev)
    Ab = torch.full((n + 1, ld), 0.5, device=dev, dtype=BF)
    W = torch.full((C + 1, ld), 0.01, device=dev)
    co = torch.full((4, C), 0.5, device=dev)
    ws = torch.zeros(128 << 20, dtype=torch.uint8, device=dev)    # ample: no refusal here is about the workspace
    sws = torch.zeros(max(L.ddmp_gemm_nt_stats_workspace_bytes(n, C), 1 << 20), dtype=torch.uint8, device=dev)
    out = torch.full((n + 1, ld), SENT, device=dev)
    outb = torch.full((n + 1, ld), SENT, device=dev, dtype=BF)
    sums = torch.full((2 * C,), SENT, dtype=torch.float64, device=dev)
    c = [co[i].data_ptr() for i in range(4)]
    wsa, swsa = (ws.data_ptr(), ws.numel()), (sws.data_ptr(), sws.numel())

    def nt(a, lda, w, ldw, ldy):
        return L.ddmp_gemm_nt(a, lda, w, ldw, out.data_ptr(), ldy, n, C, C, 0, None, None, None, slope, *wsa, st)

    def nn(a, lda, w, ldw, ldy):
        return L.ddmp_gemm_nn(a, lda, w, ldw, out.data_ptr(), ldy, n, C, C, 0, *wsa, st)

    def nt_stats(a, lda, w, ldw, ldy):
        return L.ddmp_gemm_nt_stats_f32(a, lda, w, ldw, out.data_ptr(), ldy, n, C, C, None, None, None, slope, sums.data_ptr(), *wsa, *swsa, st)

    def nn_bnred(a, lda, w, ldw, ldy):
        return L.ddmp_gemm_nn_bnred_f32(a, lda, w, ldw, out.data_ptr(), ldy, n, C, C, A.data_ptr(), ld, *c, slope, sums.data_ptr(), *wsa, *swsa, st)

    def nn_bnbwd(a, lda, w, ldw, ldy):
        return L.ddmp_gemm_nn_bnbwd_f32(a, lda, A.data_ptr(), ld, w, ldw, out.data_ptr(), ldy, n, C, C, *c, slope, *wsa, st)

    def nn_bnbwd_yb(a, lda, w, ldw, ldy):                          # the same refusals of the second operand (Yb)
        return L.ddmp_gemm_nn_bnbwd_f32(A.data_ptr(), ld, a, lda, w, ldw, out.data_ptr(), ldy, n, C, C, *c, slope, *wsa, st)

    def tn(a, lda, w, ldw, ldy):                                   # (G, ldg), (Z, ldz), lddw
        return L.ddmp_gemm_tn(a, lda, w, ldw, out.data_ptr(), ldy, n, C, C, 0, None, None, slope, *wsa, st)

    def tn_bnbwd(a, lda, w, ldw, ldy):                             # (dZ, lddz), (Z, ldz), lddw
        return L.ddmp_gemm_tn_bnbwd_f32(a, lda, A.data_ptr(), ld, w, ldw, out.data_ptr(), ldy, n, C, C, *c, None, None, slope, *wsa, st)
    a0, w0 = A.data_ptr(), W.data_ptr()

    def variations(b0, which):
        """Good arguments are (a0, ld, b0, ld, ld); b0: the base of the second operand -- W [C, ld], or for the weight gradients the
        activation operand Z, n rows of it (here A again: every row the call may read lies inside the buffer)."""
        v = {"lda < K": (a0, C - 4, b0, ld, ld), "ldw < K": (a0, ld, b0, C - 4, ld), "ldy < M": (a0, ld, b0, ld, C - 4),
             "lda % 4": (a0, ld + 2, b0, ld, ld), "A off 16 bytes": (a0 + 4, ld, b0, ld, ld),
             "ldw % 4": (a0, ld, b0, ld + 2, ld), "W off 16 bytes": (a0, ld, b0 + 4, ld, ld)}
        return (b0, {k: v[k] for k in which})
    small = ("lda < K", "ldw < K", "ldy < M")
    first = small + ("lda % 4", "A off 16 bytes")
    every = first + ("ldw % 4", "W off 16 bytes")
    entries = [(nt, variations(w0, every)), (nn, variations(w0, every)), (nt_stats, variations(w0, every)),
               (nn_bnred, variations(w0, every)), (nn_bnbwd, variations(w0, every)),
               (nn_bnbwd_yb, variations(w0, [k for k in first if k != "ldy < M"])),
               (tn, variations(a0, every)), (tn_bnbwd, variations(a0, small))]      # (the second operand of a wgrad is Z [n, K])
    if not DEFAULT_CONFIG:
        entries = [e for e in entries if e[0] in (nt, nn, tn)]      # the fused forms may be switched off: every call is then refused
    for fn, (b0, cases) in entries:
        assert fn(a0, ld, b0, ld, ld) == 0, fn.__name__
        torch.cuda.synchronize()
        out.fill_(SENT)
        sums.fill_(SENT)
        for what, args in cases.items():
            assert fn(*args) == -1, (fn.__name__, what)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and bool((sums == SENT).all()), fn.__name__
    # bfloat16 features: leading dimensions multiples of 8, bases on 16 bytes
    ab, ob = Ab.data_ptr(), outb.data_ptr()

    def nt_b(a, lda, ldw, y, ldy):
        return L.ddmp_gemm_nt(a, lda, w0, ldw, y, ldy, n, C, C, 1, None, None, None, slope, *wsa, st)

    def nn_b(a, lda, ldw, y, ldy):
        return L.ddmp_gemm_nn(a, lda, w0, ldw, y, ldy, n, C, C, 1, ws.data_ptr(), ws.numel(), st)

    def tn_b(a, lda, ldw, y, ldy):                                 # (G, ldg), ldz, (dW, lddw)
        return L.ddmp_gemm_tn(a, lda, ab, ldw, out.data_ptr(), ldy, n, C, C, 1, None, None, slope, *wsa, st)
    bad_b = {"lda % 8": (ab, ld + 4, ld, ob, ld), "lda < K": (ab, C - 8, ld, ob, ld), "ldw < K": (ab, ld, C - 8, ob, ld),
             "ldy < M": (ab, ld, ld, ob, C - 8), "A off 16 bytes": (ab + 8, ld, ld, ob, ld)}
    bad_y = {"ldy % 8": (ab, ld, ld, ob, ld + 4), "Y off 16 bytes": (ab, ld, ld, ob + 8, ld)}
    for fn, cases in ((nt_b, dict(bad_b, **bad_y)), (nn_b, dict(bad_b, **bad_y)), (tn_b, dict(bad_b, **{"ldz % 8": (ab, ld, ld + 4, ob, ld)}))):
        assert fn(ab, ld, ld, ob, ld) == 0, fn.__name__
        torch.cuda.synchronize()
        out.fill_(SENT)
        outb.fill_(SENT)
        for what, args in cases.items():
            assert fn(*args) == -1, (fn.__name__, what)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and bool((outb == SENT).all()), fn.__name__


# ------------------------------------------------------------------------------------------------ rows past 4 GiB
def test_an_operand_whose_rows_lie_past_4_gib(dev, in_mode):
    """A as a block of a buffer with lda = 107,400 floats: n_rows * lda * 4 exceeds 2^32 and the last rows start beyond 4 GiB.  The
    row-register kernel forms 32-bit lane offsets: rr_kernel_ok sends the call to the row-panel kernel, whose row pointers are
    A + (int64_t)row * lda.  gemm_nn_bnred exists on the row-register kernel only for this shape: it is refused and writes nothing."""
    from dual_dmp_amd import ops
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GB of free device memory")
    c = gc.BIG
    n, KD, MD, lda = c.n, c.KD, c.MD, gc.BIG_LDA
    T = data(dev, "row", n, KD, MD)
    route = ops.gemm_row_route(n, KD, MD, False, lda, 0, MD)
    assert not route[1], "32-bit lane offsets cannot reach these rows"
    if DEFAULT_CONFIG:
        assert route == c.fam[13]
    ref = row_reference("nt", T, ops.SLOPE)
    buf = torch.empty((n + 3, lda), device=dev)
    off = lda - KD - 4                                             # the block at the far end of every row
    for fname, fill in HOSTILE.items():
        buf.fill_(fill)
        a = buf[:, off:off + KD]
        a[:n].copy_(T["a"])
        y = torch.full((n, MD), SENT, device=dev)
        ops.gemm_nt(a, T["w"], out=y, bias=T["bias"], n_rows=n)
        err = relerr(y, ref)
        print("GEMMLAYOUT nt %s mode 13 %s lda %d %s rel-L2 %.2e" % (gc.row_id(c), route, lda, fname, err))
        assert err < GEMM_TOL[13]
        assert torch.equal(bits(a[:n]), bits(T["a"]))
        out = torch.full((n, MD), SENT, device=dev)
        sums = torch.full((2 * MD,), SENT, dtype=torch.float64, device=dev)
        with pytest.raises(ops.DdmpError, match="status -1 "):
            ops.gemm_nn_bnred(a, T["wt"], T["yp"], T["rbn4"], sums, out=out, n_rows=n)
        assert bool((out == SENT).all()) and bool((sums == SENT).all())

"""The kernels that exponentiate, saturate or divide, at operands where float32 breaks unless the kernel guards it
(tests/extreme_operands.py; tests/test_extremes_cpu.py checks without a GPU that every family holds its condition and that the
references stay finite and meaningful there).  Every other parity test of the suite feeds ``randn``: a kernel with ``m = 0`` in
place of the row maximum, an unclamped clip coefficient or a step counter read one step late passes all of them.

1. edge softmax (gat.hip, gatv2.hip, tconv.hip): overflow / underflow / dominant / ties scores;
2. output heads (head.hip): every row count at which a loop wraps, strided buffers, ``n_rows`` below the buffer, tanh = +-1, u = 0;
3. optimizer (optim.hip): the clamp of the clip coefficient, a zero gradient, squares outside float32, the device-side step
   counter and coefficients;
4. the nine drop-ins of nn_ops.py on path graphs of 1 .. 65 nodes, and the refusal of a graph without any entry;
5. head softmax (feast.hip): steep logits, offsets of +-300, all-zero logits;
6. Gaussian mixture (gmm.hip): sigma = 2^-10, 0 and 2^10, mu = +-2^10, with and without the root term.

Tolerances.  Ordinary operands keep the bounds of the tests they extend (heads: out 2e-6, dz and parameter gradients 1e-5;
optimizer 1e-6; drop-ins on tiny graphs: OP_TOL, and the yardstick bound for the gradients their own files hold to it).  On the extreme families float32 input rounding is amplified by the score magnitude, so every compared quantity
uses the yardstick policy of test_gpu_gat.py: bound = max(4 x yardstick, FLOOR), the yardstick being the rel-L2 distance of the
float32 CPU evaluation of the same reference from its float64 evaluation on the same operands.  Norms are taken over whole
arrays.  Every test prints error, yardstick and bound."""
import numpy as np
import pytest
import torch

import extreme_operands as X
from extreme_operands import FLOOR, bound, graphs  # noqa: F401  (graphs: the fixture of test_gpu_gat.py)
from test_gpu_gat import dev  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
relerr = X.relerr
BF = torch.bfloat16


def ulp32(x):
    """float64 array: the spacing of float32 at |x|."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. edge softmax
def _run_softmax(op, ops, g, o, heads):
    got = {}
    if op == "gat":
        got["s_src"], got["s_dst"] = ops.gat_scores(o["hf"], o["att_src"], o["att_dst"], heads)
        got["y"], got["alpha"] = ops.gat_fwd(g, o["hf"], got["s_src"], got["s_dst"], heads, 0.2, bias=o["bias"])
        got["ds"], got["ds_dst"] = ops.gat_bwd_edge(g, o["dout"], o["hf"], got["s_src"], got["s_dst"], got["alpha"], heads, 0.2)
        got["dhf"], got["ds_src"] = ops.gat_bwd_node(g, o["dout"], got["alpha"], got["ds"], got["ds_dst"], o["att_src"],
                                                     o["att_dst"], heads)
        got["datt_src"], got["datt_dst"] = ops.gat_datt(o["hf"], got["ds_src"], got["ds_dst"], heads)
    elif op == "gatv2":
        got["y"], got["alpha"] = ops.gatv2_fwd(g, o["xl"], o["xr"], o["att"], heads, 0.2, bias=o["bias"])
        got["dz"], got["dxr"], part = ops.gatv2_bwd_edge(g, o["dout"], o["xl"], o["xr"], o["att"], got["alpha"], heads, 0.2)
        got["dxl"] = ops.gatv2_bwd_node(g, o["dout"], o["xl"], o["xr"], o["att"], got["alpha"], got["dz"], heads, 0.2)
        got["datt"] = ops.gatv2_datt(part, heads)
    else:
        got["y"], got["alpha"] = ops.tconv_fwd(g, o["q"], o["k"], o["v"], heads, skip=o["skip"])
        got["dz"], got["dq"] = ops.tconv_bwd_edge(g, o["dout"], o["k"], o["v"], got["alpha"], heads)
        got["dk"], got["dv"] = ops.tconv_bwd_node(g, o["dout"], o["q"], got["alpha"], got["dz"], heads)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.parametrize("op,family,name,loops,C,heads", X.softmax_cases())
def test_edge_softmax_at_extreme_scores(dev, graphs, op, family, name, loops, C, heads):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    o = X.softmax_operands(op, family, n, C, heads)
    ref, rows = X.softmax_reference(op, o, ei, n, heads, loops, torch.float64)
    r32, _ = X.softmax_reference(op, o, ei, n, heads, loops, torch.float32)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=loops)
    assert g.nnz == len(rows)
    got = _run_softmax(op, ops, g, {k: v.to(dev) for k, v in o.items()}, heads)
    assert sorted(got) == sorted(ref)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    # each row's alpha sums to 1 per head, to exactly 0 on the empty row, whose output is the bias / skip row alone
    alpha = got["alpha"].double()
    sums = torch.zeros((n, heads), dtype=torch.float64).index_add_(0, rows, alpha)
    empty = torch.from_numpy(np.bincount(rows.numpy(), minlength=n) == 0)
    assert bool(empty.any()) == name.endswith("-iso")
    assert float((sums[~empty] - 1).abs().max()) < 1e-5
    if empty.any():
        assert float(sums[empty].abs().max()) == 0.0
        init = o["skip"][empty] if op == "tconv" else o["bias"].expand(int(empty.sum()), -1)
        assert torch.equal(got["y"][empty], init)
    dz = got["ds" if op == "gat" else "dz"]
    if family == "dominant":
        assert bool(((alpha == 0) | (alpha == 1)).all()) and not dz.any()
    if family == "ties":
        mult = X.multiplicities(ei, n, loops)
        share = (mult / torch.zeros(n, dtype=torch.float64).index_add_(0, rows, mult)[rows]).unsqueeze(1).expand(-1, heads)
        over = ((alpha - share).abs().numpy() / ulp32(share.numpy())).max()
        print("%s ties %s C=%d heads=%d: alpha within %.2f float32 ulps of mult / sum(mult)" % (op, name, C, heads, over))
        assert over <= 2.0
    bad = []
    for k in ref:
        e, yard = X.measure(op, family, k, got, ref), X.measure(op, family, k, r32, ref)
        print("%s %s %s C=%d heads=%d %s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e"
              % (op, family, name, C, heads, k, e, yard, bound(yard)))
        if not e <= bound(yard):
            bad.append((k, e, yard))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 2. output heads
HEAD_SIZES = [1, 255, 256, 257, 131073, 524289]     # 131073 = 512 * 256 + 1: the backward tile loop wraps; 524289: the forward grid


def _head_call(ops, dev, o, kind, dtype, n, n_rows=None, strided=None):
    """One forward + backward.  ``strided`` = (first column, buffer width): y is that column block of a wider buffer, dz goes into
    the same block of a NaN-filled one.  -> dict(out [n, 3], dz [n, 32], dW1, db1, dW2, db2, dzbuf (the whole dz buffer))."""
    y = o["y"].to(dtype)
    nan = float("nan")
    if strided is None:
        yd = y.to(dev)
        dzbuf = torch.full((n, 32), nan, dtype=dtype, device=dev)
        dz = dzbuf
    else:
        c0, width = strided
        ybuf = torch.randn(n, width, generator=torch.Generator().manual_seed(n)).to(dtype).to(dev)
        ybuf[:, c0:c0 + 32] = y.to(dev)
        yd = ybuf[:, c0:c0 + 32]
        dzbuf = torch.full((n, width), nan, dtype=dtype, device=dev)
        dz = dzbuf[:, c0:c0 + 32]
    bn4 = torch.stack([o["a"], o["b"], torch.zeros(32), torch.ones(32)]).to(dev)
    P = [o[k].to(dev).contiguous() for k in ("W1", "b1", "W2", "b2")]
    out = torch.full((n, 3), nan, device=dev)
    ops.head_fwd(yd, bn4, *P, kind, o["x_pos"].to(dev), out, n_rows=n_rows)
    G = [torch.full_like(p, nan) for p in P]
    ops.head_bwd(yd, bn4, *P, kind, o["dout"].to(dev), dz, *G, n_rows=n_rows)
    torch.cuda.synchronize()
    fill = [torch.full((1,), nan, dtype=d, device=dev).cpu() for d in (torch.float32, dtype)]      # the fill's own bits
    return dict(out=out.cpu(), dz=dz.cpu(), dW1=G[0].cpu(), db1=G[1].cpu(), dW2=G[2].cpu(), db2=G[3].cpu(), dzbuf=dzbuf.cpu(),
                fill=fill)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _untouched(res, n, n_rows, strided):
    """Rows from ``n_rows`` on of out and dz, and every column of the dz buffer outside the block, are the NaN they were filled
    with, bit for bit."""
    buf = res["dzbuf"]
    nan32, nanb = _bits(res["fill"][0]), _bits(res["fill"][1])
    assert bool((_bits(res["out"][n_rows:]) == nan32).all())
    assert bool((_bits(buf[n_rows:]) == nanb).all())
    if strided is not None:
        c0 = strided[0]
        assert bool((_bits(buf[:, :c0]) == nanb).all()) and bool((_bits(buf[:, c0 + 32:]) == nanb).all())
    assert bool(torch.isfinite(res["out"][:n_rows]).all()) and bool(torch.isfinite(res["dz"][:n_rows].float()).all())


def _head_layouts(n, dtype):
    """(n_rows, strided): contiguous | columns 4:36 of an [n, 40] buffer with n_rows = n - 3.  bfloat16 rows are read 16 bytes at
    a time and the library refuses a block that does not start on 16 bytes (column 4 of bfloat16 is byte 8), so bfloat16 takes
    columns 8:40 of an [n, 48] buffer."""
    short = n - 3 if n > 3 else n
    return [(n, None), (short, (4, 40) if dtype == torch.float32 else (8, 48))]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", HEAD_SIZES)
def test_heads_float32_at_every_wrap_and_stride(dev, kind, n):
    from dual_dmp_amd import ops
    o = X.head_operands("ordinary", n, kind)
    for n_rows, strided in _head_layouts(n, torch.float32):
        ref = X.head_reference(o, kind, torch.float64, n_rows=n_rows)
        res = _head_call(ops, dev, o, kind, torch.float32, n, n_rows, strided)
        _untouched(res, n, n_rows, strided)
        for k in X.HEAD_KEYS:
            got = res[k][:n_rows] if k in ("out", "dz") else res[k]
            e = relerr(got, ref[k])
            print("head kind %d n=%d n_rows=%d %s %s: rel-L2 %.2e (tolerance %.0e)"
                  % (kind, n, n_rows, "strided" if strided else "contiguous", k, e, X.HEAD_TOL[k]))
            assert e < X.HEAD_TOL[k], (k, e)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", HEAD_SIZES)
def test_heads_bfloat16_equal_the_float32_heads_on_the_same_values(dev, kind, n):
    """The reference of the bfloat16 heads is the float32 head on the same rounded values
    (test_heads_bf16_equal_the_float32_heads_on_the_same_values): out and the parameter gradients bit for bit, dz rounded once."""
    from dual_dmp_amd import ops
    o = X.head_operands("ordinary", n, kind)
    o["y"] = (o["y"] * 1.5).to(BF).float()
    for n_rows, strided in _head_layouts(n, BF):
        f32 = _head_call(ops, dev, o, kind, torch.float32, n, n_rows, None)
        b16 = _head_call(ops, dev, o, kind, BF, n, n_rows, strided)
        _untouched(b16, n, n_rows, strided)
        assert torch.equal(b16["out"][:n_rows], f32["out"][:n_rows])
        assert torch.equal(b16["dz"][:n_rows], f32["dz"][:n_rows].to(BF))
        for k in ("dW1", "db1", "dW2", "db2"):
            assert torch.equal(b16[k], f32[k]), k


def test_heads_bfloat16_refuse_a_block_off_16_bytes(dev):
    from dual_dmp_amd import ops
    o = X.head_operands("ordinary", 257, 1)
    with pytest.raises(ops.DdmpError):
        _head_call(ops, dev, o, 1, BF, 257, 254, (4, 40))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("family", ["saturated", "zero"])
@pytest.mark.parametrize("n", [257, 131073])
def test_normal_head_saturated_and_zero(dev, family, n, dtype):
    """kind 1 where tanh(u) = +-1 exactly on every third row (1 - v^2 = 0: those rows' dz is exactly 0, the others carry the
    norms), and where u = 0 exactly on every row (r = 0: the ``r > 0 ? .. : 0`` guard and the 1 / (r + 1e-12) factor decide; out
    is exactly 0 and the gradients are of order 1e12 -- a case of its own, or they would carry every norm)."""
    from dual_dmp_amd import ops
    o = X.head_operands(family, n, 1)
    if dtype == BF:
        o["y"] = o["y"].to(BF).float()
        if family == "zero":                                     # y = -b / a is exact in 8 bits: still u = 0
            assert not X.head_reference(o, 1, torch.float32)["u"].any()
    ref, r32 = X.head_reference(o, 1, torch.float64), X.head_reference(o, 1, torch.float32)
    res = _head_call(ops, dev, o, 1, dtype, n)
    third = torch.arange(n) % 3 == 0
    for k in X.HEAD_KEYS:
        assert bool(torch.isfinite(res[k].float()).all()), k
    if family == "saturated":
        if dtype == BF:                                          # (rounding y may take a row out of saturation: re-select)
            third = third & (ref["u"].abs().min(1).values >= 20.0)
            assert int(third.sum()) > n // 4
        assert not res["dz"][third].any()
        assert float((res["out"][third].abs().double() - 3.0 ** -0.5).abs().max()) <= 2 * 2.0 ** -24      # +-1 / sqrt(3), 2 ulps
    else:
        assert not res["out"].any() and not res["dW1"].any() and not res["dW2"].any()
    if dtype == BF:                                              # its reference: the float32 head on the same rounded values
        f32 = _head_call(ops, dev, o, 1, torch.float32, n)
        assert torch.equal(res["out"], f32["out"]) and torch.equal(res["dz"], f32["dz"].to(BF))
        for k in ("dW1", "db1", "dW2", "db2"):
            assert torch.equal(res[k], f32[k]), k
        return
    bad = []
    for k in X.HEAD_KEYS:
        e, yard = relerr(res[k], ref[k]), relerr(r32[k], ref[k])
        print("head %s n=%d %s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (family, n, k, e, yard, bound(yard)))
        if not e <= bound(yard):
            bad.append((k, e, yard))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3. optimizer
def _state(n, dev):
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(n))
    return p0, p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)


@pytest.mark.parametrize("n", X.OPT_SIZES)
def test_a_norm_below_max_norm_is_not_touched(dev, n):
    """clip_coef clamps to 1: ``grad_clip_`` leaves g bit-identical, and ``adam_step_`` with ``clip_sumsq`` gives the bits of the
    call without it."""
    from dual_dmp_amd import ops
    _, p, m, v = _state(n, dev)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    for step in range(1, 4):
        g = X.optimizer_gradient("below", n, step).to(dev)
        ss = ops.grad_sumsq(g)
        assert 0.2 ** 2 < float(ss) <= 0.4 ** 2 * (1 + 1e-6) < X.MAX_NORM ** 2
        g2 = g.clone()
        ops.grad_clip_(g2, ss, X.MAX_NORM)
        assert torch.equal(g2, g)
        ops.adam_step_(p, g, m, v, X.LR, step, clip_sumsq=ss, max_norm=X.MAX_NORM)
        ops.adam_step_(p2, g, m2, v2, X.LR, step)
        assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2)
    assert not torch.equal(p.cpu(), _state(n, dev)[0])


@pytest.mark.parametrize("n", X.OPT_SIZES)
def test_a_zero_gradient_changes_nothing(dev, n):
    from dual_dmp_amd import ops
    p0, p, m, v = _state(n, dev)
    g = X.optimizer_gradient("zero", n, 1).to(dev)
    ss = ops.grad_sumsq(g)
    assert float(ss) == 0.0
    for step in (1, 2):
        ops.adam_step_(p, g, m, v, X.LR, step, clip_sumsq=ss, max_norm=X.MAX_NORM)
        ops.adam_step_(p, g, m, v, X.LR, step)
    ops.grad_clip_(g, ss, X.MAX_NORM)
    assert torch.equal(p.cpu(), p0) and not m.any() and not v.any() and not g.any()


@pytest.mark.parametrize("kind", X.OPT_SETS)
@pytest.mark.parametrize("n", X.OPT_SIZES)
def test_gradients_whose_squares_leave_float32(dev, n, kind):
    """+-1e20 and +-1e-30: the sum of squares is float64 by design; clip and five Adam steps against the float64 restatement.  p,
    m and v are compared with the restatement rounded to float32, their storage format: (1 - b2) g^2 of a clipped 1e-30 is not a
    float32 number."""
    from dual_dmp_amd import ops
    p0, p, m, v = _state(n, dev)
    rp, rm, rv = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        g = X.optimizer_gradient(kind, n, step)
        gd = g.to(dev)
        ss = ops.grad_sumsq(gd)
        want = float((g.double() ** 2).sum())
        assert abs(float(ss) - want) <= 1e-12 * want, (float(ss), want)
        rp, rm, rv, rg = X.clip_adam_f64(rp, rm, rv, g, step)
        g2 = gd.clone()
        ops.grad_clip_(g2, ss, X.MAX_NORM)
        ops.adam_step_(p, gd, m, v, X.LR, step, clip_sumsq=ss, max_norm=X.MAX_NORM)
        errs = [relerr(g2, rg.float())] + [relerr(a, b.float()) for a, b in ((p, rp), (m, rm), (v, rv))]
        print("%s n=%d step %d: rel-L2 clipped g %.2e, p %.2e, m %.2e, v %.2e (tolerance 1e-6)" % ((kind, n, step) + tuple(errs)))
        for a in (g2, p, m, v):
            assert bool(torch.isfinite(a).all())
        assert max(errs) < 1e-6, errs


def _prepare(ops, dev, start, times):
    counter = torch.tensor([start], dtype=torch.int32, device=dev)
    coef = torch.full((2,), float("nan"), device=dev)
    out = []
    for _ in range(times):
        ops.adam_prepare(counter, X.LR, coef)
        out.append((int(counter.item()), coef.cpu().double().numpy().copy()))
    return out


@pytest.mark.parametrize("start,times", [(0, 5), (999, 1), (99999, 1)])
def test_device_step_counter_and_coefficients(dev, start, times):
    """``adam_prepare``: ++counter, coef = (lr / (1 - b1^t), sqrt(1 - b2^t)) of the NEW count, within 2 float32 ulps of the float64
    value from the float32 lr and betas; ``adam_step_dev_`` with them against ``adam_step_`` at the same step."""
    from dual_dmp_amd import ops
    n = 65537
    for i, (t, coef) in enumerate(_prepare(ops, dev, start, times)):
        assert t == start + i + 1
        want = np.array(X.adam_coefficients(t))
        over = np.abs(coef - want) / ulp32(want)
        print("t=%d: coef %r, float64 %r, off by %s float32 ulps" % (t, coef.tolist(), want.tolist(), over.tolist()))
        assert np.all(np.isfinite(coef)) and np.all(over <= 2.0)
    # the same step through both entry points, from a state two ordinary steps old
    for t, coef in _prepare(ops, dev, start, times):
        _, p, m, v = _state(n, dev)
        for s in (1, 2):
            ops.adam_step_(p, X.optimizer_gradient("below", n, s).to(dev), m, v, X.LR, s)
        g = (X.optimizer_gradient("below", n, 3) * 8).to(dev)           # norm 1.6 .. 3.2: clipped
        ss = ops.grad_sumsq(g)
        a, b = [p.clone(), m.clone(), v.clone()], [p.clone(), m.clone(), v.clone()]
        ops.adam_step_(a[0], g, a[1], a[2], X.LR, t, clip_sumsq=ss, max_norm=X.MAX_NORM)
        ops.adam_step_dev_(b[0], g, b[1], b[2], torch.tensor(coef, dtype=torch.float32, device=dev), clip_sumsq=ss,
                           max_norm=X.MAX_NORM)
        errs = [relerr(y, x) for x, y in zip(a, b)]
        host = np.array(X.adam_coefficients(t)).astype(np.float32).astype(np.float64)  # (the host's own rounding of the same two)
        same = bool(np.array_equal(host, coef))
        print("t=%d: adam_step_dev_ against adam_step_ rel-L2 p %.2e m %.2e v %.2e; coefficient pairs %s"
              % (t, errs[0], errs[1], errs[2], "identical" if same else "differ"))
        assert max(errs) <= 2e-7, errs
        assert not torch.equal(a[0], p)
        if same:
            assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 4. tiny and edgeless graphs
def _path(n):
    """edge_index of the path 0 - 1 - ... - (n - 1), both directions: the end nodes have degree 1; n = 1: no edge at all."""
    i = torch.arange(n - 1, dtype=torch.int64)
    return torch.stack([torch.cat([i, i + 1]), torch.cat([i + 1, i])]).contiguous()


CIN, COUT, HEADS, DIM = 5, 4, 2, 2


def _gmm(loops):
    from dual_dmp_amd.nn_ops import GMMConv
    conv = GMMConv(CIN, COUT, DIM, 3)
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():                                        # (as test_gpu_gmm.py redraws them: mu in the unit cube, sigma of order 1)
        conv.mu.copy_(torch.rand(conv.mu.shape, generator=gen))
        conv.sigma.copy_(0.3 + 0.7 * torch.rand(conv.sigma.shape, generator=gen))
    return conv


def _gcn_ref(conv, loops, dtype):
    from gcnw_ref import GCNConvRef
    ref = GCNConvRef(CIN, COUT, add_self_loops=loops).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in conv.state_dict().items()})
    return ref


def _drop_ins():
    """name -> dict(make(loops) -> the drop-in on the CPU, ref(conv, loops, dtype) -> its reference, width of y, loops: has the
    add_self_loops option, extra: None | "attr" (pseudo-coordinates, with a gradient when ``dattr``) | "weight" (edge weights),
    yard: the gradients the operator's own test file holds to the yardstick bound instead of OP_TOL)."""
    from dual_dmp_amd import nn_ops as N
    import edgeconv_ref, feast_ref, gat_ref, gatv2_ref, gmm_ref, resgated_ref, spline_ref, transformer_ref
    T = {}
    T["gat"] = dict(make=lambda lp: N.GATConv(CIN, COUT, heads=HEADS, add_self_loops=lp), width=HEADS * COUT, loops=True,
                    ref=lambda c, lp, dt: gat_ref.GATConvRef(CIN, COUT, HEADS, True, 0.2, lp, dtype=dt).load_from(c),
                    yard=("d att_src", "d att_dst"))
    T["gatv2"] = dict(make=lambda lp: N.GATv2Conv(CIN, COUT, heads=HEADS, add_self_loops=lp), width=HEADS * COUT, loops=True,
                      ref=lambda c, lp, dt: gatv2_ref.GATv2ConvRef(CIN, COUT, HEADS, True, 0.2, lp, dtype=dt).load_from(c),
                      yard=("d att",))
    T["transformer"] = dict(make=lambda lp: N.TransformerConv(CIN, COUT, heads=HEADS), width=HEADS * COUT,
                            ref=lambda c, lp, dt: transformer_ref.TransformerConvRef(CIN, COUT, HEADS, dtype=dt).load_from(c))
    T["resgated"] = dict(make=lambda lp: N.ResGatedGraphConv(CIN, COUT),
                         ref=lambda c, lp, dt: resgated_ref.ResGatedGraphConvRef(CIN, COUT, dtype=dt).load_from(c))
    T["feast"] = dict(make=lambda lp: N.FeaStConv(CIN, COUT, heads=HEADS, add_self_loops=lp), loops=True,
                      ref=lambda c, lp, dt: feast_ref.FeaStConvRef(CIN, COUT, HEADS, lp, dtype=dt).load_from(c),
                      yard=("d u.weight", "d c"))
    T["edgeconv"] = dict(make=lambda lp: N.EdgeConv(torch.nn.Linear(2 * CIN, COUT)),
                         ref=lambda c, lp, dt: edgeconv_ref.EdgeConvRef(c.nn, dtype=dt))
    T["gmm"] = dict(make=_gmm, extra="attr", dattr=True, yard=("d attr", "d mu", "d sigma"),
                    ref=lambda c, lp, dt: gmm_ref.GMMConvRef(CIN, COUT, DIM, 3, dtype=dt).load_from(c))
    T["spline"] = dict(make=lambda lp: N.SplineConv(CIN, COUT, DIM, 3), extra="attr",
                       ref=lambda c, lp, dt: spline_ref.SplineConvRef(CIN, COUT, DIM, 3, dtype=dt).load_from(c))
    T["gcn-valued"] = dict(make=lambda lp: N.GCNConv(CIN, COUT, add_self_loops=lp), loops=True, extra="weight", ref=_gcn_ref)
    return T


DROP_INS = ("gat", "gatv2", "transformer", "resgated", "feast", "edgeconv", "gmm", "spline", "gcn-valued")
# zero in exact arithmetic, measured against its sibling's norm: see test_gpu_transformer.py
SIBLING = {"d lin_key.bias": "d lin_query.bias"}


def _dropin_run(conv, spec, x, ei, extra, t):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    args = []
    if extra is not None:
        extra = extra.clone().requires_grad_(spec.get("extra") == "weight" or bool(spec.get("dattr")))
        args.append(extra)
    y = conv(x, ei, *args)
    (y * t).sum().backward()
    out = dict([("y", y.detach()), ("dx", x.grad)] + [("d " + k, p.grad) for k, p in conv.named_parameters()])
    if extra is not None and extra.requires_grad:
        out["d " + spec["extra"]] = extra.grad
    return out


def _dropin_operands(spec, n, ei, dtype_seed):
    gen = torch.Generator().manual_seed(17 * n + dtype_seed)
    x, t = torch.randn(n, CIN, generator=gen), torch.randn(n, spec.get("width", COUT), generator=gen)
    extra = None
    if spec.get("extra") == "attr":
        extra = torch.rand(ei.shape[1], DIM, generator=gen)
    elif spec.get("extra") == "weight":
        extra = torch.rand(ei.shape[1], generator=gen) + 0.25
    return x, t, extra


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("name", DROP_INS)
def test_drop_ins_on_a_path_graph(dev, name, n):
    """n < 64: one partly filled chunk, seven of the eight launched workgroups return; the end nodes have degree 1 -- a softmax
    over a single entry where no self loop is added.  n = 1 has no edge: with the self loop an operator adds it is a one-entry
    graph, without one it is refused (test_an_edgeless_graph_is_refused)."""
    spec = _drop_ins()[name]
    loops = bool(spec.get("loops"))
    ei = _path(n)
    torch.manual_seed(n)
    conv = spec["make"](loops)
    bias = getattr(conv, "bias", None)
    if bias is not None:
        with torch.no_grad():
            bias.uniform_(-0.5, 0.5)                             # (zeros at initialisation: give it something to add)
    x, t, extra = _dropin_operands(spec, n, ei, 0)
    if n == 1 and not loops:
        with pytest.raises(ValueError, match="no edge"):
            _dropin_run(conv.to(dev), spec, x.to(dev), ei.to(dev), None if extra is None else extra.to(dev), t.to(dev))
        return
    r64, r32 = (_dropin_run(spec["ref"](conv, loops, dt), spec, x.to(dt), ei, None if extra is None else extra.to(dt), t.to(dt))
                for dt in (torch.float64, torch.float32))
    conv.to(dev)
    got = _dropin_run(conv, spec, x.to(dev), ei.to(dev), None if extra is None else extra.to(dev), t.to(dev))
    assert sorted(got) == sorted(r64)
    bad = []
    for k in got:
        assert got[k] is not None and got[k].shape == r64[k].shape and bool(torch.isfinite(got[k]).all()), k
        den = float(r64[SIBLING.get(k, k)].double().norm()) + 1e-30
        e = float((got[k].double().cpu() - r64[k]).norm()) / den
        yard = float((r32[k].double() - r64[k]).norm()) / den
        lim = bound(yard) if k in spec.get("yard", ()) else X.OP_TOL
        print("%s path n=%d %s: rel-L2 %.2e, float32 CPU %.2e, limit %.2e" % (name, n, k, e, yard, lim))
        if not e <= lim:
            bad.append((k, e, yard, lim))
    assert not bad, bad


@pytest.mark.parametrize("name", DROP_INS)
def test_an_edgeless_graph_is_refused(dev, name):
    """Five nodes and an empty edge_index, without added self loops where the operator has the option: PyG gives the root / skip /
    bias term alone; every drop-in here refuses with ValueError before any launch, not with a status from inside
    the library over the null pointer of an empty per-entry array."""
    from dual_dmp_amd import ops
    spec = _drop_ins()[name]
    n, ei = 5, torch.empty((2, 0), dtype=torch.int64)
    torch.manual_seed(5)
    conv = spec["make"](False).to(dev)
    x, t, extra = _dropin_operands(spec, n, ei, 1)
    with pytest.raises(ValueError, match="no edge"):
        _dropin_run(conv, spec, x.to(dev), ei.to(dev), None if extra is None else extra.to(dev), t.to(dev))
    if name == "gat":                                            # the kernel-level calls refuse the graph itself
        g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
        assert g.nnz == 0
        hf = torch.randn(n, HEADS * COUT, device=dev)
        s = torch.zeros(n, HEADS, device=dev)
        with pytest.raises(ValueError, match="no entry"):
            ops.gat_fwd(g, hf, s, s.clone(), HEADS, 0.2)


# ------------------------------------------------------------------------------------------------ 5. head softmax (feast.hip)
@pytest.mark.parametrize("family", X.FEAST_FAMILIES)
@pytest.mark.parametrize("name,loops", X.FEAST_GRAPHS)
@pytest.mark.parametrize("C,heads", X.FEAST_WIDTHS)
def test_head_softmax_at_extreme_logits(dev, graphs, family, name, loops, C, heads):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    hc = heads * C
    o = X.feast_operands(family, n, C, heads)
    ref, rows, aux = X.feast_reference(o, ei, n, heads, loops, torch.float64)
    r32, _, _ = X.feast_reference(o, ei, n, heads, loops, torch.float32)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=loops)
    assert g.nnz == len(rows)
    d = {k: v.to(dev) for k, v in o.items()}
    got = {}
    got["y"], got["beta"] = ops.feast_fwd(g, d["hf"], d["p"], d["c"], heads, bias=d["bias"])
    got["dz"], got["rs"] = ops.feast_bwd_edge(g, d["dout"], d["hf"], got["beta"], heads)
    got["dhf"], got["dp"] = ops.feast_bwd_node(g, d["dout"], got["beta"], got["dz"], got["rs"], heads)
    got["dc"] = ops.feast_dc(got["rs"], heads)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in got.items()}
    assert sorted(got) == sorted(ref)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    # each non-empty row's beta sums to 1 over its entries and heads, the empty row has none and gets the bias
    sums = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, got["beta"].double().sum(1))
    empty = torch.from_numpy(np.bincount(rows.numpy(), minlength=n) == 0)
    assert bool(empty.any()) == name.endswith("-iso")
    assert float((sums[~empty] - 1).abs().max()) < 1e-5
    if empty.any():
        assert float(sums[empty].abs().max()) == 0.0 and torch.equal(got["y"][empty], o["bias"].expand(int(empty.sum()), -1))
    if family == "flat":                                         # beta = mult / (deg heads)
        mult = X.multiplicities(ei, n, loops)
        share = (mult / torch.zeros(n, dtype=torch.float64).index_add_(0, rows, mult)[rows] / heads).unsqueeze(1).expand(-1, heads)
        over = ((got["beta"].double() - share).abs().numpy() / ulp32(share.numpy())).max()
        print("feast flat %s C=%d heads=%d: beta within %.2f float32 ulps of mult / (deg heads)" % (name, C, heads, over))
        assert over <= 2.0
    bad = []
    for k in ref:
        e, yard = relerr(got[k], ref[k]), relerr(r32[k], ref[k])
        print("feast %s %s C=%d heads=%d %s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e"
              % (family, name, C, heads, k, e, yard, bound(yard)))
        if not e <= bound(yard):
            bad.append((k, e, yard))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 6. Gaussian mixture (gmm.hip)
@pytest.mark.parametrize("family", X.GMM_FAMILIES)
@pytest.mark.parametrize("C,K,dim", X.GMM_WIDTHS)
@pytest.mark.parametrize("root", [True, False])
def test_gaussian_mixture_at_extreme_sigma_and_mu(dev, graphs, family, C, K, dim, root):
    from dual_dmp_amd import ops
    ei, n = graphs[X.GMM_GRAPH]
    kd = K * dim
    o = X.gmm_operands(family, n, ei.shape[1], C, K, dim)
    ref, rows, aux = X.gmm_reference(o, ei, n, K, torch.float64, root)
    r32, _, _ = X.gmm_reference(o, ei, n, K, torch.float32, root)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    assert g.nnz == len(rows) and g.nnz_in == ei.shape[1]
    d = {k: v.to(dev) for k, v in o.items()}
    got = {}
    got["y"], got["w"] = ops.gmm_fwd(g, d["hf"], d["attr"], d["mu"], d["sigma"], K, root=d["r"] if root else None, bias=d["bias"])
    parts, got["dattr"] = ops.gmm_bwd_edge(g, d["dout"], d["hf"], d["attr"], d["mu"], d["sigma"], K, want_dattr=True)
    got["dhf"], dr = ops.gmm_bwd_node(g, d["dout"], got["w"], K, root=root)
    if root:
        got["dr"] = dr
    dms = ops.feast_dc(parts, 2 * kd)
    got["dmu"], got["dsigma"] = dms[:kd].view(K, dim), dms[kd:].view(K, dim)
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in got.items()}
    assert sorted(got) == sorted(ref)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
    # rows whose weights all underflow (and the edgeless row) hold exactly root + bias
    live = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, got["w"].double().abs().sum(1)) > 0
    init = (o["r"] + o["bias"]) if root else o["bias"].expand(n, -1)
    print("gmm %s C=%d K=%d dim=%d: %d of %d rows keep no Gaussian" % (family, C, K, dim, int((~live).sum()), n))
    assert torch.equal(got["y"][~live], init[~live])
    if family == "tiny-sigma":
        assert int((~live).sum()) > n // 20 and bool(live.any())
    if family == "far-mu":
        assert not live.any() and not got["dmu"].any() and not got["dsigma"].any() and not got["dattr"].any()
    bad = []
    for k in ref:
        e, yard = relerr(got[k], ref[k]), relerr(r32[k], ref[k])
        print("gmm %s C=%d K=%d dim=%d root=%s %s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e"
              % (family, C, K, dim, root, k, e, yard, bound(yard)))
        if not e <= bound(yard):
            bad.append((k, e, yard))
    assert not bad, bad

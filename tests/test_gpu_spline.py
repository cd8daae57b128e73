"""SplineConv on the GPU: the two B-spline launches (basis + block gather, the node-side backward) and the drop-in against the
float64 edge-list reference (tests/spline_ref.py) on the icosphere (ragged last chunk), the open grid (boundary) and the hub graph
(one 1200-entry row), with duplicate edges and explicit loops on top, and with one edgeless node.

Inputs: pseudo-coordinates uniform in [0, 1]^dim per input edge (so the duplicated edges carry different ones); the first rows sit
exactly on 0, on 1 and on interior knots.  The kernels round v = a (kernel_size - open) to float32 before the floor, the reference
works in float64 on the same float32 pseudo-coordinates: next to a knot the two may pick neighbouring block pairs, with weights
that differ by the rounding of v -- the degree-1 basis is continuous, so this is inside the tolerance.

Tolerance policy: every comparison against ``SplineConvRef`` / ``spline_basis`` in float64 is at the project's operator tolerance,
rel-L2 <= 1e-5 (y, dHf, dx, dweight, dlin, db); the training test's loss and whole-gradient figures have no project tolerance and
use the yardstick of test_gpu_gat.py: 4x the float32 CPU reference's own distance from float64, not below its FLOOR."""
import math

import numpy as np
import pytest
import torch

import oracle_jobs as OJ
from spline_ref import SplineConvRef, sizes, spline_basis
from test_gpu_gat import OP_TOL, bound, dev, entry_map, graphs, relerr  # noqa: F401  (dev, graphs: the fixtures)

pytestmark = pytest.mark.gpu

# (C, dim, kernel_size, open): the scalar path, one / two / eight lanes per block, a ragged q loop, a wide block, S = 32, K = 1
KCASES = [(3, 1, 3, True), (4, 2, (2, 3), (True, False)), (8, 3, 2, True), (40, 3, 3, False), (64, 3, 5, True), (16, 5, 2, True),
          (8, 2, 1, True)]


def draw_attr(gen, E, dim):
    """[E, dim] float32 in [0, 1]; rows 0 .. 8 exactly on 0, 1 and knots (1/2, 1/4, 3/4: knots of kernel_size 3 and 5 open, of 2 and
    4 closed; 1/3, 2/3: of 3 closed and 4 open), row 7 alternating 0 / 1 per coordinate, row 8 the reverse."""
    a = torch.rand(E, dim, generator=gen)
    for r, v in enumerate((0.0, 1.0, 0.5, 0.25, 0.75, 1.0 / 3.0, 2.0 / 3.0)):
        a[r] = v
    a[7] = torch.arange(dim) % 2
    a[8] = 1 - a[7]
    return a


def kernel_reference(hf, r, attr, bias, dout, ei, n, ks, op, mean, dtype=torch.float64):
    """y and dHf of the two launches from ``spline_basis`` in ``dtype`` with Hf as the (differentiable) input."""
    K = math.prod(ks)
    C = hf.shape[1] // K
    x = hf.to(dtype).requires_grad_(True)
    b, k = spline_basis(attr.to(dtype), ks, op)
    src, dst = ei[0], ei[1]
    msg = (b.unsqueeze(-1) * x.view(n, K, C)[src.unsqueeze(1), k]).sum(1)
    y = torch.zeros((n, C), dtype=dtype).index_add_(0, dst, msg)
    cnt = torch.zeros(n, dtype=dtype).index_add_(0, dst, torch.ones(len(dst), dtype=dtype))
    if mean:
        y = y / cnt.clamp(min=1.0).unsqueeze(1)
    y = y + r.to(dtype) + bias.to(dtype)
    (y * dout.to(dtype)).sum().backward()
    return y.detach(), x.grad, k, cnt


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("name", ["ico", "grid", "hub", "grid-iso", "hub-iso"])
@pytest.mark.parametrize("C,dim,ks,op", KCASES)
@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_kernels_match_the_reference(dev, graphs, name, C, dim, ks, op, aggr):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    ks, op = sizes(dim, ks, op)
    K, mean = math.prod(ks), aggr == "mean"
    hc = K * C
    gen = torch.Generator().manual_seed(n + C)
    hf, r = torch.randn(n, hc, generator=gen), torch.randn(n, C, generator=gen)
    bias, dout = torch.randn(C, generator=gen), torch.randn(n, C, generator=gen)
    attr = draw_attr(gen, ei.shape[1], dim)
    assert not torch.equal(attr[9:50], attr[-100 + 9:-50])       # the duplicated edges carry other pseudo-coordinates
    y_ref, dhf_ref, k64, cnt = kernel_reference(hf, r, attr, bias, dout, ei, n, ks, op, mean)
    eid = ei.to(dev)
    g = ops.graph_for(eid, n, norm="gat", add_self_loops=False)
    _, rows, _ = entry_map(ei, n, False, ei[0], ei[1])
    assert g.nnz == len(rows) and g.nnz_in == ei.shape[1]
    wt = hc + C
    wtp = (wt + 3) // 4 * 4                                       # the operator's layout: one row buffer [Hf | R | padding]
    buf = torch.zeros(n, wtp, device=dev)
    buf[:, :hc], buf[:, hc:wt] = hf.to(dev), r.to(dev)
    hfd, rd, doutd, ad, bd = buf[:, :hc], buf[:, hc:wt], dout.to(dev), attr.to(dev), bias.to(dev)
    y = ops.spline_fwd(g, hfd, ad, ks, op, root=rd, bias=bd, mean=mean)
    gbuf = torch.full((n, wtp), float("nan"), device=dev)
    dhf, dr = ops.spline_bwd_node(g, doutd, ad, ks, op, C, mean=mean, out=gbuf, root=True)
    # the variants: no root, no bias
    y0 = ops.spline_fwd(g, hfd, ad, ks, op, mean=mean)
    gbuf0 = torch.full((n, wtp), float("nan"), device=dev)
    dhf0, none = ops.spline_bwd_node(g, doutd, ad, ks, op, C, mean=mean, out=gbuf0)
    torch.cuda.synchronize()
    assert y.shape == (n, C) and dhf.shape == (n, hc) and dr.shape == (n, C) and none is None
    assert torch.equal(dhf0, dhf) and bool(torch.isnan(gbuf0[:, hc:]).all())
    # padding columns untouched, the root block a bitwise copy of dOut
    assert bool(torch.isnan(gbuf[:, wt:]).all()) and bool(torch.isfinite(gbuf[:, :wt]).all())
    assert torch.equal(dr, doutd)
    # an edgeless row: R[i] + bias bit for bit, a zero gradient row
    empty = cnt == 0
    assert bool(empty.any()) == name.endswith("-iso")
    if empty.any():
        assert torch.equal(y.cpu()[empty], r[empty] + bias)
        assert torch.equal(y0.cpu()[empty], torch.zeros(int(empty.sum()), C))
        assert bool((dhf.cpu()[empty] == 0).all())
    # blocks that no edge of the node selects -- neither with v rounded to float32 nor in float64 -- are exactly zero
    _, k32 = spline_basis(attr, ks, op)
    sel = torch.zeros(n * K, dtype=torch.bool)
    for k in (k64, k32):
        sel[(ei[0].unsqueeze(1) * K + k).reshape(-1)] = True
    blocks = dhf.cpu().view(n * K, C)
    assert bool((blocks[~sel] == 0).all())
    if K > 1 << dim:
        assert int((~sel).sum()) > 0
    for key, got, ref in (("y", y, y_ref), ("dhf", dhf, dhf_ref), ("y without root and bias", y0, y_ref - r.double() - bias.double())):
        e = relerr(got, ref)
        print("%s C=%d dim=%d kernel_size=%s open=%s %s %s: rel-L2 %.2e (tolerance %.0e)" % (name, C, dim, ks, op, aggr, key, e, OP_TOL))
        assert e <= OP_TOL, (key, e)


def test_pseudo_coordinates_outside_the_unit_cube_stay_in_bounds(dev, graphs):
    """Negative, > 1, huge, infinite and NaN pseudo-coordinates: the block indices stay inside the neighbour's row, so the rows whose
    edges are all regular keep their bits and nothing outside the buffers is touched (the results of the others are unspecified)."""
    from dual_dmp_amd import ops
    ei, n = graphs["grid"]
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    gen = torch.Generator().manual_seed(2)
    C, ks, op = 8, [3, 2], [True, False]
    hf, dout = torch.randn(n, 6 * C, generator=gen).to(dev), torch.randn(n, C, generator=gen).to(dev)
    attr = torch.rand(ei.shape[1], 2, generator=gen)
    y1 = ops.spline_fwd(g, hf, attr.to(dev), ks, op)
    d1, _ = ops.spline_bwd_node(g, dout, attr.to(dev), ks, op, C)
    bad = attr.clone()
    odd = torch.tensor([-0.3, 1.7, -5.0, 1e30, -1e30, float("inf"), -float("inf"), float("nan")])
    hit = torch.arange(len(odd)) * 3
    bad[hit, 0], bad[hit + 1, 1] = odd, odd
    guard = torch.full((n + 2, 6 * C), 7.0, device=dev)
    y2 = ops.spline_fwd(g, hf, bad.to(dev), ks, op)
    d2, _ = ops.spline_bwd_node(g, dout, bad.to(dev), ks, op, C, out=guard[1:n + 1])
    torch.cuda.synchronize()
    touched = torch.cat([hit, hit + 1])
    clean_t = torch.ones(n, dtype=torch.bool)
    clean_t[ei[1][touched]] = False
    clean_s = torch.ones(n, dtype=torch.bool)
    clean_s[ei[0][touched]] = False
    assert int(clean_t.sum()) > n // 2 and int(clean_s.sum()) > n // 2
    assert torch.equal(y2.cpu()[clean_t], y1.cpu()[clean_t]) and torch.equal(d2.cpu()[clean_s], d1.cpu()[clean_s])
    assert bool((guard[0] == 7.0).all()) and bool((guard[n + 1] == 7.0).all())


# ------------------------------------------------------------------------------------------------ 2. column blocks, aliasing
@pytest.mark.parametrize("C,dim,ks,op", [(8, 2, (2, 3), (True, False)), (3, 1, 3, True), (40, 3, 3, False)])
def test_column_blocks_of_one_row_buffer(dev, graphs, C, dim, ks, op):
    """Hf and R as column blocks of a packed [Hf | R | padding] buffer, y into a column block of a wider buffer and [dHf | dR] into
    the leading columns of a NaN-prefilled one give the bits of the contiguous calls.  The buffers' widths are multiples of 4, as
    the operator's are: a row stride that is not takes the scalar kernels, whose sums run in another order."""
    from dual_dmp_amd import ops
    ei, n = graphs["ico-iso"]
    ks, op = sizes(dim, ks, op)
    K = math.prod(ks)
    hc = K * C
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(3)
    wide = (hc + C + 3) // 4 * 4 + 4
    buf, dout, bias = torch.randn(n, wide, device=dev), torch.randn(n, C, device=dev), torch.randn(C, device=dev)
    attr = torch.rand(ei.shape[1], dim, device=dev)
    hf, r = buf[:, :hc], buf[:, hc:hc + C]
    chf, cr = hf.contiguous(), r.contiguous()
    ybuf = torch.full((n, 2 * C + 4), float("nan"), device=dev)
    for mean in (True, False):
        y = ops.spline_fwd(g, hf, attr, ks, op, root=r, bias=bias, mean=mean, out=ybuf[:, C:2 * C])
        assert y.data_ptr() == ybuf[:, C:].data_ptr()
        assert torch.equal(y, ops.spline_fwd(g, chf, attr, ks, op, root=cr, bias=bias, mean=mean))
        assert bool(torch.isnan(ybuf[:, :C]).all()) and bool(torch.isnan(ybuf[:, 2 * C:]).all())
        gbuf = torch.full((n, wide), float("nan"), device=dev)
        dhf, dr = ops.spline_bwd_node(g, dout, attr, ks, op, C, mean=mean, out=gbuf, root=True)
        dhf2, dr2 = ops.spline_bwd_node(g, dout, attr, ks, op, C, mean=mean, root=True)
        dhf3, none = ops.spline_bwd_node(g, dout, attr, ks, op, C, mean=mean)
        assert dhf.data_ptr() == gbuf.data_ptr() and dr.data_ptr() == gbuf[:, hc:].data_ptr() and none is None
        assert torch.equal(dhf, dhf2) and torch.equal(dhf, dhf3) and torch.equal(dr, dout) and torch.equal(dr2, dout)
        assert bool(torch.isnan(gbuf[:, hc + C:]).all())


def test_aliasing_and_bad_arguments_raise(dev, graphs):
    from dual_dmp_amd import ops
    ei, n = graphs["grid"]
    eid = ei.to(dev)
    g = ops.graph_for(eid, n, norm="gat", add_self_loops=False)
    C = 8
    hf1, r, dout = (torch.randn(n, C, device=dev) for _ in range(3))
    attr = torch.rand(ei.shape[1], 2, device=dev)
    one, opn = [1, 1], [True, True]                              # K = 1: Hf is [n, C], so it can be offered as the output
    ops.spline_fwd(g, hf1, attr, one, opn, root=r)
    for t in (hf1, r):
        with pytest.raises(ops.DdmpError):
            ops.spline_fwd(g, hf1, attr, one, opn, root=r, out=t)
    with pytest.raises(ops.DdmpError):
        ops.spline_bwd_node(g, dout, attr, one, opn, C, out=dout)                       # dHf is dOut
    gb = torch.randn(n, 2 * C, device=dev)
    with pytest.raises(ops.DdmpError):
        ops.spline_bwd_node(g, gb[:, C:], attr, one, opn, C, out=gb, root=True)         # dR is dOut
    hf = torch.randn(n, 6 * C, device=dev)
    with pytest.raises(ops.DdmpError):
        ops.spline_fwd(ops.graph_for(eid, n), hf, attr, [2, 3], opn)                    # an unvalued graph
    with pytest.raises(ops.DdmpError):
        ops.spline_fwd(ops.graph_for(eid, n, norm="gat"), hf, attr, [2, 3], opn)        # the attention graph WITH loop handling
    with pytest.raises(ops.DdmpError):
        ops.spline_fwd(g, hf, attr[:-1], [2, 3], opn)            # not one row per input edge
    with pytest.raises(ops.DdmpError):
        ops.spline_fwd(g, hf, attr, [2, 3, 1], [True] * 3)       # kernel_size longer than dim
    with pytest.raises(ops.DdmpError):
        ops.spline_fwd(g, hf, attr, [5, 2], opn)                 # 48 columns are not 10 blocks
    with pytest.raises(ops.DdmpError):
        ops.spline_fwd(g, hf, torch.rand(ei.shape[1], 6, device=dev), [1] * 6, [True] * 6)      # dim > 5
    with pytest.raises(ops.DdmpError):
        ops.spline_bwd_node(g, torch.randn(n, 3, device=dev), attr, [2, 3], opn, C)
    with pytest.raises(ops.DdmpError):
        ops.spline_fwd(g, hf, attr.cpu(), [2, 3], opn)


# ------------------------------------------------------------------------------------------------ 3. the operator
PNAMES = ("weight", "lin.weight", "bias")
# (in, out, dim, kernel_size, open)
OCASES = [(3, 3, 1, 3, True), (16, 4, 2, (2, 3), (True, False)), (8, 8, 3, 2, True), (32, 40, 3, 3, False), (16, 64, 3, 5, True)]


def _named(conv):
    have = dict(conv.named_parameters())
    return [(k, have[k]) for k in PNAMES if k in have]


def _operator_run(conv, x, ei, attr, t):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, ei, attr)
    (y * t).sum().backward()
    return dict([("y", y.detach()), ("dx", x.grad)] + [("d " + k, p.grad) for k, p in _named(conv)])


@pytest.mark.parametrize("cin,cout,dim,ks,op", OCASES)
@pytest.mark.parametrize("gname", ["hub", "ico-iso"])
@pytest.mark.parametrize("root", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_operator_matches_the_float64_reference(dev, graphs, cin, cout, dim, ks, op, gname, root, bias, aggr):
    from dual_dmp_amd.nn_ops import SplineConv
    ei, n = graphs[gname]
    torch.manual_seed(cin + cout)
    conv = SplineConv(cin, cout, dim, ks, is_open_spline=op, aggr=aggr, root_weight=root, bias=bias)
    if bias:
        with torch.no_grad():
            conv.bias.uniform_(-0.5, 0.5)                        # (zeros at initialisation: give it something to add)
    gen = torch.Generator().manual_seed(n)
    x, t = torch.randn(n, cin, generator=gen), torch.randn(n, cout, generator=gen)
    attr = draw_attr(gen, ei.shape[1], dim)
    refs = {dtype: SplineConvRef(cin, cout, dim, ks, op, aggr, root, bias, dtype=dtype).load_from(conv)
            for dtype in (torch.float64, torch.float32)}
    r64, r32 = (_operator_run(refs[dtype], x.to(dtype), ei, attr.to(dtype), t.to(dtype)) for dtype in (torch.float64, torch.float32))
    conv.to(dev)
    got = _operator_run(conv, x.to(dev), ei.to(dev), attr.to(dev), t.to(dev))
    assert list(got) == list(r64) and len(got) == 3 + (1 if root else 0) + (1 if bias else 0)
    assert all(v is not None for v in got.values())
    for key in got:
        assert got[key].shape == r64[key].shape, key
        e = relerr(got[key], r64[key])
        print("%s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)" % (key, e, OP_TOL, relerr(r32[key], r64[key])))
        assert e <= OP_TOL, (key, e)
    if gname == "ico-iso":                                       # the node without incoming edges: lin(x_i) + bias
        want = (x[-1].double() @ refs[torch.float64].lin.weight.t() if root else torch.zeros(cout, dtype=torch.float64))
        want = (want + (refs[torch.float64].bias if bias else 0.0)).detach()
        assert float((got["y"][-1].double().cpu() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))


def test_float64_pseudo_coordinates_frozen_parameters_and_device_refusals(dev, graphs):
    from dual_dmp_amd import ops
    from dual_dmp_amd.nn_ops import SplineConv
    ei, n = graphs["grid"]
    eid = ei.to(dev)
    torch.manual_seed(2)
    conv = SplineConv(8, 8, dim=2, kernel_size=3).to(dev)
    x, attr = torch.randn(n, 8, device=dev), torch.rand(ei.shape[1], 2, device=dev, dtype=torch.float64)
    assert torch.equal(conv(x, eid, attr), conv(x, eid, attr.float()))                  # rounded once
    conv.lin.weight.requires_grad_(False)
    conv(x, eid, attr).sum().backward()
    assert x.grad is None and conv.lin.weight.grad is None and conv.weight.grad is not None and conv.bias.grad is not None
    with pytest.raises(ops.DdmpError):
        conv(x, eid, attr.cpu())                                 # pseudo-coordinates left on the host
    with pytest.raises(ValueError):
        conv(x, eid, attr.clone().requires_grad_(True))
    with pytest.raises(ValueError):                              # a non-symmetric structure (2 -> 0 without 0 -> 2): the valued graph's own error
        conv(x[:3], torch.tensor([[0, 1, 2], [1, 0, 0]], device=dev), attr[:3])


# ------------------------------------------------------------------------------------------------ 4. reproducibility
def test_two_runs_give_the_same_bits(dev, graphs):
    from dual_dmp_amd.nn_ops import SplineConv
    ei, n = graphs["hub"]
    eid = ei.to(dev)
    for cin, cout, dim, ks, op in OCASES + [(8, 16, 5, 2, True), (8, 8, 2, 1, True)]:
        for aggr in ("mean", "add"):
            torch.manual_seed(1)
            conv = SplineConv(cin, cout, dim, ks, is_open_spline=op, aggr=aggr).to(dev)
            x, t = torch.randn(n, cin, device=dev), torch.randn(n, cout, device=dev)
            attr = torch.rand(ei.shape[1], dim, device=dev)
            a = {k: v.clone() for k, v in _operator_run(conv, x, eid, attr, t).items()}
            b = _operator_run(conv, x, eid, attr, t)
            for k in a:
                assert torch.equal(a[k], b[k]), (cin, cout, dim, ks, aggr, k)


# ------------------------------------------------------------------------------------------------ 5. training
class _TwoLayer(torch.nn.Module):
    def __init__(self, mk):
        super().__init__()
        self.c1, self.c2 = mk(8, 16), mk(16, 3)

    def forward(self, x, ei, attr):
        return self.c2(torch.relu(self.c1(x, ei, attr)), ei, attr)


def test_short_training_loop(dev, graphs):
    """10 Adam steps of a two-layer spline net (dim 3, kernel_size 3) regressing a fixed target on "ico": the loss falls; for the
    first 3 steps the loss and the full parameter gradient stay within the yardstick-derived bound of the float64 reference
    evaluated at the SAME parameters (teacher-forced: the reference is loaded from the GPU model before every compared step)."""
    from dual_dmp_amd.nn_ops import SplineConv
    ei, n = graphs["ico"]
    gen = torch.Generator().manual_seed(4)
    x, target = torch.randn(n, 8, generator=gen), torch.randn(n, 3, generator=gen)
    attr = torch.rand(ei.shape[1], 3, generator=gen)
    torch.manual_seed(4)
    net = _TwoLayer(lambda i, o: SplineConv(i, o, dim=3, kernel_size=3)).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    xd, td, eid, ad = x.to(dev), target.to(dev), ei.to(dev), attr.to(dev)
    cat = lambda m: torch.cat([p.grad.reshape(-1) for c in (m.c1, m.c2) for _, p in _named(c)])

    def ref_eval(dtype):
        r = _TwoLayer(lambda i, o: SplineConvRef(i, o, 3, 3, dtype=dtype))
        r.c1.load_from(net.c1), r.c2.load_from(net.c2)
        loss = ((r(x.to(dtype), ei, attr.to(dtype)) - target.to(dtype)) ** 2).mean()
        loss.backward()
        return float(loss.detach()), cat(r)

    losses = []
    for step in range(10):
        opt.zero_grad()
        loss = ((net(xd, eid, ad) - td) ** 2).mean()
        loss.backward()
        if step < 3:
            l64, g64 = ref_eval(torch.float64)
            l32, g32 = ref_eval(torch.float32)
            g = cat(net)
            el, yl = abs(float(loss.detach()) - l64) / l64, abs(l32 - l64) / l64
            eg, yg = relerr(g, g64), relerr(g32, g64)
            print("step %d: loss rel %.2e (yardstick %.2e, bound %.2e), gradient rel-L2 %.2e (yardstick %.2e, bound %.2e)"
                  % (step, el, yl, bound(yl), eg, yg, bound(yg)))
            assert el <= bound(yl) and eg <= bound(yg), (step, el, yl, eg, yg)
        opt.step()
        losses.append(float(loss.detach()))
    print("loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]


def test_adam_steps_of_the_modular_posnet(dev):
    """Two Adam steps of ``PosNet(dev, fused=False, conv="spline", K=2)`` on the icosphere, loss = mean squared distance to the
    clean vertices, the pseudo-coordinates ``cartesian_pseudo`` of the smoothed positions (cached on the dataset): finite, and
    decreasing."""
    from dual_dmp_amd.networks import PosNet
    from dual_dmp_amd.nn_ops import SplineConv
    gt, noisy, smooth, data = OJ.case("ico3")
    torch.manual_seed(6)
    net = PosNet(dev, fused=False, conv="spline", K=2)
    assert isinstance(net.conv7, SplineConv) and net.conv7.kernel_size == (2, 2, 2)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    td = torch.tensor(np.asarray(gt.vs), dtype=torch.float32, device=dev)
    losses = []
    for step in range(2):
        opt.zero_grad()
        loss = ((net(data) - td) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        for name, p in net.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        opt.step()
    print("loss %.6f -> %.6f" % tuple(losses))
    assert all(math.isfinite(v) for v in losses) and losses[1] < losses[0]
    cached = [v for k, v in data.__dict__["_ddmp_dev"].items() if k[0] == "cartesian:edge_attr"]
    assert len(cached) == 1 and cached[0][3].shape == (data.edge_index.shape[1], 3)


# ------------------------------------------------------------------------------------------------ 6. index width
def test_offsets_beyond_2_31_bytes(dev):
    """140,000-node vertex graph of a torus, kernel_size 5, dim 3, C = 32: Hf is [N, 4000] (+ the root block, in one row buffer) of
    N * 4000 * 4 bytes = 2.24e9 > 2^31, and [dHf | dR] is as large.  Forward and backward once; from the GPU's own Hf and R, y and
    the whole dHf row of 600 sampled rows (the last 10 among them) are recomputed in float64 on the CPU from their one-ring
    neighbourhoods and compared at the operator tolerance."""
    from dual_dmp_amd import ops, synth
    ks, op, C, cin, dim = [5, 5, 5], [True] * 3, 32, 16, 3
    K = 125
    hc = K * C
    v, f = synth.torus(400, 350)
    n = len(v)
    assert n == 140000 and n * hc * 4 > 2 ** 31
    f = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // n, key % n])).contiguous()
    t = ops.csr_build_valued_host(ei.numpy(), n, 0)
    rowptr, col, mirror = t["rowptr"].astype(np.int64), t["col"].astype(np.int64), t["mirror"].astype(np.int64)
    ee_ptr, ee_idx = t["ee_ptr"].astype(np.int64), t["ee_idx"].astype(np.int64)
    assert np.all(np.diff(ee_ptr) == 1)                           # no duplicate edges: one input edge per entry
    edge_of = ee_idx[ee_ptr[:-1]]
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(7)
    x, wgt = torch.randn(n, cin, device=dev), torch.randn(hc + C, cin, device=dev) * 0.3
    attr = torch.rand(ei.shape[1], dim, device=dev)
    buf = ops.gemm_nt(x, wgt)                                    # [N, 4032] = [Hf | R]
    hf, r = buf[:, :hc], buf[:, hc:]
    dout = torch.randn(n, C, device=dev)
    y = ops.spline_fwd(g, hf, attr, ks, op, root=r)
    gbuf = torch.empty(n, hc + C, device=dev)
    dhf, dr = ops.spline_bwd_node(g, dout, attr, ks, op, C, out=gbuf, root=True)
    torch.cuda.synchronize()
    # sampled rows, the last rows among them: the largest offsets
    rng = np.random.default_rng(0)
    s0 = np.unique(np.concatenate([rng.choice(n - 10, 590, replace=False), np.arange(n - 10, n)]))
    assert len(s0) == 600
    ent = np.concatenate([np.arange(rowptr[q], rowptr[q + 1]) for q in s0])
    cnt = rowptr[s0 + 1] - rowptr[s0]
    ecol = col[ent]
    i0 = torch.from_numpy(np.repeat(np.arange(len(s0)), cnt))
    dv = lambda q: torch.from_numpy(q).to(dev)
    fetch = lambda m, q: m[dv(q)].double().cpu()
    # y[i] = (1 / n_i) sum_{j in row i} sum_s b_{j -> i, s} Hf[j, k_{j -> i, s}] + R[i]   (only the selected blocks leave the GPU)
    b, k = spline_basis(fetch(attr, edge_of[ent]), ks, op)
    nb = hf[dv(ecol)].reshape(-1, K, C)                          # the neighbours' rows, gathered on the GPU
    blocks = nb[torch.arange(len(ecol), device=dev).unsqueeze(1), k.to(dev)].double().cpu()
    msg = (b.unsqueeze(-1) * blocks).sum(1)
    y_ref = torch.zeros((len(s0), C), dtype=torch.float64).index_add_(0, i0, msg) / torch.from_numpy(cnt).double().unsqueeze(1)
    y_ref = y_ref + fetch(r, s0)
    # dHf[j, k] = sum_{i in row j} sum_{s: k_{j -> i, s} = k} b_{j -> i, s} dOut[i] / n_i   (symmetric structure: row j lists its
    # targets; the edge j -> i belongs to the mirror entry)
    bt, kt = spline_basis(fetch(attr, edge_of[mirror[ent]]), ks, op)
    gi = fetch(dout, ecol) / torch.from_numpy(rowptr[ecol + 1] - rowptr[ecol]).double().unsqueeze(1)
    dh_ref = torch.zeros((len(s0) * K, C), dtype=torch.float64)
    for s in range(8):
        dh_ref.index_add_(0, i0 * K + kt[:, s], bt[:, s].unsqueeze(1) * gi)
    rows0 = dv(s0)
    e_y, e_d = relerr(y[rows0], y_ref), relerr(dhf[rows0].reshape(-1, C), dh_ref)
    print("140k nodes x (125 x 32): y rel-L2 %.2e, dHf rel-L2 %.2e over %d sampled rows (tolerance %.0e)" % (e_y, e_d, len(s0), OP_TOL))
    assert e_y <= OP_TOL and e_d <= OP_TOL
    assert torch.equal(dr[rows0], dout[rows0])

"""GATv2Conv on the GPU: the dynamic-attention kernels (per-edge scores + edge softmax + gather, the two backward launches, the
attention-vector reduction) and the drop-in against the float64 edge-list reference (tests/gatv2_ref.py) on the graphs of
test_gpu_gat.py: the icosphere (ragged last chunk), the open grid (boundary) and the hub graph (one 1200-entry row), with
duplicate edges and explicit loops on top, and the "-iso" variants for an empty row.

Tolerance policy (that of test_gpu_gat.py), every comparison against the float64 reference:
* y, dXl, dXr, dx, dW_l, dW_r, db and the lin bias gradients: the project's operator tolerance, rel-L2 <= 1e-5;
* alpha, dz and datt have no project tolerance: the yardstick is the float32 CPU evaluation of the same reference against its
  float64 evaluation on the same inputs, the bound 4x that and not below 16 float32 epsilons.  Both figures are printed.

THE KINK.  leaky' jumps at u = 0.  At kernel level Xl and Xr are given in float32 and u is ONE float32 addition, which has the
sign of the exact sum: nothing to handle.  At operator level the device's Xl / Xr come from a split-precision GEMM, so a u within
its rounding of zero can take the other branch than the float64 reference, and a single such term moves dW by far more than
1e-5.  The operator tests are therefore teacher-forced on the branch decisions: the device's [Xl | Xr] is recomputed through the
same ``ops.gemm_nt`` call (bitwise reproducible), ``pos = Xl[src] + Xr[dst] > 0`` is formed in float32 on the CPU and passed to
the reference as ``pos=``.  Asserted and printed for every case: (a) every term whose forced decision differs from the
reference's own has |u_ref| <= 64 float32 epsilons x (|x| |W_l|^T + |x| |W_r|^T); (b) such terms are <= 1e-4 of all terms."""
import numpy as np
import pytest
import torch

import edge_weight_route_worker as W
from gatv2_ref import GATv2ConvRef, gatv2_core, gatv2_edges
from test_gpu_gat import FLOOR, OP_TOL, bound, dev, entry_map, graphs  # noqa: F401  (dev, graphs: the fixtures)

pytestmark = pytest.mark.gpu
relerr = W.relerr
EPS = 2.0 ** -23

# (in, C per head, heads): scalar kernels | one lane per head | two lanes per head, last pass partly invalid | four lanes per
# head, last pass partly invalid | eight lanes per head | ragged q loop | wide head
CASES = [(3, 3, 2), (16, 4, 8), (8, 8, 3), (8, 16, 3), (8, 32, 1), (32, 40, 3), (64, 64, 4)]


# ------------------------------------------------------------------------------------------------ 1. the kernels
def kernel_reference(xl, xr, att, bias, dout, ei, n, heads, loops, dtype):
    """Everything the kernels produce, from the edge-list reference in ``dtype`` with Xl and Xr as the inputs."""
    xl, xr = xl.to(dtype).requires_grad_(True), xr.to(dtype).requires_grad_(True)
    a = att.to(dtype).requires_grad_(True)
    y, aux = gatv2_core(xl, xr, ei, a, bias.to(dtype), heads, True, 0.2, loops, full=True)
    (y * dout.to(dtype)).sum().backward()
    _, rows, ent = entry_map(ei, n, loops, aux["src"], aux["dst"])
    nnz = len(rows)
    alpha = torch.zeros((nnz, heads), dtype=dtype).index_add_(0, ent, aux["alpha"].detach())
    dz = torch.zeros((nnz, heads), dtype=dtype).index_add_(0, ent, aux["z"].grad)
    return dict(y=y.detach(), alpha=alpha, dz=dz, dxl=xl.grad, dxr=xr.grad, datt=a.grad.view(heads, -1)), rows


@pytest.mark.parametrize("name,loops", [("ico", True), ("grid", True), ("hub", True), ("grid-iso", False), ("hub-iso", False)])
@pytest.mark.parametrize("C,heads", [(c[1], c[2]) for c in CASES])
def test_kernels_match_the_reference(dev, graphs, name, loops, C, heads):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    gen = torch.Generator().manual_seed(n + C)
    hc = heads * C
    xl, xr = torch.randn(n, hc, generator=gen), torch.randn(n, hc, generator=gen)
    att = torch.randn(heads, C, generator=gen) * 0.5
    bias, dout = torch.randn(hc, generator=gen), torch.randn(n, hc, generator=gen)
    ref, rows = kernel_reference(xl, xr, att, bias, dout, ei, n, heads, loops, torch.float64)
    r32, _ = kernel_reference(xl, xr, att, bias, dout, ei, n, heads, loops, torch.float32)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=loops)
    assert g.nnz == len(rows)
    xld, xrd, attd, doutd = xl.to(dev), xr.to(dev), att.to(dev), dout.to(dev)
    got = {}
    got["y"], got["alpha"] = ops.gatv2_fwd(g, xld, xrd, attd, heads, 0.2, bias=bias.to(dev))
    got["dz"], got["dxr"], part = ops.gatv2_bwd_edge(g, doutd, xld, xrd, attd, got["alpha"], heads, 0.2)
    got["dxl"] = ops.gatv2_bwd_node(g, doutd, xld, xrd, attd, got["alpha"], got["dz"], heads, 0.2)
    got["datt"] = ops.gatv2_datt(part, heads)
    torch.cuda.synchronize()
    # each row's alpha sums to 1 per head, to 0 on an empty row
    sums = torch.zeros((n, heads), dtype=torch.float64).index_add_(0, rows, got["alpha"].double().cpu())
    empty = torch.from_numpy(np.bincount(rows.numpy(), minlength=n) == 0)
    assert bool(empty.any()) == (not loops)
    assert float((sums[~empty] - 1).abs().max()) < 1e-5 and float(sums[empty].abs().max() if empty.any() else 0.0) == 0.0
    if empty.any():
        assert torch.equal(got["y"].cpu()[empty], bias.expand(int(empty.sum()), -1))    # zero aggregate plus bias
        assert not got["dxr"].cpu()[empty].any()
    for k in ("y", "dxl", "dxr"):
        e = relerr(got[k], ref[k])
        print("%s C=%d heads=%d %s: rel-L2 %.2e (tolerance %.0e)" % (name, C, heads, k, e, OP_TOL))
        assert e <= OP_TOL, (k, e)
    for k in ("alpha", "dz", "datt"):
        e, yard = relerr(got[k], ref[k]), relerr(r32[k], ref[k])
        print("%s C=%d heads=%d %s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (name, C, heads, k, e, yard, bound(yard)))
        assert e <= bound(yard), (k, e, yard)


def test_column_blocks_of_one_row_buffer_and_the_shared_operand(dev, graphs):
    """Xl and Xr as column blocks of a packed [Xl | Xr] buffer, outputs into column blocks, and Xl passed twice, give the bits of
    the contiguous call."""
    from dual_dmp_amd import ops
    ei, n = graphs["ico"]
    heads, C = 3, 8
    hc = heads * C
    g = ops.graph_for(ei.to(dev), n, norm="gat")
    torch.manual_seed(3)
    buf, att, dout = torch.randn(n, 2 * hc, device=dev), torch.randn(heads, C, device=dev), torch.randn(n, hc, device=dev)
    for xl, xr, cl, cr in ((buf[:, :hc], buf[:, hc:], buf[:, :hc].contiguous(), buf[:, hc:].contiguous()),
                           (buf[:, :hc], buf[:, :hc], buf[:, :hc].contiguous(), buf[:, :hc].contiguous())):
        y, alpha = ops.gatv2_fwd(g, xl, xr, att, heads, 0.2)
        y2, alpha2 = ops.gatv2_fwd(g, cl, cr, att, heads, 0.2)
        assert torch.equal(y, y2) and torch.equal(alpha, alpha2)
        gbuf = torch.zeros(n, 2 * hc, device=dev)
        dz, dxr, part = ops.gatv2_bwd_edge(g, dout, xl, xr, att, alpha, heads, 0.2, out=gbuf[:, hc:])
        dxl = ops.gatv2_bwd_node(g, dout, xl, xr, att, alpha, dz, heads, 0.2, out=gbuf[:, :hc])
        dz2, dxr2, part2 = ops.gatv2_bwd_edge(g, dout, cl, cr, att, alpha2, heads, 0.2)
        dxl2 = ops.gatv2_bwd_node(g, dout, cl, cr, att, alpha2, dz2, heads, 0.2)
        assert torch.equal(dz, dz2) and torch.equal(gbuf[:, hc:], dxr2) and torch.equal(part, part2) and torch.equal(gbuf[:, :hc], dxl2)
        assert dxr.data_ptr() == gbuf[:, hc:].data_ptr() and dxl.data_ptr() == gbuf.data_ptr()
        assert ops.gatv2_bwd_edge(g, dout, cl, cr, att, alpha2, heads, 0.2, want_datt=False)[2] is None


# ------------------------------------------------------------------------------------------------ 2. the operator
PNAMES = ("lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias")


def _named(conv):
    have = dict(conv.named_parameters())
    return [(k, have[k]) for k in PNAMES if k in have]                # (shared weights: lin_r.* are lin_l.*, listed once)


def _operator_run(conv, x, ei, t, **kw):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, ei, **kw)
    (y * t).sum().backward()
    return dict([("y", y.detach()), ("dx", x.grad)] + [("d " + k, p.grad) for k, p in _named(conv)])


def device_decisions(conv, xd, ei, n):
    """The device's own branch decisions for ``conv`` at the device input ``xd``: [Xl | Xr] through the GEMM call the operator
    makes, then u = Xl[src] + Xr[dst] > 0 in float32 on the CPU.  -> pos [E, heads, C] bool."""
    from dual_dmp_amd import nn_ops, ops
    hc = conv.heads * conv.out_channels
    share = conv.share_weights
    with torch.no_grad():
        xp = nn_ops._pad_cols(xd.detach().to(torch.float32))
        wp = nn_ops._packed_rows((conv.lin_l.weight, None if share else conv.lin_r.weight), xp.shape[1], xd.device)
        lb = None
        if conv.lin_l.bias is not None:
            lb = nn_ops._packed_rows((conv.lin_l.bias.view(-1, 1), None if share else conv.lin_r.bias.view(-1, 1)), 1, xd.device).view(-1)
        buf = ops.gemm_nt(xp, wp, bias=lb).cpu()
    xl = buf[:, :hc].reshape(n, conv.heads, -1)
    xr = xl if share else buf[:, hc:2 * hc].reshape(n, conv.heads, -1)
    src, dst = gatv2_edges(ei, n, conv.add_self_loops)
    return (xl[src] + xr[dst]) > 0


def check_decisions(tag, pos, ref, x64, ei):
    """Conditions (a) and (b) of the module docstring for the float64 reference ``ref`` at its input ``x64``."""
    with torch.no_grad():
        _, aux = ref(x64, ei, full=True)
        ml = x64.abs() @ ref.lin_l.weight.abs().t()
        mr = x64.abs() @ ref.lin_r.weight.abs().t()
    margin = 64 * EPS * (ml[aux["src"]] + mr[aux["dst"]]).view(aux["u"].shape)
    diff = pos != aux["own"]
    worst = float((aux["u"].abs() / margin)[diff].max()) if diff.any() else 0.0
    share = float(diff.sum()) / diff.numel()
    print("%s: %d of %d branch decisions differ (share %.2e, bound 1e-4); largest |u_ref| / margin among them %.3f (bound 1)"
          % (tag, int(diff.sum()), diff.numel(), share, worst))
    assert worst <= 1.0, (tag, worst)
    assert share <= 1e-4, (tag, share)


@pytest.mark.parametrize("cin,cout,heads", CASES)
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("share", [False, True])
def test_operator_matches_the_float64_reference(dev, graphs, cin, cout, heads, concat, loops, share):
    from dual_dmp_amd.nn_ops import GATv2Conv
    ei, n = graphs["hub" if loops else "ico-iso"]
    torch.manual_seed(cin + heads)
    conv = GATv2Conv(cin, cout, heads=heads, concat=concat, add_self_loops=loops, share_weights=share)
    with torch.no_grad():
        conv.bias.normal_(std=0.3)
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, cin, generator=gen)
    t = torch.randn(n, heads * cout if concat else cout, generator=gen)
    refs = {dtype: GATv2ConvRef(cin, cout, heads, concat, 0.2, loops, share_weights=share, dtype=dtype).load_from(conv)
            for dtype in (torch.float64, torch.float32)}
    conv.to(dev)
    got = _operator_run(conv, x.to(dev), ei.to(dev), t.to(dev))
    pos = device_decisions(conv, x.to(dev), ei, n)
    check_decisions("in=%d C=%d heads=%d" % (cin, cout, heads), pos, refs[torch.float64], x.double(), ei)
    r64, r32 = (_operator_run(refs[dtype], x.to(dtype), ei, t.to(dtype), pos=pos) for dtype in (torch.float64, torch.float32))
    assert list(got) == list(r64) and len(got) == (6 if share else 8)
    for k in got:
        assert got[k].shape == r64[k].shape, k
        e, yard = relerr(got[k], r64[k]), relerr(r32[k], r64[k])
        if k == "d att":
            print("%s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (k, e, yard, bound(yard)))
            assert e <= bound(yard), (k, e, yard)
        else:
            print("%s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)" % (k, e, OP_TOL, yard))
            assert e <= OP_TOL, (k, e)


# ------------------------------------------------------------------------------------------------ 3. reproducibility
def test_two_runs_give_the_same_bits(dev, graphs):
    from dual_dmp_amd.nn_ops import GATv2Conv
    ei, n = graphs["hub"]
    eid = ei.to(dev)
    for (cin, cout, heads), share in (((32, 40, 3), False), ((8, 16, 3), True), ((3, 3, 2), False)):
        torch.manual_seed(1)
        conv = GATv2Conv(cin, cout, heads=heads, share_weights=share).to(dev)
        x, t = torch.randn(n, cin, device=dev), torch.randn(n, heads * cout, device=dev)
        a = {k: v.clone() for k, v in _operator_run(conv, x, eid, t).items()}
        b = _operator_run(conv, x, eid, t)
        for k in a:
            assert torch.equal(a[k], b[k]), (cin, cout, heads, k)


# ------------------------------------------------------------------------------------------------ 4. training
class _TwoLayer(torch.nn.Module):
    def __init__(self, mk):
        super().__init__()
        self.c1, self.c2 = mk(8, 8, 2), mk(16, 3, 1)

    def forward(self, x, ei, pos=(None, None)):
        kw = [{} if p is None else {"pos": p} for p in pos]
        return self.c2(torch.relu(self.c1(x, ei, **kw[0])), ei, **kw[1])


def test_short_training_loop(dev, graphs):
    """10 Adam steps of a two-layer GATv2 regressing a fixed target on "ico": the loss falls; for the first 3 steps the loss and
    the full parameter gradient stay within the yardstick-derived bound of the float64 reference evaluated at the SAME parameters
    and the SAME branch decisions (teacher-forced: the reference is loaded from the GPU model, and both layers' decisions are
    recomputed from the GPU model, before every compared step)."""
    from dual_dmp_amd.nn_ops import GATv2Conv
    ei, n = graphs["ico"]
    gen = torch.Generator().manual_seed(4)
    x, target = torch.randn(n, 8, generator=gen), torch.randn(n, 3, generator=gen)
    torch.manual_seed(4)
    net = _TwoLayer(lambda i, o, h: GATv2Conv(i, o, heads=h)).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    xd, td, eid = x.to(dev), target.to(dev), ei.to(dev)

    def ref_eval(dtype, pos, step):
        r = _TwoLayer(lambda i, o, h: GATv2ConvRef(i, o, h, dtype=dtype))
        r.c1.load_from(net.c1), r.c2.load_from(net.c2)
        if dtype == torch.float64:
            with torch.no_grad():
                h1 = torch.relu(r.c1(x.double(), ei, pos=pos[0]))
            check_decisions("step %d layer 1" % step, pos[0], r.c1, x.double(), ei)
            check_decisions("step %d layer 2" % step, pos[1], r.c2, h1, ei)
        loss = ((r(x.to(dtype), ei, pos=pos) - target.to(dtype)) ** 2).mean()
        loss.backward()
        return float(loss.detach()), torch.cat([p.grad.reshape(-1) for _, p in _named(r.c1) + _named(r.c2)])

    losses = []
    for step in range(10):
        opt.zero_grad()
        loss = ((net(xd, eid) - td) ** 2).mean()
        loss.backward()
        if step < 3:
            with torch.no_grad():
                h1d = torch.relu(net.c1(xd, eid))
            pos = (device_decisions(net.c1, xd, ei, n), device_decisions(net.c2, h1d, ei, n))
            l64, g64 = ref_eval(torch.float64, pos, step)
            l32, g32 = ref_eval(torch.float32, pos, step)
            g = torch.cat([p.grad.reshape(-1) for _, p in _named(net.c1) + _named(net.c2)])
            el, yl = abs(float(loss.detach()) - l64) / l64, abs(l32 - l64) / l64
            eg, yg = relerr(g, g64), relerr(g32, g64)
            print("step %d: loss rel %.2e (yardstick %.2e, bound %.2e), gradient rel-L2 %.2e (yardstick %.2e, bound %.2e)"
                  % (step, el, yl, bound(yl), eg, yg, bound(yg)))
            assert el <= bound(yl) and eg <= bound(yg), (step, el, yl, eg, yg)
        opt.step()
        losses.append(float(loss.detach()))
    print("loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------ 5. index width
def two_ring_reference(rowptr, col, s0, fetch_xl, fetch_xr, fetch_dout, att, heads, C, slope=0.2):
    """y, dXl and dXr of the rows ``s0`` in float64 from rows of Xl, Xr and dOut alone (``fetch_*``: row ids -> float64 CPU rows),
    on a graph without duplicate edges: ring 1 = the rows s0 references (whose softmax, delta and dz are needed in full), ring 2 =
    those rows' columns (whose Xl is needed).  Written per entry, without the mirror map."""
    span = lambda rows: np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows])
    s1 = np.unique(np.concatenate([col[span(s0)], s0]))
    ent = span(s1)
    erow, ecol = np.repeat(s1, rowptr[s1 + 1] - rowptr[s1]), col[ent]
    s2 = np.unique(np.concatenate([ecol, s1]))
    i1, i2 = torch.from_numpy(np.searchsorted(s1, erow)), torch.from_numpy(np.searchsorted(s2, ecol))
    XL = fetch_xl(s2).view(len(s2), heads, C)
    XR = fetch_xr(s1).view(len(s1), heads, C)
    D = fetch_dout(s1).view(len(s1), heads, C)
    zero = lambda k: torch.zeros((k, heads), dtype=torch.float64)
    u = XL[i2] + XR[i1]                                           # (float32 values added in float64: the sign of the float32 sum)
    z = (torch.where(u > 0, u, slope * u) * att).sum(-1)
    m = torch.full((len(s1), heads), -float("inf"), dtype=torch.float64).scatter_reduce(0, i1.view(-1, 1).expand(-1, heads), z, "amax")
    ex = torch.exp(z - m[i1])                                     # (no duplicate edges: every multiplicity is 1)
    al = ex / zero(len(s1)).index_add_(0, i1, ex)[i1]
    dal = (D[i1] * XL[i2]).sum(-1)
    delta = zero(len(s1)).index_add_(0, i1, al * dal)
    dz = al * (dal - delta[i1])
    du = dz.unsqueeze(-1) * att * torch.where(u > 0, torch.ones_like(u), torch.full_like(u, slope))
    y_ref = torch.zeros((len(s1), heads, C), dtype=torch.float64).index_add_(0, i1, al.unsqueeze(-1) * XL[i2])
    dxr_ref = torch.zeros((len(s1), heads, C), dtype=torch.float64).index_add_(0, i1, du)
    dxl_ref = torch.zeros((len(s2), heads, C), dtype=torch.float64).index_add_(0, i2, al.unsqueeze(-1) * D[i1] + du)
    p1, p2 = torch.from_numpy(np.searchsorted(s1, s0)), torch.from_numpy(np.searchsorted(s2, s0))
    return y_ref[p1], dxl_ref[p2], dxr_ref[p1]


def test_offsets_beyond_2_31_bytes(dev):
    """1,100,000-node vertex graph of a torus, heads * C = 4 * 128 = 512: N * heads * C * 4 bytes = 2.25e9 > 2^31, and Xl / Xr are
    the column blocks of ONE [N, 1024] row buffer.  Forward and backward once; from the GPU's own Xl and Xr, the y, dXl and dXr of
    600 sampled rows are recomputed in float64 on the CPU from their two-ring neighbourhoods and compared at the operator
    tolerance."""
    from dual_dmp_amd import ops, synth
    heads, C, cin = 4, 128, 16
    hc = heads * C
    v, f = synth.torus(1100, 1000)
    n = len(v)
    assert n == 1100000 and n * hc * 4 > 2 ** 31
    f = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // n, key % n])).contiguous()
    t = ops.csr_build_valued_host(ei.numpy(), n, ops.GV_LOOPS)
    rowptr, col = t["rowptr"].astype(np.int64), t["col"].astype(np.int64)
    g = ops.graph_for(ei.to(dev), n, norm="gat")
    torch.manual_seed(7)
    x, wgt = torch.randn(n, cin, device=dev), torch.randn(2 * hc, cin, device=dev) * 0.3
    att = torch.randn(heads, C, device=dev) * 0.1
    buf = ops.gemm_nt(x, wgt)
    xl, xr = buf[:, :hc], buf[:, hc:]
    dout = torch.randn(n, hc, device=dev)
    y, alpha = ops.gatv2_fwd(g, xl, xr, att, heads, 0.2)
    gbuf = torch.empty(n, 2 * hc, device=dev)
    dz, dxr, _ = ops.gatv2_bwd_edge(g, dout, xl, xr, att, alpha, heads, 0.2, out=gbuf[:, hc:], want_datt=False)
    dxl = ops.gatv2_bwd_node(g, dout, xl, xr, att, alpha, dz, heads, 0.2, out=gbuf[:, :hc])
    torch.cuda.synchronize()
    # sampled rows, the last rows among them: the largest offsets
    rng = np.random.default_rng(0)
    s0 = np.unique(np.concatenate([rng.choice(n - 10, 590, replace=False), np.arange(n - 10, n)]))
    assert len(s0) == 600
    fetch = lambda m: (lambda r: m[torch.from_numpy(r).to(dev)].double().cpu())
    y_ref, dxl_ref, dxr_ref = two_ring_reference(rowptr, col, s0, fetch(xl), fetch(xr), fetch(dout), att.double().cpu(), heads, C)
    rows0 = torch.from_numpy(s0).to(dev)
    errs = [relerr(a[rows0].reshape(-1, heads, C), b) for a, b in ((y, y_ref), (dxl, dxl_ref), (dxr, dxr_ref))]
    print("1.1M nodes x 512: y rel-L2 %.2e, dXl rel-L2 %.2e, dXr rel-L2 %.2e over %d sampled rows (tolerance %.0e)"
          % (errs[0], errs[1], errs[2], len(s0), OP_TOL))
    assert max(errs) <= OP_TOL

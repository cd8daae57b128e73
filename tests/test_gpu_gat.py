"""GATConv on the GPU: the attention kernels (scores, edge softmax + gather, the two backward launches, the attention-vector
reduction) and the drop-in against the float64 edge-list reference (tests/gat_ref.py) on the icosphere (ragged last chunk), the
open grid (boundary) and the hub graph (one 1200-entry row), with duplicate edges and explicit loops on top.

Tolerance policy, every comparison against ``GATConvRef`` / ``gat_edge_list`` in float64:
* y, dx, dW, db, dHf: the project's operator tolerance, rel-L2 <= 1e-5;
* datt_src / datt_dst and the kernel-level arrays (alpha, ds, ds_src, ds_dst) have no project tolerance: the yardstick is the
  float32 CPU evaluation of the same reference against its float64 evaluation on the same inputs, the bound 4x that and not
  below FLOOR (the policy of test_gpu_edge_weight.py).  Both figures are printed."""
import numpy as np
import pytest
import torch

import edge_weight_route_worker as W
import oracle_jobs as OJ
from gat_ref import GATConvRef, gat_edge_list

pytestmark = pytest.mark.gpu
relerr = W.relerr

OP_TOL = 1e-5
# 16 float32 epsilons: two float32 evaluations of a sum of a few hundred to a few thousand terms in different orders differ by
# about sqrt(terms) * 2^-24 relative to the terms' norm, whatever the yardstick's own (pairwise) order happens to give
FLOOR = 16 * 2.0 ** -23

CASES = [(3, 3, 2), (16, 4, 8), (8, 32, 1), (32, 40, 3), (64, 64, 4)]          # (in, out per head, heads)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graphs():
    """name -> (edge_index, n): the route worker's graphs + duplicates and explicit loops (two on node 5); "<name>-iso": one more
    node without any edge (an empty row when no loops are added)."""
    out = {}
    base = W.graphs()
    for name in ("ico", "grid", "hub"):
        ei, n = base[name]
        extra = torch.tensor([[3, 9, 5, 5, 40], [9, 3, 5, 5, 40]])
        dup = ei[:, :50]
        ei = torch.cat([ei, extra, dup, dup[[1, 0]]], 1).contiguous()
        out[name] = (ei, n)
        out[name + "-iso"] = (ei, n + 1)
    return out


def bound(yard):
    return max(4.0 * yard, FLOOR)


def entry_map(ei, n, loops, src, dst):
    """Host CSR tables of the attention graph and, for every reference edge, the index of its coalesced entry."""
    from dual_dmp_amd import ops
    t = ops.csr_build_valued_host(ei.numpy(), n, ops.GV_LOOPS if loops else 0)
    rows = np.repeat(np.arange(n), np.diff(t["rowptr"]))
    keys = rows.astype(np.int64) * n + t["col"]
    assert np.all(np.diff(keys) > 0)
    ent = np.searchsorted(keys, dst.numpy() * n + src.numpy())
    assert np.array_equal(keys[ent], dst.numpy() * n + src.numpy())
    return t, torch.from_numpy(rows), torch.from_numpy(ent)


def kernel_reference(hf, att_src, att_dst, bias, dout, ei, n, heads, loops, dtype):
    """Everything the kernels produce, from the edge-list reference in ``dtype`` with Hf as the input (identity weight)."""
    hc = hf.shape[1]
    x = hf.to(dtype).requires_grad_(True)
    a_s, a_d = att_src.to(dtype).requires_grad_(True), att_dst.to(dtype).requires_grad_(True)
    y, aux = gat_edge_list(x, ei, torch.eye(hc, dtype=dtype), a_s, a_d, bias.to(dtype), heads, True, 0.2, loops, full=True)
    (y * dout.to(dtype)).sum().backward()
    _, rows, ent = entry_map(ei, n, loops, aux["src"], aux["dst"])
    nnz = len(rows)
    alpha = torch.zeros((nnz, heads), dtype=dtype).index_add_(0, ent, aux["alpha"].detach())
    ds = torch.zeros((nnz, heads), dtype=dtype).index_add_(0, ent, aux["pre"].grad)
    ds_dst = torch.zeros((n, heads), dtype=dtype).index_add_(0, aux["dst"], aux["pre"].grad)
    ds_src = torch.zeros((n, heads), dtype=dtype).index_add_(0, aux["src"], aux["pre"].grad)
    return dict(s_src=aux["s_src"].detach(), s_dst=aux["s_dst"].detach(), y=y.detach(), alpha=alpha, ds=ds, ds_dst=ds_dst,
                ds_src=ds_src, dhf=x.grad, datt_src=a_s.grad.view(heads, -1), datt_dst=a_d.grad.view(heads, -1)), rows


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("name,loops", [("ico", True), ("grid", True), ("hub", True), ("grid-iso", False), ("hub-iso", False)])
@pytest.mark.parametrize("C,heads", [(c[1], c[2]) for c in CASES])
def test_kernels_match_the_reference(dev, graphs, name, loops, C, heads):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    gen = torch.Generator().manual_seed(n + C)
    hf = torch.randn(n, heads * C, generator=gen)
    att_src, att_dst = torch.randn(heads, C, generator=gen) * 0.5, torch.randn(heads, C, generator=gen) * 0.5
    bias, dout = torch.randn(heads * C, generator=gen), torch.randn(n, heads * C, generator=gen)
    ref, rows = kernel_reference(hf, att_src, att_dst, bias, dout, ei, n, heads, loops, torch.float64)
    r32, _ = kernel_reference(hf, att_src, att_dst, bias, dout, ei, n, heads, loops, torch.float32)
    eid = ei.to(dev)
    g = ops.graph_for(eid, n, norm="gat", add_self_loops=loops)
    assert g.nnz == len(rows)
    hfd, asd, add, doutd = hf.to(dev), att_src.to(dev), att_dst.to(dev), dout.to(dev)
    got = {}
    got["s_src"], got["s_dst"] = ops.gat_scores(hfd, asd, add, heads)
    got["y"], got["alpha"] = ops.gat_fwd(g, hfd, got["s_src"], got["s_dst"], heads, 0.2, bias=bias.to(dev))
    got["ds"], got["ds_dst"] = ops.gat_bwd_edge(g, doutd, hfd, got["s_src"], got["s_dst"], got["alpha"], heads, 0.2)
    got["dhf"], got["ds_src"] = ops.gat_bwd_node(g, doutd, got["alpha"], got["ds"], got["ds_dst"], asd, add, heads)
    got["datt_src"], got["datt_dst"] = ops.gat_datt(hfd, got["ds_src"], got["ds_dst"], heads)
    torch.cuda.synchronize()
    # each row's alpha sums to 1 per head, to 0 on an empty row
    sums = torch.zeros((n, heads), dtype=torch.float64).index_add_(0, rows, got["alpha"].double().cpu())
    empty = torch.from_numpy(np.bincount(rows.numpy(), minlength=n) == 0)
    assert bool(empty.any()) == (not loops)
    assert float((sums[~empty] - 1).abs().max()) < 1e-5 and float(sums[empty].abs().max() if empty.any() else 0.0) == 0.0
    if empty.any():
        assert torch.equal(got["y"].cpu()[empty], bias.expand(int(empty.sum()), -1))    # zero aggregate plus bias
    for k in ("y", "dhf", "s_src", "s_dst"):
        e = relerr(got[k], ref[k])
        print("%s C=%d heads=%d %s: rel-L2 %.2e (tolerance %.0e)" % (name, C, heads, k, e, OP_TOL))
        assert e <= OP_TOL, (k, e)
    for k in ("alpha", "ds", "ds_src", "ds_dst", "datt_src", "datt_dst"):
        e, yard = relerr(got[k], ref[k]), relerr(r32[k], ref[k])
        print("%s C=%d heads=%d %s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (name, C, heads, k, e, yard, bound(yard)))
        assert e <= bound(yard), (k, e, yard)


# ------------------------------------------------------------------------------------------------ 2. the operator
def _operator_run(conv, x, ei, t):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, ei)
    (y * t).sum().backward()
    return [y.detach(), x.grad] + [p.grad for p in (conv.lin_src.weight, conv.att_src, conv.att_dst, conv.bias)]


NAMES = ("y", "dx", "dW", "datt_src", "datt_dst", "db")


@pytest.mark.parametrize("cin,cout,heads", CASES)
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("loops", [True, False])
def test_operator_matches_the_float64_reference(dev, graphs, cin, cout, heads, concat, loops):
    from dual_dmp_amd.nn_ops import GATConv
    ei, n = graphs["hub" if loops else "ico-iso"]
    torch.manual_seed(cin + heads)
    conv = GATConv(cin, cout, heads=heads, concat=concat, add_self_loops=loops)
    with torch.no_grad():
        conv.bias.normal_(std=0.3)
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, cin, generator=gen)
    t = torch.randn(n, heads * cout if concat else cout, generator=gen)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        r = GATConvRef(cin, cout, heads, concat, 0.2, loops, dtype=dtype).load_from(conv)
        refs[dtype] = _operator_run(r, x.to(dtype), ei, t.to(dtype))
    conv.to(dev)
    got = _operator_run(conv, x.to(dev), ei.to(dev), t.to(dev))
    for k, a, b, c in zip(NAMES, got, refs[torch.float64], refs[torch.float32]):
        assert a.shape == b.shape, k
        e, yard = relerr(a, b), relerr(c, b)
        if k.startswith("datt"):
            print("%s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (k, e, yard, bound(yard)))
            assert e <= bound(yard), (k, e, yard)
        else:
            print("%s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)" % (k, e, OP_TOL, yard))
            assert e <= OP_TOL, (k, e)


def test_two_runs_give_the_same_bits(dev, graphs):
    from dual_dmp_amd.nn_ops import GATConv
    ei, n = graphs["hub"]
    eid = ei.to(dev)
    for cin, cout, heads in ((32, 40, 3), (16, 4, 8), (3, 3, 2)):
        torch.manual_seed(1)
        conv = GATConv(cin, cout, heads=heads).to(dev)
        x, t = torch.randn(n, cin, device=dev), torch.randn(n, heads * cout, device=dev)
        a = [v.clone() for v in _operator_run(conv, x, eid, t)]
        b = _operator_run(conv, x, eid, t)
        for k, u, v in zip(NAMES, a, b):
            assert torch.equal(u, v), (cin, cout, heads, k)


def test_gcnconv_and_gatconv_keep_their_own_graphs(dev, graphs):
    from dual_dmp_amd import ops
    from dual_dmp_amd.nn_ops import GATConv, GCNConv
    ei, n = graphs["ico"]
    eid = ei.to(dev)
    torch.manual_seed(2)
    gcn, gat = GCNConv(16, 8).to(dev), GATConv(16, 4, heads=2).to(dev)
    x, t = torch.randn(n, 16, device=dev), torch.randn(n, 8, device=dev)
    w = W.weights(ei.shape[1], 3).to(dev)

    def gcn_run(weight=None):
        xx = x.clone().requires_grad_(True)
        y = gcn(xx, eid) if weight is None else gcn(xx, eid, weight)
        g, = torch.autograd.grad((y * t).sum(), xx)
        return y.detach(), g

    alone_gat = [v.clone() for v in _operator_run(gat, x, eid, t)]
    alone_gcn, alone_gcnw = gcn_run(), gcn_run(w)
    g_gat = ops.graph_for(eid, n, norm="gat")
    assert g_gat is not ops.graph_for(eid, n) and g_gat is not ops.graph_for(eid, n, edge_weight=w)
    assert g_gat is not ops.graph_for(eid, n, add_self_loops=False, normalize=False)
    # interleaved: a weighted and a plain GCNConv call between the GAT forward and its backward
    xx = x.clone().requires_grad_(True)
    for p in gat.parameters():
        p.grad = None
    y = gat(xx, eid)
    mid_w, mid = gcn_run(w), gcn_run()
    (y * t).sum().backward()
    mixed = [y.detach(), xx.grad] + [p.grad for p in (gat.lin_src.weight, gat.att_src, gat.att_dst, gat.bias)]
    for k, u, v in zip(NAMES, alone_gat, mixed):
        assert torch.equal(u, v), k
    for u, v in zip(alone_gcn + alone_gcnw, mid + mid_w):
        assert torch.equal(u, v)
    assert ops.graph_for(eid, n, norm="gat") is g_gat and g_gat.n_set_values == 0 and g_gat.values_key == ("ones",)


# ------------------------------------------------------------------------------------------------ 3. training
class _TwoLayer(torch.nn.Module):
    def __init__(self, mk):
        super().__init__()
        self.c1, self.c2 = mk(8, 8, 2), mk(16, 3, 1)

    def forward(self, x, ei):
        return self.c2(torch.relu(self.c1(x, ei)), ei)


def test_short_training_loop(dev, graphs):
    """20 Adam steps of a two-layer GAT regressing a fixed target on "ico": the loss falls; for the first 3 steps the loss and the
    full parameter gradient stay within the yardstick-derived bound of the float64 reference evaluated at the SAME parameters
    (teacher-forced: the reference is loaded from the GPU model before every compared step)."""
    from dual_dmp_amd.nn_ops import GATConv
    ei, n = graphs["ico"]
    gen = torch.Generator().manual_seed(4)
    x, target = torch.randn(n, 8, generator=gen), torch.randn(n, 3, generator=gen)
    torch.manual_seed(4)
    net = _TwoLayer(lambda i, o, h: GATConv(i, o, heads=h)).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    xd, td, eid = x.to(dev), target.to(dev), ei.to(dev)

    def ref_eval(dtype):
        r = _TwoLayer(lambda i, o, h: GATConvRef(i, o, h, dtype=dtype))
        r.c1.load_from(net.c1), r.c2.load_from(net.c2)
        loss = ((r(x.to(dtype), ei) - target.to(dtype)) ** 2).mean()
        loss.backward()
        return float(loss.detach()), torch.cat([p.grad.reshape(-1) for p in r.parameters()])

    losses = []
    for step in range(20):
        opt.zero_grad()
        loss = ((net(xd, eid) - td) ** 2).mean()
        loss.backward()
        if step < 3:
            l64, g64 = ref_eval(torch.float64)
            l32, g32 = ref_eval(torch.float32)
            g = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
            el, yl = abs(float(loss.detach()) - l64) / l64, abs(l32 - l64) / l64
            eg, yg = relerr(g, g64), relerr(g32, g64)
            print("step %d: loss rel %.2e (yardstick %.2e, bound %.2e), gradient rel-L2 %.2e (yardstick %.2e, bound %.2e)"
                  % (step, el, yl, bound(yl), eg, yg, bound(yg)))
            assert el <= bound(yl) and eg <= bound(yg), (step, el, yl, eg, yg)
        opt.step()
        losses.append(float(loss.detach()))
    print("loss %.4f -> %.4f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]


def test_modular_nets_run_with_conv_gat(dev):
    from dual_dmp_amd.networks import NormalNet, PosNet
    from dual_dmp_amd.nn_ops import GATConv
    gt, noisy, smooth, data = OJ.case("ico3")
    for Ours, n_out in ((PosNet, len(noisy.vs)), (NormalNet, len(noisy.faces))):
        torch.manual_seed(6)
        net = Ours(dev, fused=False, conv="gat", heads=4)
        assert isinstance(net.conv7, GATConv)
        net.train()
        o = net(data)
        assert o.shape == (n_out, 3) and bool(torch.isfinite(o).all())
        o.backward(torch.randn(n_out, 3, device=dev))
        for name, p in net.named_parameters():
            assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name


# ------------------------------------------------------------------------------------------------ 4. index width
def two_ring_reference(rowptr, col, s0, fetch_hf, fetch_dout, a_s, a_d, heads, C, slope=0.2):
    """y and dHf of the rows ``s0`` in float64 from rows of Hf and dOut alone (``fetch_*``: row ids -> float64 CPU rows), on a
    graph without duplicate edges: ring 1 = the rows s0 references (whose softmax, delta and ds are needed in full), ring 2 =
    those rows' columns (whose Hf is needed).  Written per entry, without the mirror map."""
    span = lambda rows: np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows])
    s1 = np.unique(np.concatenate([col[span(s0)], s0]))
    ent = span(s1)
    erow, ecol = np.repeat(s1, rowptr[s1 + 1] - rowptr[s1]), col[ent]
    s2 = np.unique(np.concatenate([ecol, s1]))
    i1, i2 = torch.from_numpy(np.searchsorted(s1, erow)), torch.from_numpy(np.searchsorted(s2, ecol))
    H = fetch_hf(s2).view(len(s2), heads, C)
    Hrow = H[torch.from_numpy(np.searchsorted(s2, s1))]
    D = fetch_dout(s1).view(len(s1), heads, C)
    ss, sd = (H * a_s).sum(-1), (Hrow * a_d).sum(-1)
    z0 = ss[i2] + sd[i1]
    z = torch.where(z0 > 0, z0, slope * z0)
    zero = lambda k: torch.zeros((k, heads), dtype=torch.float64)
    m = torch.full((len(s1), heads), -float("inf"), dtype=torch.float64).scatter_reduce(0, i1.view(-1, 1).expand(-1, heads), z, "amax")
    ex = torch.exp(z - m[i1])                                     # (no duplicate edges: every multiplicity is 1)
    al = ex / zero(len(s1)).index_add_(0, i1, ex)[i1]
    dal = (D[i1] * H[i2]).sum(-1)
    delta = zero(len(s1)).index_add_(0, i1, al * dal)
    dsr = al * (dal - delta[i1]) * torch.where(z0 > 0, torch.ones_like(z0), torch.full_like(z0, slope))
    dsd = zero(len(s1)).index_add_(0, i1, dsr)
    dss = zero(len(s2)).index_add_(0, i2, dsr)
    y_ref = torch.zeros((len(s1), heads, C), dtype=torch.float64)
    dh_ref = torch.zeros((len(s2), heads, C), dtype=torch.float64)
    for h in range(heads):                                        # (per head: [entries, C] float64 at a time)
        y_ref[:, h].index_add_(0, i1, al[:, h, None] * H[i2, h])
        dh_ref[:, h].index_add_(0, i2, al[:, h, None] * D[i1, h])
    p1, p2 = torch.from_numpy(np.searchsorted(s1, s0)), torch.from_numpy(np.searchsorted(s2, s0))
    return y_ref[p1], dh_ref[p2] + dss[p2].unsqueeze(-1) * a_s + dsd[p1].unsqueeze(-1) * a_d


def test_offsets_beyond_2_31_bytes(dev):
    """1,100,000-node vertex graph of a torus, heads * C = 4 * 128 = 512: N * heads * C * 4 bytes = 2.25e9 > 2^31.  Forward and
    backward once; from the GPU's own Hf, y and dHf of 2,000 sampled rows are recomputed in float64 on the CPU from their two-ring
    neighbourhoods (the rows' entries, and every entry of the rows those reference) and compared at the operator tolerance."""
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
    eid = ei.to(dev)
    g = ops.graph_for(eid, n, norm="gat")
    torch.manual_seed(7)
    x, wgt = torch.randn(n, cin, device=dev), torch.randn(hc, cin, device=dev) * 0.3
    att_src, att_dst = torch.randn(heads, C, device=dev) * 0.1, torch.randn(heads, C, device=dev) * 0.1
    hf = ops.gemm_nt(x, wgt)
    dout = torch.randn(n, hc, device=dev)
    s_src, s_dst = ops.gat_scores(hf, att_src, att_dst, heads)
    y, alpha = ops.gat_fwd(g, hf, s_src, s_dst, heads, 0.2)
    ds, ds_dst = ops.gat_bwd_edge(g, dout, hf, s_src, s_dst, alpha, heads, 0.2)
    dhf, ds_src = ops.gat_bwd_node(g, dout, alpha, ds, ds_dst, att_src, att_dst, heads)
    torch.cuda.synchronize()
    # sampled rows, the last rows among them: the largest offsets
    rng = np.random.default_rng(0)
    s0 = np.unique(np.concatenate([rng.choice(n - 10, 1990, replace=False), np.arange(n - 10, n)]))
    assert len(s0) == 2000
    y_ref, dh_ref = two_ring_reference(rowptr, col, s0, lambda r: hf[torch.from_numpy(r).to(dev)].double().cpu(),
                                       lambda r: dout[torch.from_numpy(r).to(dev)].double().cpu(), att_src.double().cpu(),
                                       att_dst.double().cpu(), heads, C)
    rows0 = torch.from_numpy(s0).to(dev)
    e_y, e_d = relerr(y[rows0].view(-1, heads, C), y_ref), relerr(dhf[rows0].view(-1, heads, C), dh_ref)
    print("1.1M nodes x 512: y rel-L2 %.2e, dHf rel-L2 %.2e over %d sampled rows (tolerance %.0e)" % (e_y, e_d, len(s0), OP_TOL))
    assert e_y <= OP_TOL and e_d <= OP_TOL

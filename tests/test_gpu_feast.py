"""FeaStConv on the GPU: the feature-steered kernels (head softmax + gather, the two backward launches, the offset reduction) and
the drop-in against the float64 edge-list reference (tests/feast_ref.py) on the icosphere (ragged last chunk), the open grid
(boundary) and the hub graph (one 1200-entry row), with duplicate edges and explicit loops on top, and with one edgeless node.

Tolerance policy, every comparison against ``FeaStConvRef`` / ``feast_edge_list`` in float64:
* y, dx, dW, db, dHf: the project's operator tolerance, rel-L2 <= 1e-5;
* beta, dz, rs, dP, du, dc have no project tolerance: the yardstick is the float32 CPU evaluation of the same reference against
  its float64 evaluation on the same inputs, the bound 4x that and not below FLOOR (the policy of test_gpu_gat.py).  Both
  figures are printed;
* heads = 1: the reference's dz, rs, dP, du and dc are identically zero (a softmax over one head is constant), so a rel-L2
  against them means nothing.  The condition instead: their norm is <= 16 float32 epsilons x the norm of the float64 per-entry
  array m_e g_e (m_e = a_e / deg_i, g_e = dOut[i,:] . Hf[j,0,:]), the quantity whose cancellation produces the zero."""
import numpy as np
import pytest
import torch

import edge_weight_route_worker as W
import oracle_jobs as OJ
from feast_ref import FeaStConvRef, feast_edge_list

pytestmark = pytest.mark.gpu
relerr = W.relerr

OP_TOL = 1e-5
# 16 float32 epsilons: two float32 evaluations of a sum of a few hundred to a few thousand terms in different orders differ by
# about sqrt(terms) * 2^-24 relative to the terms' norm, whatever the yardstick's own (pairwise) order happens to give
FLOOR = 16 * 2.0 ** -23

CASES = [(3, 3, 2), (16, 4, 8), (8, 32, 1), (32, 40, 3), (64, 64, 4)]          # (in, out, heads)


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
    """Host CSR tables of the graph and, for every reference edge, the index of its coalesced entry."""
    from dual_dmp_amd import ops
    t = ops.csr_build_valued_host(ei.numpy(), n, ops.GV_LOOPS if loops else 0)
    rows = np.repeat(np.arange(n), np.diff(t["rowptr"]))
    keys = rows.astype(np.int64) * n + t["col"]
    assert np.all(np.diff(keys) > 0)
    ent = np.searchsorted(keys, dst.numpy() * n + src.numpy())
    assert np.array_equal(keys[ent], dst.numpy() * n + src.numpy())
    return t, torch.from_numpy(rows), torch.from_numpy(ent)


def per_entry(aux, ei, n, loops, dtype):
    """From the ``full`` record of the edge-list reference (after its backward): the row of every CSR entry, the entry of every
    reference edge, and beta, dz [entries, heads], rs [n, heads] -- an entry sums its duplicate edges."""
    _, rows, ent = entry_map(ei, n, loops, aux["src"], aux["dst"])
    heads = aux["q"].shape[1]
    nnz = len(rows)
    beta = torch.zeros((nnz, heads), dtype=dtype).index_add_(0, ent, aux["q"].detach() / aux["deg"][aux["dst"]].unsqueeze(1))
    dz = torch.zeros((nnz, heads), dtype=dtype).index_add_(0, ent, aux["z"].grad)
    rs = torch.zeros((n, heads), dtype=dtype).index_add_(0, aux["dst"], aux["z"].grad)
    return rows, ent, beta, dz, rs


def mg_norm(aux, ent, nnz, dout):
    """|| m_e g_e || over the CSR entries in float64, heads = 1: m_e g_e = sum over the entry's edges of dOut[i] . Hf[j, 0] / deg_i."""
    g = (dout.double()[aux["dst"]] * aux["hf"].detach().double()[aux["src"], 0]).sum(1) / aux["deg"].double()[aux["dst"]]
    return float(torch.zeros(nnz, dtype=torch.float64).index_add_(0, ent, g).norm())


def kernel_reference(hf, p, c, bias, dout, ei, n, heads, loops, dtype):
    """Everything the kernels produce, from the edge-list reference in ``dtype`` with [Hf | P] as the input and selector weights
    (identity blocks: Hf and P reach the reference exactly)."""
    hc = hf.shape[1]
    x = torch.cat([hf, p], 1).to(dtype).requires_grad_(True)
    eye = torch.eye(hc + heads, dtype=dtype)
    cc = c.to(dtype).requires_grad_(True)
    y, aux = feast_edge_list(x, ei, eye[:hc], eye[hc:], cc, bias.to(dtype), heads, loops, full=True)
    (y * dout.to(dtype)).sum().backward()
    rows, ent, beta, dz, rs = per_entry(aux, ei, n, loops, dtype)
    return dict(y=y.detach(), beta=beta, dz=dz, rs=rs, dhf=x.grad[:, :hc], dp=x.grad[:, hc:], dc=cc.grad), rows, ent, aux


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("name,loops", [("ico", True), ("grid", True), ("hub", True), ("grid-iso", False), ("hub-iso", False)])
@pytest.mark.parametrize("C,heads", [(c[1], c[2]) for c in CASES])
def test_kernels_match_the_reference(dev, graphs, name, loops, C, heads):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    hc = heads * C
    gen = torch.Generator().manual_seed(n + C)
    hf, p = torch.randn(n, hc, generator=gen), torch.randn(n, heads, generator=gen)
    c, bias, dout = torch.randn(heads, generator=gen) * 0.5, torch.randn(C, generator=gen), torch.randn(n, C, generator=gen)
    ref, rows, ent, aux = kernel_reference(hf, p, c, bias, dout, ei, n, heads, loops, torch.float64)
    r32 = kernel_reference(hf, p, c, bias, dout, ei, n, heads, loops, torch.float32)[0]
    eid = ei.to(dev)
    g = ops.graph_for(eid, n, norm="gat", add_self_loops=loops)
    assert g.nnz == len(rows)
    wtp = (hc + heads + 3) // 4 * 4                               # the operator's layout: one row buffer [Hf | P | padding]
    buf = torch.zeros(n, wtp, device=dev)
    buf[:, :hc], buf[:, hc:hc + heads] = hf.to(dev), p.to(dev)
    hfd, pd, doutd = buf[:, :hc], buf[:, hc:hc + heads], dout.to(dev)
    got = {}
    got["y"], got["beta"] = ops.feast_fwd(g, hfd, pd, c.to(dev), heads, bias=bias.to(dev))
    got["dz"], got["rs"] = ops.feast_bwd_edge(g, doutd, hfd, got["beta"], heads)
    gbuf = torch.full((n, wtp), float("nan"), device=dev)
    got["dhf"], got["dp"] = ops.feast_bwd_node(g, doutd, got["beta"], got["dz"], got["rs"], heads, out=gbuf)
    got["dc"] = ops.feast_dc(got["rs"], heads)
    torch.cuda.synchronize()
    assert got["y"].shape == (n, C) and got["dhf"].shape == (n, hc) and got["dp"].shape == (n, heads) and got["dc"].shape == (heads,)
    assert bool(torch.isnan(gbuf[:, hc + heads:]).all()) and bool(torch.isfinite(gbuf[:, :hc + heads]).all())
    # each non-empty row's beta sums to 1 over its entries and heads, an empty row has none and gets the bias
    sums = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, got["beta"].double().cpu().sum(1))
    empty = torch.from_numpy(np.bincount(rows.numpy(), minlength=n) == 0)
    assert bool(empty.any()) == (not loops)
    assert float((sums[~empty] - 1).abs().max()) < 1e-5
    if empty.any():
        assert torch.equal(got["y"].cpu()[empty], bias.expand(int(empty.sum()), -1))
    for k in ("y", "dhf"):
        e = relerr(got[k], ref[k])
        print("%s C=%d heads=%d %s: rel-L2 %.2e (tolerance %.0e)" % (name, C, heads, k, e, OP_TOL))
        assert e <= OP_TOL, (k, e)
    e, yard = relerr(got["beta"], ref["beta"]), relerr(r32["beta"], ref["beta"])
    print("%s C=%d heads=%d beta: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (name, C, heads, e, yard, bound(yard)))
    assert e <= bound(yard), ("beta", e, yard)
    if heads == 1:
        lim = FLOOR * mg_norm(aux, ent, len(rows), dout)
        for k in ("dz", "rs", "dp", "dc"):
            assert float(ref[k].abs().max()) < 1e-12, k
            nrm = float(got[k].double().norm())
            print("%s C=%d heads=1 %s: norm %.2e (reference zero; limit 16 eps x ||m g|| = %.2e)" % (name, C, k, nrm, lim))
            assert nrm <= lim, (k, nrm, lim)
        return
    for k in ("dz", "rs", "dp", "dc"):
        e, yard = relerr(got[k], ref[k]), relerr(r32[k], ref[k])
        print("%s C=%d heads=%d %s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (name, C, heads, k, e, yard, bound(yard)))
        assert e <= bound(yard), (k, e, yard)


@pytest.mark.parametrize("heads", [3, 256])
def test_offset_reduction_over_five_partials(dev, heads):
    """``feast_dc`` alone on 4100 rows: five partials of 1024 rows, so every one of the final stage's four float64 lanes takes a
    partial and the first takes a second one (the graphs above stop at two partials).  256 columns is the widest it accepts.
    Against the float64 column sum, dc's comparison above: the float32 CPU column sum as the yardstick."""
    from dual_dmp_amd import ops
    rs = torch.randn(4100, heads, generator=torch.Generator().manual_seed(heads))
    ref = rs.double().sum(0)
    got = ops.feast_dc(rs.to(dev), heads)
    torch.cuda.synchronize()
    assert got.shape == (heads,)
    e, yard = relerr(got, ref), relerr(rs.sum(0), ref)
    print("feast_dc [4100, %d]: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (heads, e, yard, bound(yard)))
    assert e <= bound(yard), (e, yard)


# ------------------------------------------------------------------------------------------------ 2. the operator
def _operator_run(conv, x, ei, t, full=False):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    aux = None
    if full:
        y, aux = conv(x, ei, full=True)
    else:
        y = conv(x, ei)
    (y * t).sum().backward()
    return [y.detach(), x.grad] + [p.grad for p in (conv.lin.weight, conv.u.weight, conv.c, conv.bias)], aux


NAMES = ("y", "dx", "dW", "du", "dc", "db")


@pytest.mark.parametrize("cin,cout,heads", CASES)
@pytest.mark.parametrize("loops", [True, False])
def test_operator_matches_the_float64_reference(dev, graphs, cin, cout, heads, loops):
    from dual_dmp_amd.nn_ops import FeaStConv
    ei, n = graphs["hub" if loops else "ico-iso"]
    torch.manual_seed(cin + heads)
    conv = FeaStConv(cin, cout, heads=heads, add_self_loops=loops)
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, cin, generator=gen)
    t = torch.randn(n, cout, generator=gen)
    refs, aux = {}, None
    for dtype in (torch.float64, torch.float32):
        r = FeaStConvRef(cin, cout, heads, loops, dtype=dtype).load_from(conv)
        refs[dtype], a = _operator_run(r, x.to(dtype), ei, t.to(dtype), full=True)
        aux = a if dtype == torch.float64 else aux
    conv.to(dev)
    got, _ = _operator_run(conv, x.to(dev), ei.to(dev), t.to(dev))
    lim = None
    if heads == 1:
        _, rows, ent = entry_map(ei, n, loops, aux["src"], aux["dst"])
        lim = FLOOR * mg_norm(aux, ent, len(rows), t)
    for k, a, b, c in zip(NAMES, got, refs[torch.float64], refs[torch.float32]):
        assert a.shape == b.shape, k
        if k in ("du", "dc") and heads == 1:
            nrm = float(a.double().norm())
            print("%s: norm %.2e (reference zero; limit 16 eps x ||m g|| = %.2e)" % (k, nrm, lim))
            assert float(b.abs().max()) < 1e-12 and nrm <= lim, (k, nrm, lim)
            continue
        e, yard = relerr(a, b), relerr(c, b)
        if k in ("du", "dc"):
            print("%s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (k, e, yard, bound(yard)))
            assert e <= bound(yard), (k, e, yard)
        else:
            print("%s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)" % (k, e, OP_TOL, yard))
            assert e <= OP_TOL, (k, e)


# ------------------------------------------------------------------------------------------------ 3. training
class _RefPosNet(torch.nn.Module):
    """The modular PosNet with FeaStConvRef layers, in ``dtype``: same parameter and buffer names as the net under test."""

    def __init__(self, widths, heads, dtype):
        super().__init__()
        for i in range(12):
            setattr(self, "conv%d" % (i + 1), FeaStConvRef(widths[i], widths[i + 1], heads, dtype=dtype))
            setattr(self, "bn%d" % (i + 1), torch.nn.BatchNorm1d(widths[i + 1], dtype=dtype))
        self.linear1 = torch.nn.Linear(widths[12], widths[13], dtype=dtype)
        self.linear2 = torch.nn.Linear(widths[13], widths[14], dtype=dtype)
        self.l_relu = torch.nn.LeakyReLU()

    def forward(self, z1, x_pos, ei):
        x = z1
        for i in range(1, 13):
            x = self.l_relu(getattr(self, "bn%d" % i)(getattr(self, "conv%d" % i)(x, ei)))
        return x_pos + self.linear2(self.l_relu(self.linear1(x)))


def test_teacher_forced_training_steps_of_the_modular_posnet(dev):
    """Two Adam steps of ``PosNet(fused=False, conv="feast", heads=4)`` on the icosphere, loss = mean squared distance to the clean
    vertices.  Before each step the float64 (and float32 CPU) reference module is loaded from the GPU model's state, so both see
    the SAME parameters; the loss and the full parameter gradient are compared.  Every parameter's gradient is part of the
    concatenated vector (and its own figure is printed); the assertion is on the whole vector because a conv bias in front of a
    BatchNorm has a gradient that is zero in exact arithmetic -- rounding noise in all three evaluations, with no meaningful
    relative error of its own.  The bound is the yardstick's: 4x the float32 CPU reference's own distance from float64."""
    from dual_dmp_amd.engine import POS_WIDTHS
    from dual_dmp_amd.networks import PosNet
    from dual_dmp_amd.nn_ops import FeaStConv
    gt, noisy, smooth, data = OJ.case("ico3")
    torch.manual_seed(6)
    net = PosNet(dev, fused=False, conv="feast", heads=4)
    assert isinstance(net.conv7, FeaStConv)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    target = torch.tensor(np.asarray(gt.vs), dtype=torch.float64)
    z1, x_pos, ei = data.z1.detach().cpu(), data.x_pos.detach().cpu(), data.edge_index.cpu()
    td = target.float().to(dev)

    def ref_eval(dtype):
        r = _RefPosNet(POS_WIDTHS, 4, dtype)
        r.load_state_dict({k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu())
                           for k, v in net.state_dict().items()})
        r.train()
        loss = ((r(z1.to(dtype), x_pos.to(dtype), ei) - target.to(dtype)) ** 2).mean()
        loss.backward()
        return float(loss.detach()), {k: p.grad for k, p in r.named_parameters()}

    for step in range(2):
        opt.zero_grad()
        loss = ((net(data) - td) ** 2).mean()
        loss.backward()
        l64, g64 = ref_eval(torch.float64)
        l32, g32 = ref_eval(torch.float32)
        got = {k: p.grad for k, p in net.named_parameters()}
        assert sorted(got) == sorted(g64) and all(got[k] is not None and got[k].shape == g64[k].shape for k in got)
        for k in sorted(got):
            print("step %d %-20s gradient rel-L2 %.2e (float32 CPU %.2e; norm %.2e)" % (step, k, relerr(got[k], g64[k]),
                                                                                      relerr(g32[k], g64[k]), float(g64[k].norm())))
        cat = lambda d: torch.cat([d[k].reshape(-1).double().cpu() for k in sorted(got)])
        el, yl = abs(float(loss.detach()) - l64) / l64, abs(l32 - l64) / l64
        eg, yg = relerr(cat(got), cat(g64)), relerr(cat(g32), cat(g64))
        print("step %d: loss %.6f rel %.2e (yardstick %.2e, bound %.2e), gradient rel-L2 %.2e (yardstick %.2e, bound %.2e)"
              % (step, l64, el, yl, bound(yl), eg, yg, bound(yg)))
        assert el <= bound(yl) and eg <= bound(yg), (step, el, yl, eg, yg)
        opt.step()


def test_normalnet_runs_with_conv_feast(dev):
    from dual_dmp_amd.networks import NormalNet
    from dual_dmp_amd.nn_ops import FeaStConv
    gt, noisy, smooth, data = OJ.case("ico3")
    torch.manual_seed(6)
    net = NormalNet(dev, fused=False, conv="feast", heads=4)
    assert isinstance(net.conv7, FeaStConv)
    net.train()
    o = net(data)
    assert o.shape == (len(noisy.faces), 3) and bool(torch.isfinite(o).all())
    o.backward(torch.randn(len(noisy.faces), 3, device=dev))
    for name, p in net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name


# ------------------------------------------------------------------------------------------------ 4. reproducibility
def test_two_runs_give_the_same_bits(dev, graphs):
    from dual_dmp_amd.nn_ops import FeaStConv
    ei, n = graphs["hub"]
    eid = ei.to(dev)
    for cin, cout, heads in ((32, 40, 3), (16, 4, 8), (3, 3, 2), (64, 64, 4)):
        torch.manual_seed(1)
        conv = FeaStConv(cin, cout, heads=heads).to(dev)
        x, t = torch.randn(n, cin, device=dev), torch.randn(n, cout, device=dev)
        a = [v.clone() for v in _operator_run(conv, x, eid, t)[0]]
        b = _operator_run(conv, x, eid, t)[0]
        for k, u, v in zip(NAMES, a, b):
            assert torch.equal(u, v), (cin, cout, heads, k)


# ------------------------------------------------------------------------------------------------ 5. index width
def test_offsets_beyond_2_31_bytes(dev):
    """1,100,000-node vertex graph of a torus, heads x C = 4 x 128: the gathered rows [N, 512] (+ the P columns, in one row
    buffer) span N * 516 * 4 bytes = 2.27e9 > 2^31.  Forward and backward once; from the GPU's own Hf and P, y and dHf of 2,000
    sampled rows are recomputed in float64 on the CPU from their one-ring neighbourhoods and compared at the operator tolerance."""
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
    x, wgt = torch.randn(n, cin, device=dev), torch.randn(hc + heads, cin, device=dev) * 0.3
    cvec = torch.randn(heads, device=dev) * 0.5
    buf = ops.gemm_nt(x, wgt)                                    # [N, 516] = [Hf | P]
    hf, p = buf[:, :hc], buf[:, hc:]
    dout = torch.randn(n, C, device=dev)
    y, beta = ops.feast_fwd(g, hf, p, cvec, heads)
    dz, rs = ops.feast_bwd_edge(g, dout, hf, beta, heads)
    gbuf = torch.empty(n, hc + heads, device=dev)
    dhf, dp = ops.feast_bwd_node(g, dout, beta, dz, rs, heads, out=gbuf)
    torch.cuda.synchronize()
    # sampled rows, the last rows among them: the largest offsets
    rng = np.random.default_rng(0)
    s0 = np.unique(np.concatenate([rng.choice(n - 10, 1990, replace=False), np.arange(n - 10, n)]))
    assert len(s0) == 2000
    ent = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in s0])
    cnt = rowptr[s0 + 1] - rowptr[s0]
    erow, ecol = np.repeat(s0, cnt), col[ent]                    # (no duplicate edges: every multiplicity is 1, deg = entries)
    i0 = torch.from_numpy(np.repeat(np.arange(len(s0)), cnt))
    fetch = lambda m, r: m[torch.from_numpy(r).to(dev)].double().cpu()
    c64 = cvec.double().cpu()
    # y[i] = (1 / deg_i) sum_{j in row i} sum_h softmax_h(P[j] - P[i] + c) Hf[j, h]
    q = torch.softmax(fetch(p, ecol) - fetch(p, erow) + c64, 1)
    msg = (q.unsqueeze(-1) * fetch(hf, ecol).view(-1, heads, C)).sum(1)
    y_ref = torch.zeros((len(s0), C), dtype=torch.float64).index_add_(0, i0, msg) / torch.from_numpy(cnt).double().unsqueeze(1)
    # dHf[j, h] = sum_{i in row j} softmax_h(P[j] - P[i] + c)[h] / deg_i dOut[i]   (symmetric structure: row j lists its targets)
    qt = torch.softmax(fetch(p, erow) - fetch(p, ecol) + c64, 1) / torch.from_numpy(rowptr[ecol + 1] - rowptr[ecol]).double().unsqueeze(1)
    dh_ref = torch.zeros((len(s0), heads, C), dtype=torch.float64).index_add_(0, i0, qt.unsqueeze(-1) * fetch(dout, ecol).unsqueeze(1))
    rows0 = torch.from_numpy(s0).to(dev)
    e_y, e_d = relerr(y[rows0], y_ref), relerr(dhf[rows0].reshape(-1, heads, C), dh_ref)
    print("1.1M nodes x (4 x 128): y rel-L2 %.2e, dHf rel-L2 %.2e over %d sampled rows (tolerance %.0e)" % (e_y, e_d, len(s0), OP_TOL))
    assert e_y <= OP_TOL and e_d <= OP_TOL
    assert bool(torch.isfinite(dp[rows0]).all())

"""TransformerConv on the GPU: the dot-product attention kernels (scores + edge softmax + gather + skip, the two backward launches)
and the drop-in against the float64 edge-list reference (tests/transformer_ref.py) on the graphs of test_gpu_gat.py: the
icosphere (ragged last chunk), the open grid (boundary) and the hub graph (one 1200-entry row), with duplicate edges and explicit
loops on top, and the "-iso" variants for an empty row.  No self loops are added anywhere.

Tolerance policy (that of test_gpu_gat.py), every comparison against the float64 reference:
* y, dQ, dK, dV, dx and the parameter gradients: the project's operator tolerance, rel-L2 <= 1e-5;
* alpha and dz have no project tolerance: the yardstick is the float32 CPU evaluation of the same reference against its float64
  evaluation on the same inputs, the bound 4x that and not below 16 float32 epsilons.  Both figures are printed.
* ONE quantity has no relative error of its own: the gradient of ``lin_key.bias`` is ZERO in exact arithmetic (the bias adds
  ``Q[i,h,:] . bk[h,:]`` to every score of row i, and a softmax does not see a constant), so the reference, its float32 evaluation
  and the device all hold rounding noise.  Its error is taken relative to the norm of its sibling of the same shape and scale, the
  gradient of ``lin_query.bias`` (both are column sums of blocks of one gradient row buffer), and held to the operator tolerance
  in that measure."""
import math

import numpy as np
import pytest
import torch

import edge_weight_route_worker as W
import oracle_jobs as OJ
from test_gpu_gat import FLOOR, OP_TOL, bound, dev, entry_map, graphs  # noqa: F401  (dev, graphs: the fixtures)
from test_gpu_gatv2 import CASES
from transformer_ref import TransformerConvRef, transformer_core

pytestmark = pytest.mark.gpu
relerr = W.relerr

# CASES, (in, C per head, heads): scalar kernels | one lane per head | two lanes per head, last pass partly invalid | four lanes
# per head, last pass partly invalid | eight lanes per head | ragged q loop | wide head
assert [(c[1], c[2]) for c in CASES] == [(3, 2), (4, 8), (8, 3), (16, 3), (32, 1), (40, 3), (64, 4)]


# ------------------------------------------------------------------------------------------------ 1. the kernels
def kernel_reference(q, k, v, skip, dout, ei, n, heads, dtype):
    """Everything the kernels produce, from the edge-list reference in ``dtype`` with Q, K, V and the skip as the inputs."""
    q, k, v = (t.to(dtype).requires_grad_(True) for t in (q, k, v))
    m, aux = transformer_core(q, k, v, ei, heads, True, full=True)
    y = m + skip.to(dtype)
    (y * dout.to(dtype)).sum().backward()
    _, rows, ent = entry_map(ei, n, False, aux["src"], aux["dst"])
    nnz = len(rows)
    alpha = torch.zeros((nnz, heads), dtype=dtype).index_add_(0, ent, aux["alpha"].detach())
    dz = torch.zeros((nnz, heads), dtype=dtype).index_add_(0, ent, aux["z"].grad)
    return dict(y=y.detach(), alpha=alpha, dz=dz, dq=q.grad, dk=k.grad, dv=v.grad), rows


@pytest.mark.parametrize("name", ["ico", "grid", "hub", "grid-iso", "hub-iso"])
@pytest.mark.parametrize("C,heads", [(c[1], c[2]) for c in CASES])
def test_kernels_match_the_reference(dev, graphs, name, C, heads):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    gen = torch.Generator().manual_seed(n + C)
    hc = heads * C
    q, k, v, skip, dout = (torch.randn(n, hc, generator=gen) for _ in range(5))
    ref, rows = kernel_reference(q, k, v, skip, dout, ei, n, heads, torch.float64)
    r32, _ = kernel_reference(q, k, v, skip, dout, ei, n, heads, torch.float32)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    assert g.nnz == len(rows)
    qd, kd, vd, sd, doutd = (t.to(dev) for t in (q, k, v, skip, dout))
    got = {}
    got["y"], got["alpha"] = ops.tconv_fwd(g, qd, kd, vd, heads, skip=sd)
    got["dz"], got["dq"] = ops.tconv_bwd_edge(g, doutd, kd, vd, got["alpha"], heads)
    got["dk"], got["dv"] = ops.tconv_bwd_node(g, doutd, qd, got["alpha"], got["dz"], heads)
    torch.cuda.synchronize()
    # each row's alpha sums to 1 per head, to 0 on an empty row
    sums = torch.zeros((n, heads), dtype=torch.float64).index_add_(0, rows, got["alpha"].double().cpu())
    empty = torch.from_numpy(np.bincount(rows.numpy(), minlength=n) == 0)
    assert bool(empty.any()) == name.endswith("-iso")
    assert float((sums[~empty] - 1).abs().max()) < 1e-5 and float(sums[empty].abs().max() if empty.any() else 0.0) == 0.0
    if empty.any():
        assert torch.equal(got["y"].cpu()[empty], skip[empty])                          # zero aggregate plus the skip row
        assert not got["dq"].cpu()[empty].any()
    for key in ("y", "dq", "dk", "dv"):
        e = relerr(got[key], ref[key])
        print("%s C=%d heads=%d %s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)" % (name, C, heads, key, e, OP_TOL,
                                                                                      relerr(r32[key], ref[key])))
        assert e <= OP_TOL, (key, e)
    for key in ("alpha", "dz"):
        e, yard = relerr(got[key], ref[key]), relerr(r32[key], ref[key])
        print("%s C=%d heads=%d %s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (name, C, heads, key, e, yard, bound(yard)))
        assert e <= bound(yard), (key, e, yard)


def test_no_skip_and_an_explicit_scale(dev, graphs):
    """``skip=None`` gives y - skip of the call with it (a zero start of the same sum: the same bits as a zero skip), and ``scale``
    is what multiplies the dot product."""
    from dual_dmp_amd import ops
    ei, n = graphs["grid-iso"]
    heads, C = 3, 8
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(5)
    q, k, v = (torch.randn(n, heads * C, device=dev) for _ in range(3))
    y0, a0 = ops.tconv_fwd(g, q, k, v, heads)
    y1, a1 = ops.tconv_fwd(g, q, k, v, heads, skip=torch.zeros_like(q))
    assert torch.equal(y0, y1) and torch.equal(a0, a1)
    y2, a2 = ops.tconv_fwd(g, q * 2, k, v, heads, scale=0.5 / math.sqrt(C))                  # (powers of two: exact)
    assert torch.equal(y0, y2) and torch.equal(a0, a2)
    with pytest.raises(ops.DdmpError):
        ops.tconv_fwd(g, q, k, v, heads, out=q)                                          # an output aliasing an input


# ------------------------------------------------------------------------------------------------ 2. column blocks and aliasing
@pytest.mark.parametrize("C,heads", [(8, 3), (3, 2)])
def test_column_blocks_of_one_row_buffer_and_the_shared_operand(dev, graphs, C, heads):
    """Q, K, V and S as column blocks of a packed [Q | K | V | S] buffer, outputs into column blocks of one gradient buffer, and
    one block passed as K and V, give the bits of the contiguous calls; dS is dOut."""
    from dual_dmp_amd import ops
    ei, n = graphs["ico-iso"]
    hc = heads * C
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(3)
    buf, dout = torch.randn(n, 4 * hc, device=dev), torch.randn(n, hc, device=dev)
    blk = lambda i: buf[:, i * hc:(i + 1) * hc]
    for iq, ik, iv in ((0, 1, 2), (0, 1, 1)):
        q, k, v, s = blk(iq), blk(ik), blk(iv), blk(3)
        cq, ck, cv, cs = (t.contiguous() for t in (q, k, v, s))
        y, alpha = ops.tconv_fwd(g, q, k, v, heads, skip=s)
        y2, alpha2 = ops.tconv_fwd(g, cq, ck, cv, heads, skip=cs)
        assert torch.equal(y, y2) and torch.equal(alpha, alpha2)
        gbuf = torch.full((n, 4 * hc), float("nan"), device=dev)
        dz, dq = ops.tconv_bwd_edge(g, dout, k, v, alpha, heads, out=gbuf[:, :hc])
        dk, dv = ops.tconv_bwd_node(g, dout, q, alpha, dz, heads, out_k=gbuf[:, hc:2 * hc], out_v=gbuf[:, 2 * hc:3 * hc],
                                    out_s=gbuf[:, 3 * hc:])
        dz2, dq2 = ops.tconv_bwd_edge(g, dout, ck, cv, alpha2, heads)
        dk2, dv2 = ops.tconv_bwd_node(g, dout, cq, alpha2, dz2, heads)
        assert torch.equal(dz, dz2) and torch.equal(gbuf[:, :hc], dq2)
        assert torch.equal(gbuf[:, hc:2 * hc], dk2) and torch.equal(gbuf[:, 2 * hc:3 * hc], dv2)
        assert torch.equal(gbuf[:, 3 * hc:], dout)
        assert dq.data_ptr() == gbuf.data_ptr() and dk.data_ptr() == gbuf[:, hc:].data_ptr() and dv.data_ptr() == gbuf[:, 2 * hc:].data_ptr()


# ------------------------------------------------------------------------------------------------ 3. the operator
PNAMES = ("lin_query.weight", "lin_query.bias", "lin_key.weight", "lin_key.bias", "lin_value.weight", "lin_value.bias",
          "lin_skip.weight", "lin_skip.bias", "lin_beta.weight")
MODES = [(True, True, False), (False, True, False), (True, False, False), (True, True, True), (False, True, True)]


def _named(conv):
    have = dict(conv.named_parameters())
    if not conv.root_weight:                                     # lin_skip exists but takes no part
        have = {k: v for k, v in have.items() if not k.startswith("lin_skip")}
    return [(k, have[k]) for k in PNAMES if k in have]


def _operator_run(conv, x, ei, t):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, ei)
    (y * t).sum().backward()
    return dict([("y", y.detach()), ("dx", x.grad)] + [("d " + k, p.grad) for k, p in _named(conv)])


def operr(key, got, ref):
    """rel-L2 of ``got[key]``; for the gradient of ``lin_key.bias`` relative to the norm of the gradient of ``lin_query.bias``
    (module docstring)."""
    if key != "d lin_key.bias":
        return relerr(got[key], ref[key])
    d = got[key].detach().double().cpu() - ref[key].detach().double().cpu()
    return float(d.norm() / ref["d lin_query.bias"].detach().double().norm())


@pytest.mark.parametrize("cin,cout,heads", CASES)
@pytest.mark.parametrize("concat,root,beta", MODES)
@pytest.mark.parametrize("name", ["hub", "ico-iso"])
def test_operator_matches_the_float64_reference(dev, graphs, cin, cout, heads, concat, root, beta, name):
    from dual_dmp_amd.nn_ops import TransformerConv
    ei, n = graphs[name]
    torch.manual_seed(cin + heads)
    conv = TransformerConv(cin, cout, heads=heads, concat=concat, beta=beta, root_weight=root)
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, cin, generator=gen)
    t = torch.randn(n, heads * cout if concat else cout, generator=gen)
    refs = {dtype: TransformerConvRef(cin, cout, heads, concat, beta, root_weight=root, dtype=dtype).load_from(conv)
            for dtype in (torch.float64, torch.float32)}
    conv.to(dev)
    got = _operator_run(conv, x.to(dev), ei.to(dev), t.to(dev))
    r64, r32 = (_operator_run(refs[dtype], x.to(dtype), ei, t.to(dtype)) for dtype in (torch.float64, torch.float32))
    assert list(got) == list(r64) and len(got) == 8 + (2 if root else 0) + (1 if beta else 0)
    assert all(v is not None for v in got.values())
    for key in got:
        assert got[key].shape == r64[key].shape, key
        e, yard = operr(key, got, r64), operr(key, r32, r64)
        print("%s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)" % (key, e, OP_TOL, yard))
        assert e <= OP_TOL, (key, e)
    if not root:
        assert conv.lin_skip.weight.grad is None


# ------------------------------------------------------------------------------------------------ 4. reproducibility
def test_two_runs_give_the_same_bits(dev, graphs):
    from dual_dmp_amd.nn_ops import TransformerConv
    ei, n = graphs["hub"]
    eid = ei.to(dev)
    for (cin, cout, heads), beta in (((32, 40, 3), False), ((8, 16, 3), True), ((3, 3, 2), False)):
        torch.manual_seed(1)
        conv = TransformerConv(cin, cout, heads=heads, beta=beta).to(dev)
        x, t = torch.randn(n, cin, device=dev), torch.randn(n, heads * cout, device=dev)
        a = {k: v.clone() for k, v in _operator_run(conv, x, eid, t).items()}
        b = _operator_run(conv, x, eid, t)
        for k in a:
            assert torch.equal(a[k], b[k]), (cin, cout, heads, k)


# ------------------------------------------------------------------------------------------------ 5. training
class _TwoLayer(torch.nn.Module):
    def __init__(self, mk):
        super().__init__()
        self.c1, self.c2 = mk(8, 8, 2), mk(16, 3, 1)

    def forward(self, x, ei):
        return self.c2(torch.relu(self.c1(x, ei)), ei)


def test_short_training_loop(dev, graphs):
    """10 Adam steps of a two-layer graph transformer regressing a fixed target on "ico": the loss falls; for the first 3 steps the
    loss and the full parameter gradient stay within the yardstick-derived bound of the float64 reference evaluated at the SAME
    parameters (teacher-forced: the reference is loaded from the GPU model before every compared step)."""
    from dual_dmp_amd.nn_ops import TransformerConv
    ei, n = graphs["ico"]
    gen = torch.Generator().manual_seed(4)
    x, target = torch.randn(n, 8, generator=gen), torch.randn(n, 3, generator=gen)
    torch.manual_seed(4)
    net = _TwoLayer(lambda i, o, h: TransformerConv(i, o, heads=h)).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    xd, td, eid = x.to(dev), target.to(dev), ei.to(dev)
    cat = lambda m: torch.cat([p.grad.reshape(-1) for c in (m.c1, m.c2) for _, p in _named(c)])

    def ref_eval(dtype):
        r = _TwoLayer(lambda i, o, h: TransformerConvRef(i, o, h, dtype=dtype))
        r.c1.load_from(net.c1), r.c2.load_from(net.c2)
        loss = ((r(x.to(dtype), ei) - target.to(dtype)) ** 2).mean()
        loss.backward()
        return float(loss.detach()), cat(r)

    losses = []
    for step in range(10):
        opt.zero_grad()
        loss = ((net(xd, eid) - td) ** 2).mean()
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
    """Two Adam steps of ``PosNet(dev, fused=False, conv="transformer", heads=4)`` on the icosphere, loss = mean squared distance
    to the clean vertices: finite, and decreasing."""
    from dual_dmp_amd.networks import PosNet
    from dual_dmp_amd.nn_ops import TransformerConv
    gt, noisy, smooth, data = OJ.case("ico3")
    torch.manual_seed(6)
    net = PosNet(dev, fused=False, conv="transformer", heads=4)
    assert isinstance(net.conv7, TransformerConv)
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


# ------------------------------------------------------------------------------------------------ 6. index width
def two_ring_reference(rowptr, col, s0, fetch_q, fetch_k, fetch_v, fetch_dout, heads, C):
    """m, dQ, dK and dV of the rows ``s0`` in float64 from rows of Q, K, V and dOut alone (``fetch_*``: row ids -> float64 CPU
    rows), on a graph without duplicate edges: ring 1 = the rows s0 references (whose softmax, delta and dz are needed in full),
    ring 2 = those rows' columns (whose K and V are needed).  Written per entry, without the mirror map."""
    span = lambda rows: np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows])
    s1 = np.unique(np.concatenate([col[span(s0)], s0]))
    ent = span(s1)
    erow, ecol = np.repeat(s1, rowptr[s1 + 1] - rowptr[s1]), col[ent]
    s2 = np.unique(np.concatenate([ecol, s1]))
    i1, i2 = torch.from_numpy(np.searchsorted(s1, erow)), torch.from_numpy(np.searchsorted(s2, ecol))
    Q = fetch_q(s1).view(len(s1), heads, C)
    D = fetch_dout(s1).view(len(s1), heads, C)
    K = fetch_k(s2).view(len(s2), heads, C)
    V = fetch_v(s2).view(len(s2), heads, C)
    zero = lambda k: torch.zeros((k, heads), dtype=torch.float64)
    scale = 1.0 / math.sqrt(C)
    z = scale * (Q[i1] * K[i2]).sum(-1)
    m = torch.full((len(s1), heads), -float("inf"), dtype=torch.float64).scatter_reduce(0, i1.view(-1, 1).expand(-1, heads), z, "amax")
    ex = torch.exp(z - m[i1])                                     # (no duplicate edges: every multiplicity is 1)
    al = ex / zero(len(s1)).index_add_(0, i1, ex)[i1]
    dal = (D[i1] * V[i2]).sum(-1)
    delta = zero(len(s1)).index_add_(0, i1, al * dal)
    dz = al * (dal - delta[i1])
    big = lambda k: torch.zeros((k, heads, C), dtype=torch.float64)
    m_ref = big(len(s1)).index_add_(0, i1, al.unsqueeze(-1) * V[i2])
    dq_ref = scale * big(len(s1)).index_add_(0, i1, dz.unsqueeze(-1) * K[i2])
    dk_ref = scale * big(len(s2)).index_add_(0, i2, dz.unsqueeze(-1) * Q[i1])
    dv_ref = big(len(s2)).index_add_(0, i2, al.unsqueeze(-1) * D[i1])
    p1, p2 = torch.from_numpy(np.searchsorted(s1, s0)), torch.from_numpy(np.searchsorted(s2, s0))
    return m_ref[p1], dq_ref[p1], dk_ref[p2], dv_ref[p2]


def test_offsets_beyond_2_31_bytes(dev):
    """1,100,000-node vertex graph of a torus, heads * C = 4 * 32 = 128: Q, K, V and S are the column blocks of ONE [N, 512] row
    buffer of N * 512 * 4 bytes = 2.25e9 > 2^31, and the gradients go into the column blocks of another.  Forward and both
    backward launches once; from the GPU's own buffer, the y, dQ, dK and dV of 600 sampled rows (the last 10 among them) are
    recomputed in float64 on the CPU from their two-ring neighbourhoods and compared at the operator tolerance."""
    from dual_dmp_amd import ops, synth
    heads, C, cin = 4, 32, 16
    hc = heads * C
    v, f = synth.torus(1100, 1000)
    n = len(v)
    assert n == 1100000 and n * 4 * hc * 4 > 2 ** 31
    f = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // n, key % n])).contiguous()
    t = ops.csr_build_valued_host(ei.numpy(), n, 0)
    rowptr, col = t["rowptr"].astype(np.int64), t["col"].astype(np.int64)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(7)
    x, wgt = torch.randn(n, cin, device=dev), torch.randn(4 * hc, cin, device=dev) * 0.3
    buf = ops.gemm_nt(x, wgt)
    assert buf.shape == (n, 512) and buf.is_contiguous()
    q, k, vv, s = (buf[:, i * hc:(i + 1) * hc] for i in range(4))
    dout = torch.randn(n, hc, device=dev)
    y, alpha = ops.tconv_fwd(g, q, k, vv, heads, skip=s)
    gbuf = torch.empty(n, 4 * hc, device=dev)
    dz, dq = ops.tconv_bwd_edge(g, dout, k, vv, alpha, heads, out=gbuf[:, :hc])
    dk, dv = ops.tconv_bwd_node(g, dout, q, alpha, dz, heads, out_k=gbuf[:, hc:2 * hc], out_v=gbuf[:, 2 * hc:3 * hc],
                                out_s=gbuf[:, 3 * hc:])
    torch.cuda.synchronize()
    # sampled rows, the last rows among them: the largest offsets
    rng = np.random.default_rng(0)
    s0 = np.unique(np.concatenate([rng.choice(n - 10, 590, replace=False), np.arange(n - 10, n)]))
    assert len(s0) == 600
    fetch = lambda m: (lambda r: m[torch.from_numpy(r).to(dev)].double().cpu())
    m_ref, dq_ref, dk_ref, dv_ref = two_ring_reference(rowptr, col, s0, fetch(q), fetch(k), fetch(vv), fetch(dout), heads, C)
    rows0 = torch.from_numpy(s0).to(dev)
    y_ref = m_ref + fetch(s)(s0).view(-1, heads, C)
    errs = [relerr(a[rows0].reshape(-1, heads, C), b) for a, b in ((y, y_ref), (dq, dq_ref), (dk, dk_ref), (dv, dv_ref))]
    print("1.1M nodes x [N, 512] row buffer: y rel-L2 %.2e, dQ %.2e, dK %.2e, dV %.2e over %d sampled rows (tolerance %.0e)"
          % (errs[0], errs[1], errs[2], errs[3], len(s0), OP_TOL))
    assert max(errs) <= OP_TOL
    assert torch.equal(gbuf[rows0, 3 * hc:], dout[rows0])                                # dS is dOut

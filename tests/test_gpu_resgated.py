"""ResGatedGraphConv on the GPU: the per-channel gate kernels (gate + gather + skip + bias, the two backward launches that recompute
the gate) and the drop-in against the float64 edge-list reference (tests/resgated_ref.py) on the graphs of test_gpu_gat.py: the
icosphere (ragged last chunk), the open grid (boundary) and the hub graph (one 1200-entry row), with duplicate edges and explicit
loops on top, and the "-iso" variants for an empty row.  No self loops are added anywhere.

Tolerance policy (that of test_gpu_gat.py), every comparison against the float64 reference: y, dK, dQ, dV, dx and the parameter
gradients hold the project's operator tolerance, rel-L2 <= 1e-5; the float32 CPU evaluation of the same reference is printed
beside every figure.  The training loop's loss and full gradient have no project tolerance: ``bound(yardstick)`` of
test_gpu_gat.py."""
import math

import numpy as np
import pytest
import torch

import oracle_jobs as OJ
from resgated_ref import ResGatedGraphConvRef, resgated_core
from test_gpu_gat import OP_TOL, bound, dev, graphs, relerr  # noqa: F401  (dev, graphs: the fixtures)

pytestmark = pytest.mark.gpu

# scalar kernels | one float4, 7 idle lanes | two | exactly one q step | ragged q loop | two q steps
WIDTHS = [3, 4, 8, 32, 40, 64]


# ------------------------------------------------------------------------------------------------ 1. the kernels
def kernel_reference(k, q, v, skip, bias, dout, ei, dtype):
    """Everything the kernels produce, from the edge-list reference in ``dtype`` with K, Q, V, the skip and the bias as inputs."""
    k, q, v = (t.to(dtype).requires_grad_(True) for t in (k, q, v))
    y = resgated_core(k, q, v, ei) + skip.to(dtype) + bias.to(dtype)
    (y * dout.to(dtype)).sum().backward()
    return dict(y=y.detach(), dk=k.grad, dq=q.grad, dv=v.grad)


def kernel_run(ops, g, k, q, v, skip, bias, dout):
    got = dict(y=ops.rgate_fwd(g, k, q, v, skip=skip, bias=bias), dk=ops.rgate_bwd_row(g, dout, k, q, v))
    got["dq"], got["dv"] = ops.rgate_bwd_node(g, dout, k, q, v)
    torch.cuda.synchronize()
    return got


def check_kernels(tag, got, ref, r32, keys=("y", "dk", "dq", "dv")):
    for key in keys:
        e = relerr(got[key], ref[key])
        print("%s %s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)" % (tag, key, e, OP_TOL, relerr(r32[key], ref[key])))
        assert e <= OP_TOL, (key, e)


@pytest.mark.parametrize("name", ["ico", "grid", "hub", "grid-iso", "hub-iso"])
@pytest.mark.parametrize("C", WIDTHS)
def test_kernels_match_the_reference(dev, graphs, name, C):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    gen = torch.Generator().manual_seed(n + C)
    k, q, v, skip, dout = (torch.randn(n, C, generator=gen) for _ in range(5))
    bias = torch.randn(C, generator=gen)
    ref = kernel_reference(k, q, v, skip, bias, dout, ei, torch.float64)
    r32 = kernel_reference(k, q, v, skip, bias, dout, ei, torch.float32)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    got = kernel_run(ops, g, *(t.to(dev) for t in (k, q, v, skip, bias, dout)))
    empty = torch.from_numpy(np.bincount(ei[1].numpy(), minlength=n) == 0)
    assert bool(empty.any()) == name.endswith("-iso")
    if empty.any():
        assert torch.equal(got["y"].cpu()[empty], (skip + bias)[empty])                 # the init exactly, bit for bit
        assert not got["dk"].cpu()[empty].any()
    check_kernels("%s C=%d" % (name, C), got, ref, r32)


# ------------------------------------------------------------------------------------------------ 2. asymmetric multiplicities
@pytest.mark.parametrize("C", [3, 8])
def test_asymmetric_multiplicities(dev, graphs, C):
    """"grid" plus one-directional duplicates of existing edges: the structure stays symmetric, the multiplicities do not, and
    the node side has to read the multiplicity of the MIRRORED entry (with ``mult[e]`` dQ and dV miss the tolerance)."""
    from dual_dmp_amd import ops
    ei, n = graphs["grid"]
    ei = torch.cat([ei, ei[:, 100:107], ei[:, 100:103], ei[:, 300:304]], 1).contiguous()
    t = ops.csr_build_valued_host(ei.numpy(), n, 0)
    a = ops.valued_values_host(t, None, 0)[0]
    assert int((a != a[t["mirror"]]).sum()) >= 10                                       # asymmetric indeed
    gen = torch.Generator().manual_seed(C)
    k, q, v, skip, dout = (torch.randn(n, C, generator=gen) for _ in range(5))
    bias = torch.randn(C, generator=gen)
    ref = kernel_reference(k, q, v, skip, bias, dout, ei, torch.float64)
    r32 = kernel_reference(k, q, v, skip, bias, dout, ei, torch.float32)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    got = kernel_run(ops, g, *(t_.to(dev) for t_ in (k, q, v, skip, bias, dout)))
    check_kernels("grid+asym C=%d" % C, got, ref, r32)


# ------------------------------------------------------------------------------------------------ 3. saturation
@pytest.mark.parametrize("C", [3, 40])
def test_saturated_gates_stay_finite(dev, graphs, C):
    """One row in eight of K and of Q times 60: gate arguments of a few hundred either way, where exp overflows.  Every output is
    finite and the operator tolerance holds (the error norms are carried by the unsaturated rows)."""
    from dual_dmp_amd import ops
    ei, n = graphs["hub"]
    gen = torch.Generator().manual_seed(C + 1)
    k, q, v, skip, dout = (torch.randn(n, C, generator=gen) for _ in range(5))
    bias = torch.randn(C, generator=gen)
    k[::8] *= 60
    q[3::8] *= 60
    assert float((k[ei[1]] + q[ei[0]]).abs().max()) > 100
    ref = kernel_reference(k, q, v, skip, bias, dout, ei, torch.float64)
    r32 = kernel_reference(k, q, v, skip, bias, dout, ei, torch.float32)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    got = kernel_run(ops, g, *(t.to(dev) for t in (k, q, v, skip, bias, dout)))
    for key, val in got.items():
        assert bool(torch.isfinite(val).all()), key
    check_kernels("hub saturated C=%d" % C, got, ref, r32)


# ------------------------------------------------------------------------------------------------ 4. options
@pytest.mark.parametrize("C", [3, 8])
def test_no_skip_no_bias_and_aliasing(dev, graphs, C):
    """``skip=None`` / ``bias=None`` give the bits of zero tensors in their place; an output that is one of the inputs (or another
    output) raises."""
    from dual_dmp_amd import ops
    ei, n = graphs["grid-iso"]
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(5)
    k, q, v, skip, dout = (torch.randn(n, C, device=dev) for _ in range(5))
    bias = torch.randn(C, device=dev)
    zs, zb = torch.zeros_like(skip), torch.zeros_like(bias)
    assert torch.equal(ops.rgate_fwd(g, k, q, v), ops.rgate_fwd(g, k, q, v, skip=zs, bias=zb))
    assert torch.equal(ops.rgate_fwd(g, k, q, v, skip=skip), ops.rgate_fwd(g, k, q, v, skip=skip, bias=zb))
    assert torch.equal(ops.rgate_fwd(g, k, q, v, bias=bias), ops.rgate_fwd(g, k, q, v, skip=zs, bias=bias))
    for t in (k, q, v, skip):
        with pytest.raises(ops.DdmpError):
            ops.rgate_fwd(g, k, q, v, skip=skip, out=t)
    for t in (dout, k, q, v):
        with pytest.raises(ops.DdmpError):
            ops.rgate_bwd_row(g, dout, k, q, v, out=t)
        with pytest.raises(ops.DdmpError):
            ops.rgate_bwd_node(g, dout, k, q, v, out_q=t)
        with pytest.raises(ops.DdmpError):
            ops.rgate_bwd_node(g, dout, k, q, v, out_v=t)
        with pytest.raises(ops.DdmpError):
            ops.rgate_bwd_node(g, dout, k, q, v, out_s=t)
    o = torch.empty_like(k)
    for kw in (dict(out_q=o, out_v=o), dict(out_q=o, out_s=o), dict(out_v=o, out_s=o)):
        with pytest.raises(ops.DdmpError):
            ops.rgate_bwd_node(g, dout, k, q, v, **kw)
    with pytest.raises(ops.DdmpError):
        ops.rgate_fwd(g, k, q, v[:, :C - 1])                                            # widths differ


# ------------------------------------------------------------------------------------------------ 5. column blocks
@pytest.mark.parametrize("C", [8, 3])
def test_column_blocks_of_one_row_buffer(dev, graphs, C):
    """K, Q, V and S as column blocks of a packed [K | Q | V | S] buffer, outputs into column blocks of one NaN-prefilled gradient
    buffer, give the bits of the contiguous calls; dS is dOut."""
    from dual_dmp_amd import ops
    ei, n = graphs["ico-iso"]
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(3)
    buf, dout, bias = torch.randn(n, 4 * C, device=dev), torch.randn(n, C, device=dev), torch.randn(C, device=dev)
    k, q, v, s = (buf[:, i * C:(i + 1) * C] for i in range(4))
    ck, cq, cv, cs = (t.contiguous() for t in (k, q, v, s))
    assert torch.equal(ops.rgate_fwd(g, k, q, v, skip=s, bias=bias), ops.rgate_fwd(g, ck, cq, cv, skip=cs, bias=bias))
    gbuf = torch.full((n, 4 * C), float("nan"), device=dev)
    dk = ops.rgate_bwd_row(g, dout, k, q, v, out=gbuf[:, :C])
    dq, dv = ops.rgate_bwd_node(g, dout, k, q, v, out_q=gbuf[:, C:2 * C], out_v=gbuf[:, 2 * C:3 * C], out_s=gbuf[:, 3 * C:])
    dk2 = ops.rgate_bwd_row(g, dout, ck, cq, cv)
    dq2, dv2 = ops.rgate_bwd_node(g, dout, ck, cq, cv)
    assert torch.equal(gbuf[:, :C], dk2) and torch.equal(gbuf[:, C:2 * C], dq2) and torch.equal(gbuf[:, 2 * C:3 * C], dv2)
    assert torch.equal(gbuf[:, 3 * C:], dout)                                           # dS is dOut
    assert dk.data_ptr() == gbuf.data_ptr() and dq.data_ptr() == gbuf[:, C:].data_ptr() and dv.data_ptr() == gbuf[:, 2 * C:].data_ptr()


# ------------------------------------------------------------------------------------------------ 6. the operator
PNAMES = ("lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight", "lin_value.bias",
          "lin_skip.weight", "bias")


def _named(conv):
    have = dict(conv.named_parameters())
    return [(k, have[k]) for k in PNAMES if k in have]


def _operator_run(conv, x, ei, t):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, ei)
    (y * t).sum().backward()
    return dict([("y", y.detach()), ("dx", x.grad)] + [("d " + k, p.grad) for k, p in _named(conv)])


@pytest.mark.parametrize("cin,cout", [(3, 3), (16, 8), (32, 40), (64, 64)])
@pytest.mark.parametrize("root", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("name", ["hub", "ico-iso"])
def test_operator_matches_the_float64_reference(dev, graphs, cin, cout, root, bias, name):
    from dual_dmp_amd.nn_ops import ResGatedGraphConv
    ei, n = graphs[name]
    torch.manual_seed(cin + cout)
    conv = ResGatedGraphConv(cin, cout, root_weight=root, bias=bias)
    if bias:
        with torch.no_grad():
            conv.bias.uniform_(-0.5, 0.5)                        # (zeros at initialisation: give it something to add)
    gen = torch.Generator().manual_seed(n)
    x, t = torch.randn(n, cin, generator=gen), torch.randn(n, cout, generator=gen)
    refs = {dtype: ResGatedGraphConvRef(cin, cout, root_weight=root, bias=bias, dtype=dtype).load_from(conv)
            for dtype in (torch.float64, torch.float32)}
    conv.to(dev)
    got = _operator_run(conv, x.to(dev), ei.to(dev), t.to(dev))
    r64, r32 = (_operator_run(refs[dtype], x.to(dtype), ei, t.to(dtype)) for dtype in (torch.float64, torch.float32))
    assert list(got) == list(r64) and len(got) == 8 + (1 if root else 0) + (1 if bias else 0)
    assert all(v is not None for v in got.values())
    for key in got:
        assert got[key].shape == r64[key].shape, key
        e = relerr(got[key], r64[key])
        print("%s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)" % (key, e, OP_TOL, relerr(r32[key], r64[key])))
        assert e <= OP_TOL, (key, e)
    assert (conv.lin_skip is None) == (not root) and (conv.bias is None) == (not bias)
    if name == "ico-iso":                                        # the node without incoming edges: lin_skip(x_i) + bias
        want = (x[-1].double() @ refs[torch.float64].lin_skip.weight.t() if root else torch.zeros(cout, dtype=torch.float64))
        want = (want + (refs[torch.float64].bias if bias else 0.0)).detach()
        assert float((got["y"][-1].double().cpu() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))


def test_unused_parameters_keep_no_gradient(dev, graphs):
    """A frozen parameter and an x that does not require grad get no gradient (``needs_input_grad``)."""
    from dual_dmp_amd.nn_ops import ResGatedGraphConv
    ei, n = graphs["grid"]
    torch.manual_seed(2)
    conv = ResGatedGraphConv(8, 8).to(dev)
    conv.lin_skip.weight.requires_grad_(False)
    conv.lin_query.bias.requires_grad_(False)
    x = torch.randn(n, 8, device=dev)
    conv(x, ei.to(dev)).sum().backward()
    assert x.grad is None and conv.lin_skip.weight.grad is None and conv.lin_query.bias.grad is None
    assert all(p.grad is not None for p in conv.parameters() if p.requires_grad)


# ------------------------------------------------------------------------------------------------ 7. reproducibility
def test_two_runs_give_the_same_bits(dev, graphs):
    from dual_dmp_amd.nn_ops import ResGatedGraphConv
    ei, n = graphs["hub"]
    eid = ei.to(dev)
    for cin, cout in ((32, 40), (8, 64), (3, 3)):
        torch.manual_seed(1)
        conv = ResGatedGraphConv(cin, cout).to(dev)
        x, t = torch.randn(n, cin, device=dev), torch.randn(n, cout, device=dev)
        a = {k: v.clone() for k, v in _operator_run(conv, x, eid, t).items()}
        b = _operator_run(conv, x, eid, t)
        for k in a:
            assert torch.equal(a[k], b[k]), (cin, cout, k)


# ------------------------------------------------------------------------------------------------ 8. training
class _TwoLayer(torch.nn.Module):
    def __init__(self, mk):
        super().__init__()
        self.c1, self.c2 = mk(8, 16), mk(16, 3)

    def forward(self, x, ei):
        return self.c2(torch.relu(self.c1(x, ei)), ei)


def test_short_training_loop(dev, graphs):
    """10 Adam steps of a two-layer residual gated net regressing a fixed target on "ico": the loss falls; for the first 3 steps
    the loss and the full parameter gradient stay within the yardstick-derived bound of the float64 reference evaluated at the
    SAME parameters (teacher-forced: the reference is loaded from the GPU model before every compared step)."""
    from dual_dmp_amd.nn_ops import ResGatedGraphConv
    ei, n = graphs["ico"]
    gen = torch.Generator().manual_seed(4)
    x, target = torch.randn(n, 8, generator=gen), torch.randn(n, 3, generator=gen)
    torch.manual_seed(4)
    net = _TwoLayer(lambda i, o: ResGatedGraphConv(i, o)).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    xd, td, eid = x.to(dev), target.to(dev), ei.to(dev)
    cat = lambda m: torch.cat([p.grad.reshape(-1) for c in (m.c1, m.c2) for _, p in _named(c)])

    def ref_eval(dtype):
        r = _TwoLayer(lambda i, o: ResGatedGraphConvRef(i, o, dtype=dtype))
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
    """Two Adam steps of ``PosNet(dev, fused=False, conv="resgated")`` on the icosphere, loss = mean squared distance to the clean
    vertices: finite, and decreasing."""
    from dual_dmp_amd.networks import PosNet
    from dual_dmp_amd.nn_ops import ResGatedGraphConv
    gt, noisy, smooth, data = OJ.case("ico3")
    torch.manual_seed(6)
    net = PosNet(dev, fused=False, conv="resgated")
    assert isinstance(net.conv7, ResGatedGraphConv)
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


# ------------------------------------------------------------------------------------------------ 9. index width
def one_ring_reference(rowptr, col, s0, fetch_k, fetch_q, fetch_v, fetch_dout):
    """The gathered sum, dK, dQ and dV of the rows ``s0`` in float64 from rows of K, Q, V and dOut alone (``fetch_*``: row ids ->
    float64 CPU rows), on a symmetric graph without duplicate edges (every multiplicity is 1).  There is no softmax, so the
    rows' own entries suffice: row i's entries are its sources j, and -- the structure being symmetric -- also the targets it
    feeds.  Written per entry, without the mirror map."""
    ent = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in s0])
    erow, ecol = np.repeat(s0, rowptr[s0 + 1] - rowptr[s0]), col[ent]
    s1 = np.unique(np.concatenate([ecol, s0]))
    i0, i1 = torch.from_numpy(np.searchsorted(s0, erow)), torch.from_numpy(np.searchsorted(s1, ecol))
    own = torch.from_numpy(np.searchsorted(s1, s0))
    K, Q, V, D = fetch_k(s1), fetch_q(s1), fetch_v(s1), fetch_dout(s1)
    zero = torch.zeros((len(s0), K.shape[1]), dtype=torch.float64)
    # the row as a TARGET i = erow, its entries the sources j = ecol
    gt = torch.sigmoid(K[own][i0] + Q[i1])
    m = zero.clone().index_add_(0, i0, gt * V[i1])
    dk = zero.clone().index_add_(0, i0, D[own][i0] * V[i1] * gt * (1 - gt))
    # the row as a SOURCE j = erow, its entries the targets i = ecol
    gs = torch.sigmoid(K[i1] + Q[own][i0])
    dq = zero.clone().index_add_(0, i0, D[i1] * V[own][i0] * gs * (1 - gs))
    dv = zero.clone().index_add_(0, i0, D[i1] * gs)
    return m, dk, dq, dv


def test_offsets_beyond_2_31_bytes(dev):
    """1,100,000-node vertex graph of a torus, C = 128: K, Q, V and S are the column blocks of ONE [N, 512] row buffer of
    N * 512 * 4 bytes = 2.25e9 > 2^31, and the gradients go into the column blocks of another.  Forward and both backward
    launches once; from the GPU's own buffer, the y, dK, dQ and dV of 600 sampled rows (the last 10 among them) are recomputed in
    float64 on the CPU from their one-ring neighbourhoods and compared at the operator tolerance."""
    from dual_dmp_amd import ops, synth
    C, cin = 128, 16
    v, f = synth.torus(1100, 1000)
    n = len(v)
    assert n == 1100000 and n * 4 * C * 4 > 2 ** 31
    f = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // n, key % n])).contiguous()
    t = ops.csr_build_valued_host(ei.numpy(), n, 0)
    rowptr, col = t["rowptr"].astype(np.int64), t["col"].astype(np.int64)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(7)
    x, wgt = torch.randn(n, cin, device=dev), torch.randn(4 * C, cin, device=dev) * 0.3
    buf = ops.gemm_nt(x, wgt)
    assert buf.shape == (n, 512) and buf.is_contiguous()
    k, q, vv, s = (buf[:, i * C:(i + 1) * C] for i in range(4))
    dout, bias = torch.randn(n, C, device=dev), torch.randn(C, device=dev)
    y = ops.rgate_fwd(g, k, q, vv, skip=s, bias=bias)
    gbuf = torch.empty(n, 4 * C, device=dev)
    dk = ops.rgate_bwd_row(g, dout, k, q, vv, out=gbuf[:, :C])
    dq, dv = ops.rgate_bwd_node(g, dout, k, q, vv, out_q=gbuf[:, C:2 * C], out_v=gbuf[:, 2 * C:3 * C], out_s=gbuf[:, 3 * C:])
    torch.cuda.synchronize()
    # sampled rows, the last rows among them: the largest offsets
    rng = np.random.default_rng(0)
    s0 = np.unique(np.concatenate([rng.choice(n - 10, 590, replace=False), np.arange(n - 10, n)]))
    assert len(s0) == 600
    fetch = lambda m: (lambda r: m[torch.from_numpy(r).to(dev)].double().cpu())
    m_ref, dk_ref, dq_ref, dv_ref = one_ring_reference(rowptr, col, s0, fetch(k), fetch(q), fetch(vv), fetch(dout))
    rows0 = torch.from_numpy(s0).to(dev)
    y_ref = m_ref + fetch(s)(s0) + bias.double().cpu()
    errs = [relerr(a[rows0], b) for a, b in ((y, y_ref), (dk, dk_ref), (dq, dq_ref), (dv, dv_ref))]
    print("1.1M nodes x [N, 512] row buffer: y rel-L2 %.2e, dK %.2e, dQ %.2e, dV %.2e over %d sampled rows (tolerance %.0e)"
          % (errs[0], errs[1], errs[2], errs[3], len(s0), OP_TOL))
    assert max(errs) <= OP_TOL
    assert torch.equal(gbuf[rows0, 3 * C:], dout[rows0])                                # dS is dOut

"""EdgeConv on the GPU: the arg-max gather and its backward (``ops.gather_max`` / ``ops.gather_max_bwd``) and the drop-in against
the float64 edge-list reference (tests/edgeconv_ref.py) on the icosphere (ragged last chunk), the open grid (boundary) and the hub
graph (one 1200-entry row), with duplicate edges and explicit loops on top, and with one edgeless node.

Tolerance policy:
* kernel level, on exact float32 A, B, dG: y is one maximum and one add, so it must equal torch's float32 ``A + segment_max(B)``
  bit for bit; arg must be the smallest source id that attains the maximum; dA is a copy, bit for bit; dB differs from a float64
  sum over the kernel's own arg only in the summation order: the project's gather tolerance, rel-L2 <= 1e-6;
* operator level, against ``EdgeConvRef`` in float64: near-ties make the winner ill-conditioned -- a float32 evaluation may
  legitimately pick the other neighbour and move a whole dG[i, c].  An output (i, c) whose float64 top-two gap of B is below
  1e-3 x rms(B) is called ambiguous; dG is zeroed there on both sides, the ambiguous share must stay <= 1 % (printed), arg must
  equal the reference winner at every other output, and y, dx, dW, db meet the project's operator tolerance, rel-L2 <= 1e-5."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import edge_weight_route_worker as W
import oracle_jobs as OJ
from edgeconv_ref import EdgeConvRef, winners_and_gaps

pytestmark = pytest.mark.gpu
relerr = W.relerr

OP_TOL = 1e-5
GATHER_TOL = 1e-6
AMB_GAP = 1e-3                  # x rms(B)
AMB_SHARE = 0.01

CASES = [(3, 3), (16, 4), (8, 32), (32, 40), (64, 64)]          # (in, out): scalar path, float4 path, a ragged packed width


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graphs():
    """name -> (edge_index, n): the route worker's graphs + duplicates and explicit loops (two on node 5); "<name>-iso": one more
    node without any edge (an empty row: EdgeConv adds no loops)."""
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


def host_csr(ei, n):
    """(rows, cols) int64 of the coalesced CSR entries in CSR order, empty [n] bool."""
    from dual_dmp_amd import ops
    t = ops.csr_build_valued_host(ei.numpy(), n, 0)
    cnt = np.diff(t["rowptr"])
    return torch.from_numpy(np.repeat(np.arange(n), cnt)), torch.from_numpy(t["col"].astype(np.int64)), torch.from_numpy(cnt == 0)


def segment_max_f32(b, rows, cols, n):
    """torch's float32 maximum of b[cols] over each row's entries; -inf for a row without entries."""
    idx = rows.view(-1, 1).expand(-1, b.shape[1])
    return torch.full((n, b.shape[1]), -float("inf")).scatter_reduce(0, idx, b[cols], "amax")


def db_from_arg(dg, arg, rows, cols, n):
    """float64 dB from a given arg: dB[j, c] = sum over the entries (j, i) of row j of dG[i, c] where arg[i, c] == j."""
    hit = arg.long()[cols] == rows.view(-1, 1)
    return torch.zeros((n, dg.shape[1]), dtype=torch.float64).index_add_(0, rows, torch.where(hit, dg.double()[cols], torch.zeros((), dtype=torch.float64)))


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("name", ["ico", "grid", "hub", "ico-iso", "hub-iso"])
@pytest.mark.parametrize("C", [c[1] for c in CASES])
def test_kernels_match_torch(dev, graphs, name, C):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    gen = torch.Generator().manual_seed(n + C)
    a, b, dg = (torch.randn(n, C, generator=gen) for _ in range(3))
    rows, cols, empty = host_csr(ei, n)
    assert bool(empty.any()) == name.endswith("-iso")
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    assert g.nnz == len(rows)
    cp = (C + 3) // 4 * 4                                        # the operator's layout: one row buffer [A | pad | B | pad]
    buf = torch.zeros(n, 2 * cp, device=dev)
    buf[:, :C], buf[:, cp:cp + C] = a.to(dev), b.to(dev)
    ad, bd, dgd = buf[:, :C], buf[:, cp:cp + C], dg.to(dev)
    y, arg = ops.gather_max(g, bd, a=ad)
    y_noarg, none = ops.gather_max(g, bd, a=ad, want_arg=False)
    y_noa, arg_noa = ops.gather_max(g, bd)
    gbuf = torch.full((n, 2 * cp), float("nan"), device=dev)
    da, db = ops.gather_max_bwd(g, dgd, arg, out=gbuf)
    torch.cuda.synchronize()
    assert y.shape == (n, C) and arg.shape == (n, C) and arg.dtype == torch.int32 and none is None
    assert da.shape == db.shape == (n, C) and da.data_ptr() == gbuf.data_ptr()
    y, arg, da, db = y.cpu(), arg.cpu(), da.cpu(), db.cpu()
    mx = segment_max_f32(b, rows, cols, n)
    e2 = empty.view(-1, 1)
    zero = torch.zeros(())
    assert torch.equal(y, torch.where(e2, zero, a + mx))         # bit for bit; an empty row gets 0, not A
    assert torch.equal(y_noarg.cpu(), y) and torch.equal(y_noa.cpu(), torch.where(e2, zero, mx)) and torch.equal(arg_noa.cpu(), arg)
    ref_arg, _, ref_empty = winners_and_gaps(b, ei, n)
    assert torch.equal(ref_empty, empty)
    ne = ~empty
    assert torch.equal(b.gather(0, arg.long()[ne]), mx[ne])      # B[arg[i, c], c] is the row maximum ...
    assert torch.equal(arg.long(), ref_arg)                      # ... arg the smallest such id, -1 on an empty row
    assert bool((arg[empty] == -1).all())
    assert torch.equal(da, torch.where(e2, zero, dg))
    e = relerr(db, db_from_arg(dg, arg, rows, cols, n))
    print("%s C=%d dB: rel-L2 %.2e (tolerance %.0e)" % (name, C, e, GATHER_TOL))
    assert e <= GATHER_TOL
    pad = torch.ones(2 * cp, dtype=torch.bool)
    pad[:C], pad[cp:cp + C] = False, False
    assert bool(torch.isnan(gbuf[:, pad.to(dev)]).all()) and bool(torch.isfinite(gbuf[:, (~pad).to(dev)]).all())


@pytest.mark.parametrize("C", [3, 8])
def test_ties_go_to_the_first_entry(dev, graphs, C):
    """All rows of B equal: every entry ties, the first entry in CSR order (the smallest source id) wins, and the whole of
    dG[i] lands on it."""
    from dual_dmp_amd import ops
    ei, n = graphs["hub-iso"]
    rows, cols, empty = host_csr(ei, n)
    gen = torch.Generator().manual_seed(C)
    a, dg = torch.randn(n, C, generator=gen), torch.randn(n, C, generator=gen)
    b = torch.randn(1, C, generator=gen).expand(n, C).contiguous()
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    y, arg = ops.gather_max(g, b.to(dev), a=a.to(dev))
    da, db = ops.gather_max_bwd(g, dg.to(dev), arg)
    ne = ~empty
    assert bool((cols[1:] > cols[:-1])[rows[1:] == rows[:-1]].all())          # CSR order ascends: the first entry is the smallest id
    first = torch.full((n,), n, dtype=torch.int64).scatter_reduce(0, rows, cols, "amin")
    first[empty] = -1
    assert torch.equal(y.cpu()[ne], (a + b)[ne]) and torch.equal(arg.cpu().long(), first.view(-1, 1).expand(-1, C))
    want = torch.zeros((n, C), dtype=torch.float64).index_add_(0, first[ne], dg[ne].double())
    assert relerr(db, want) <= GATHER_TOL
    assert torch.allclose(db.double().cpu().sum(0), dg[ne].double().sum(0), atol=1e-4)


def test_bad_arguments_are_refused(dev, graphs):
    from dual_dmp_amd import ops
    ei, n = graphs["grid"]
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    plain = ops.graph_for(ei.to(dev), n)                         # not a valued graph
    b = torch.randn(n, 8, device=dev)
    with pytest.raises(ops.DdmpError):
        ops.gather_max(plain, b)
    with pytest.raises(ops.DdmpError):
        ops.gather_max(g, b[: n - 1])
    with pytest.raises(ops.DdmpError):
        ops.gather_max(g, b, a=torch.randn(n, 4, device=dev))
    with pytest.raises(ops.DdmpError):
        ops.gather_max(g, b.cpu())
    y, arg = ops.gather_max(g, b)
    with pytest.raises(ops.DdmpError):
        ops.gather_max_bwd(g, b, arg.long())
    with pytest.raises(ops.DdmpError):
        ops.gather_max_bwd(g, b, arg, out=torch.empty(n, 8, device=dev))
    import ctypes
    L = ops._lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops._stream()
    assert L.ddmp_gather_max_f32(None, p(b), 8, None, 0, 8, p(y), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_f32(plain.handle, p(b), 8, None, 0, 8, p(y), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_f32(g.handle, p(b), 8, None, 0, 0, p(y), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_f32(g.handle, p(b), 4, None, 0, 8, p(y), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_bwd_f32(g.handle, p(b), 8, p(arg), 4, 8, p(y), 8, p(y), 8, st) != 0


# ------------------------------------------------------------------------------------------------ 2. the operator
def _make_fn(cin, cout, kind, gen):
    a = 1.0 / math.sqrt(2 * cin)
    lin = nn.Linear(2 * cin, cout, bias=kind != "nobias")
    with torch.no_grad():
        for p in lin.parameters():
            p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * a)
    return nn.Sequential(lin, nn.LeakyReLU(0.2)) if kind == "leaky" else lin


def _lin_of(fn):
    return fn[0] if isinstance(fn, nn.Sequential) else fn


def _run(conv, x, ei, t):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, ei)
    (y * t).sum().backward()
    return [y.detach(), x.grad] + [p.grad for p in conv.parameters()]


def _record_arg(monkeypatch):
    """Every arg ``ops.gather_max`` returns from here on, in call order."""
    from dual_dmp_amd import ops
    args, real = [], ops.gather_max

    def recording(*a, **kw):
        y, arg = real(*a, **kw)
        args.append(arg)
        return y, arg

    monkeypatch.setattr(ops, "gather_max", recording)
    return args


@pytest.mark.parametrize("cin,cout", CASES)
@pytest.mark.parametrize("name", ["ico-iso", "grid", "hub-iso"])
@pytest.mark.parametrize("kind", ["bias", "nobias", "leaky"])
def test_operator_matches_the_float64_reference(dev, graphs, monkeypatch, cin, cout, name, kind):
    from dual_dmp_amd.nn_ops import EdgeConv
    ei, n = graphs[name]
    gen = torch.Generator().manual_seed(n + cout)
    x = torch.randn(n, cin, generator=gen)
    fn = _make_fn(cin, cout, kind, gen)
    t = torch.randn(n, cout, generator=gen)
    ref = EdgeConvRef(fn)
    b64 = x.double() @ _lin_of(ref.nn).weight.detach()[:, cin:].t()
    ref_arg, gap, _ = winners_and_gaps(b64, ei, n)
    amb = gap < AMB_GAP * float(b64.pow(2).mean().sqrt())
    share = float(amb.double().mean())
    print("%s (%d, %d) %s: ambiguous share %.3f %% (limit %.0f %%), smallest gap %.1e rms" % (name, cin, cout, kind, 100 * share, 100 * AMB_SHARE, float(gap.min() / b64.pow(2).mean().sqrt())))
    assert share <= AMB_SHARE
    t = t.masked_fill(amb, 0.0)
    want = _run(ref, x.double(), ei, t.double())
    args = _record_arg(monkeypatch)
    conv = EdgeConv(fn).to(dev)
    got = _run(conv, x.to(dev), ei.to(dev), t.to(dev))
    assert len(args) == 1 and torch.equal(args[0].cpu().long()[~amb], ref_arg[~amb])
    names = ("y", "dx", "dW", "db")
    assert len(got) == len(want) == (3 if kind == "nobias" else 4)
    for k, a, b in zip(names, got, want):
        assert a.shape == b.shape, k
        e = relerr(a, b)
        print("%s: rel-L2 %.2e (tolerance %.0e)" % (k, e, OP_TOL))
        assert e <= OP_TOL, (k, e)


def test_no_grad_forward_keeps_no_arg(dev, graphs, monkeypatch):
    from dual_dmp_amd.nn_ops import EdgeConv
    ei, n = graphs["grid"]
    args = _record_arg(monkeypatch)
    conv = EdgeConv(nn.Linear(16, 12)).to(dev)
    x, eid = torch.randn(n, 8, device=dev), ei.to(dev)
    with torch.no_grad():
        y0 = conv(x, eid)
    y1 = conv(x, eid)
    assert args[0] is None and args[1] is not None and torch.equal(y0, y1.detach())


# ------------------------------------------------------------------------------------------------ 3. reproducibility
def test_two_runs_give_the_same_bits(dev, graphs, monkeypatch):
    from dual_dmp_amd.nn_ops import EdgeConv
    ei, n = graphs["hub"]
    eid = ei.to(dev)
    args = _record_arg(monkeypatch)
    for cin, cout in CASES:
        torch.manual_seed(1)
        conv = EdgeConv(nn.Sequential(nn.Linear(2 * cin, cout), nn.LeakyReLU(0.2))).to(dev)
        x, t = torch.randn(n, cin, device=dev), torch.randn(n, cout, device=dev)
        del args[:]
        a = [v.clone() for v in _run(conv, x, eid, t)]
        b = _run(conv, x, eid, t)
        assert len(a) == 4 and torch.equal(args[0], args[1])
        for k, u, v in zip(("y", "dx", "dW", "db"), a, b):
            assert torch.equal(u, v), (cin, cout, k)


# ------------------------------------------------------------------------------------------------ 4. index width
def test_offsets_beyond_2_31_bytes(dev):
    """1,100,000-node vertex graph of a torus, C = 256, A and B the halves of one [N, 512] buffer: N * 512 * 4 bytes = 2.25e9 >
    2^31.  Forward and backward once; y, arg, dA and dB of 2,000 sampled rows are recomputed on the CPU from their one-ring
    neighbourhoods."""
    from dual_dmp_amd import ops, synth
    C = 256
    v, f = synth.torus(1100, 1000)
    n = len(v)
    assert n == 1100000 and n * 2 * C * 4 > 2 ** 31
    f = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // n, key % n])).contiguous()
    t = ops.csr_build_valued_host(ei.numpy(), n, 0)
    rowptr, col = t["rowptr"].astype(np.int64), t["col"].astype(np.int64)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(7)
    buf = torch.randn(n, 2 * C, device=dev)
    a, b = buf[:, :C], buf[:, C:]
    dg = torch.randn(n, C, device=dev)
    y, arg = ops.gather_max(g, b, a=a)
    gbuf = torch.empty(n, 2 * C, device=dev)
    da, db = ops.gather_max_bwd(g, dg, arg, out=gbuf)
    torch.cuda.synchronize()
    # sampled rows, the last rows among them: the largest offsets
    rng = np.random.default_rng(0)
    s0 = np.unique(np.concatenate([rng.choice(n - 10, 1990, replace=False), np.arange(n - 10, n)]))
    assert len(s0) == 2000
    ent = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in s0])
    cnt = rowptr[s0 + 1] - rowptr[s0]
    assert cnt.min() > 0
    erow, ecol = np.repeat(s0, cnt), col[ent]
    i0 = torch.from_numpy(np.repeat(np.arange(len(s0)), cnt))
    fetch = lambda m, r: m[torch.from_numpy(r).to(dev)].cpu()
    idx = i0.view(-1, 1).expand(-1, C)
    bj = fetch(b, ecol)
    mx = torch.full((len(s0), C), -float("inf")).scatter_reduce(0, idx, bj, "amax")
    jj = torch.from_numpy(ecol).view(-1, 1).expand(-1, C)
    cand = torch.where(bj == mx[i0], jj, torch.full((), n, dtype=torch.int64))
    win = torch.full((len(s0), C), n, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin")
    assert torch.equal(fetch(y, s0), fetch(a, s0) + mx) and torch.equal(fetch(arg, s0).long(), win)
    assert torch.equal(fetch(da, s0), fetch(dg, s0))
    hit = fetch(arg, ecol).long() == torch.from_numpy(erow).view(-1, 1)
    want = torch.zeros((len(s0), C), dtype=torch.float64).index_add_(0, i0, torch.where(hit, fetch(dg, ecol).double(), torch.zeros((), dtype=torch.float64)))
    e = relerr(fetch(db, s0), want)
    print("1.1M nodes x 256: dB rel-L2 %.2e over %d sampled rows (tolerance %.0e)" % (e, len(s0), GATHER_TOL))
    assert e <= GATHER_TOL


# ------------------------------------------------------------------------------------------------ 5. training
class _RefPosNet(torch.nn.Module):
    """The modular PosNet with EdgeConvRef layers, in ``dtype``: same parameter and buffer names as the net under test.
    ``masks=None``: the ambiguous outputs of every layer are determined from this evaluation (float64) and kept in ``self.masks``;
    the gradient that reaches a layer's ambiguous outputs is zeroed."""

    def __init__(self, widths, dtype):
        super().__init__()
        for i in range(12):
            setattr(self, "conv%d" % (i + 1), EdgeConvRef(nn.Linear(2 * widths[i], widths[i + 1]), dtype=dtype))
            setattr(self, "bn%d" % (i + 1), torch.nn.BatchNorm1d(widths[i + 1], dtype=dtype))
        self.linear1 = torch.nn.Linear(widths[12], widths[13], dtype=dtype)
        self.linear2 = torch.nn.Linear(widths[13], widths[14], dtype=dtype)
        self.l_relu = torch.nn.LeakyReLU()
        self.masks = None

    def forward(self, z1, x_pos, ei, masks=None):
        x, found = z1, []
        for i in range(1, 13):
            conv = getattr(self, "conv%d" % i)
            if masks is None:
                b = x.detach() @ conv.nn.weight.detach()[:, x.shape[1]:].t()
                gap = winners_and_gaps(b, ei, x.shape[0])[1]
                found.append(gap < AMB_GAP * float(b.pow(2).mean().sqrt()))
            m = (found if masks is None else masks)[i - 1]
            y = conv(x, ei)
            y.register_hook(lambda grad, m=m: grad.masked_fill(m, 0.0))
            x = self.l_relu(getattr(self, "bn%d" % i)(y))
        self.masks = found if masks is None else masks
        return x_pos + self.linear2(self.l_relu(self.linear1(x)))


def test_teacher_forced_training_steps_of_the_modular_posnet(dev):
    """Two Adam steps of ``PosNet(fused=False, conv="edge")`` on the icosphere, loss = mean squared distance to the clean vertices.
    Before each step the float64 (and float32 CPU) reference module is loaded from the GPU model's state, so all see the SAME
    parameters.  The ambiguity masking of the operator test is applied to the loss gradient at every layer: the float64
    evaluation determines each layer's ambiguous outputs, and the gradient reaching them is zeroed in all three evaluations.
    The share per layer is printed, not bounded: the operator test's 1 % belongs to independent random rows, while the trunk's
    features are smooth over the mesh, so neighbouring rows of B lie closer together relative to rms(B).
    The loss and the full parameter gradient (one concatenated vector: a conv bias in front of a BatchNorm has a gradient that is
    zero in exact arithmetic) must come within max(4 x the float32 CPU module's own distance from float64, 1e-5)."""
    from dual_dmp_amd.engine import POS_WIDTHS
    from dual_dmp_amd.networks import PosNet
    from dual_dmp_amd.nn_ops import EdgeConv
    gt, noisy, smooth, data = OJ.case("ico3")
    torch.manual_seed(6)
    net = PosNet(dev, fused=False, conv="edge")
    assert isinstance(net.conv7, EdgeConv)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    target = torch.tensor(np.asarray(gt.vs), dtype=torch.float64)
    z1, x_pos, ei = data.z1.detach().cpu(), data.x_pos.detach().cpu(), data.edge_index.cpu()
    td = target.float().to(dev)
    masks = []
    for i in range(12):
        getattr(net, "conv%d" % (i + 1)).register_forward_hook(
            lambda mod, inp, out, i=i: out.register_hook(lambda grad: grad.masked_fill(masks[i].to(grad.device), 0.0)) and None)

    def ref_eval(dtype, use=None):
        r = _RefPosNet(POS_WIDTHS, dtype)
        r.load_state_dict({k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu())
                           for k, v in net.state_dict().items()})
        r.train()
        loss = ((r(z1.to(dtype), x_pos.to(dtype), ei, masks=use) - target.to(dtype)) ** 2).mean()
        loss.backward()
        return float(loss.detach()), {k: p.grad for k, p in r.named_parameters()}, r.masks

    bound = lambda yard: max(4.0 * yard, OP_TOL)
    for step in range(2):
        l64, g64, found = ref_eval(torch.float64)
        masks[:] = found
        print("step %d: ambiguous share per layer (%%): %s" % (step, " ".join("%.3f" % (100 * float(m.double().mean())) for m in masks)))
        l32, g32, _ = ref_eval(torch.float32, use=found)
        opt.zero_grad()
        loss = ((net(data) - td) ** 2).mean()
        loss.backward()
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


def test_normalnet_runs_with_conv_edge(dev):
    from dual_dmp_amd.networks import NormalNet
    from dual_dmp_amd.nn_ops import EdgeConv
    gt, noisy, smooth, data = OJ.case("ico3")
    torch.manual_seed(6)
    net = NormalNet(dev, fused=False, conv="edge")
    assert isinstance(net.conv7, EdgeConv)
    net.train()
    o = net(data)
    assert o.shape == (len(noisy.faces), 3) and bool(torch.isfinite(o).all())
    o.backward(torch.randn(len(noisy.faces), 3, device=dev))
    for name, p in net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name

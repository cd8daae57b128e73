"""SAGEConv on the GPU: the fused neighbour-statistics gather and its backward (``ops.gather_stats`` / ``ops.gather_stats_bwd``) and
the drop-in against the float64 edge-list reference (tests/sage_ref.py) on the icosphere (ragged last chunk), the open grid
(boundary) and the hub graph (one 1200-entry row), with duplicate edges and explicit loops on top, and with one edgeless node.

Tolerance policy:
* kernel level, on exact float32 inputs: Mx / Mn are comparisons only, so they must equal torch's float32 segment maximum /
  minimum bit for bit; the args must be the smallest source id that attains the extremum; Xcopy and dR are copies, bit for bit;
  invdeg is one correctly rounded division of an exactly representable integer: exact; S and dX differ from a float64 evaluation
  (dX: from the kernel's own args and invdeg) only in rounding and summation order: the project's gather tolerance, rel-L2 <= 1e-6
  (``GATHER_TOL`` of test_gpu_edgeconv.py); a block of a fused call has the bits of the same block requested alone;
* operator level, against ``SAGEConvRef`` in float64: EdgeConv's near-tie policy unchanged.  An output (i, c) of a max / min block
  whose float64 top-two gap is below 1e-3 x rms(x) is called ambiguous; the gradient reaching it is zeroed on both sides, the
  ambiguous share must stay <= 1 % (printed), the arg must equal the reference winner at every other output, and y, dx, dW_l, db,
  dW_r meet the project's operator tolerance, rel-L2 <= 1e-5 (``OP_TOL``)."""
import ctypes
import itertools

import pytest
import torch

import edge_weight_route_worker as W
import gat_ops_stub
from sage_ref import SAGEConvRef, canonical, extremum_winners

pytestmark = pytest.mark.gpu
relerr = W.relerr

OP_TOL = 1e-5
GATHER_TOL = 1e-6
AMB_GAP = 1e-3                  # x rms(x)
AMB_SHARE = 0.01

WIDTHS = [3, 4, 32, 40, 64]     # the scalar path, one float4, a full slab, a ragged packed width, two slabs
CASES = [(3, 3), (16, 4), (8, 32), (32, 40), (64, 64)]          # (in, out): both GEMM orders occur
AGGRS = ["mean", "add", "max", "min", ["mean", "max"], ["add", "max", "min"]]
ids = lambda a: a if isinstance(a, str) else "+".join(a)
SUBSETS = [s for r in (1, 2, 3) for s in itertools.combinations(("sum", "max", "min"), r)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graphs():
    """name -> (edge_index, n): the route worker's graphs + duplicates and explicit loops (two on node 5), as
    test_gpu_edgeconv.py's; "<name>-iso": one more node without any edge."""
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


@pytest.fixture(scope="module")
def host(graphs):
    """name -> the HOST structure of the valued graph without loop handling (row, col, a, mirror, rowptr of the coalesced CSR)."""
    return {name: gat_ops_stub.Graph(ei, n, 0) for name, (ei, n) in graphs.items()}


def _rowsum64(h, v):
    return torch.zeros((h.n_rows,) + tuple(v.shape[1:]), dtype=torch.float64).index_add_(0, h.row, v)


def _segment(x, h, op):
    """torch's float32 maximum / minimum of x[col] over each row's entries; 0 for a row without entries."""
    idx = h.row.view(-1, 1).expand(-1, x.shape[1])
    return torch.zeros((h.n_rows, x.shape[1])).scatter_reduce(0, idx, x[h.col], op, include_self=False)


def _want(subset, summed):
    return tuple(summed if s == "sum" else s for s in subset)


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("name", ["ico", "grid", "hub", "ico-iso", "grid-iso", "hub-iso"])
@pytest.mark.parametrize("C", WIDTHS)
def test_kernels_match_torch(dev, graphs, host, name, C):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    h = host[name]
    gen = torch.Generator().manual_seed(n + C)
    x, root, ds, dmx, dmn, dx0 = (torch.randn(n, C, generator=gen) for _ in range(6))
    bias = torch.randn(C, generator=gen)
    empty = h.rowptr[1:] == h.rowptr[:-1]
    assert bool(empty.any()) == name.endswith("-iso")
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    assert g.nnz == h.nnz
    # the references, once
    deg = _rowsum64(h, h.a)
    assert float(deg.sum()) == ei.shape[1]                       # every input edge counts, duplicates and loops included
    inv32 = torch.where(empty, torch.zeros(()), 1.0 / deg.float())
    s64 = _rowsum64(h, h.a.view(-1, 1) * x.double()[h.col])
    ref = {"add": s64 + root.double() + bias.double(), "mean": s64 / deg.clamp(min=1).view(-1, 1) + root.double() + bias.double(),
           "max": _segment(x, h, "amax"), "min": _segment(x, h, "amin")}
    ref_arg = {k: extremum_winners(x, ei, n, k)[0] for k in ("max", "min")}
    xd, rd, bd = x.to(dev), root.to(dev), bias.to(dev)
    dsd, dmxd, dmnd, dx0d = ds.to(dev), dmx.to(dev), dmn.to(dev), dx0.to(dev)
    alone = {}
    for k in ("mean", "add", "max", "min"):                      # each statistic on its own
        kw = dict(root=rd, bias=bd) if k in ("mean", "add") else {}
        (blk,), (arg,), invdeg = ops.gather_stats(g, xd, want=(k,), **kw)
        alone[k] = (blk.cpu(), None if arg is None else arg.cpu())
        if k in ("max", "min"):
            assert torch.equal(alone[k][0], ref[k])              # bit for bit; an empty row gets 0
            assert torch.equal(arg.cpu().long(), ref_arg[k])     # the smallest source id attaining it, -1 on an empty row
            assert invdeg is None
        else:
            e = relerr(blk, ref[k])
            print("%s C=%d %s alone: rel-L2 %.2e (tolerance %.0e)" % (name, C, k, e, GATHER_TOL))
            assert e <= GATHER_TOL and arg is None
            assert (invdeg is None) == (k == "add")
            if k == "mean":
                assert torch.equal(invdeg.cpu(), inv32)          # exact
                inv_d = invdeg
    (y_plain,), _, _ = ops.gather_stats(g, xd, want=("add",))    # no root, no bias: an empty row gets zeros
    assert relerr(y_plain, s64) <= GATHER_TOL and bool((y_plain.cpu()[empty] == 0).all())
    for subset in SUBSETS:
        for summed in (("mean", "add") if "sum" in subset else ("add",)):
            want = _want(subset, summed)
            nb = len(want) + 1
            width = (nb * C + 3) // 4 * 4 + 4
            buf = torch.full((n, width), float("nan"), device=dev)
            kw = dict(root=rd, bias=bd) if "sum" in subset else {}
            blocks, args, invdeg = ops.gather_stats(g, xd, want=want, copy_x=True, out=buf, **kw)
            again = torch.full((n, width), float("nan"), device=dev)
            _, args2, _ = ops.gather_stats(g, xd, want=want, copy_x=True, out=again, **kw)
            torch.cuda.synchronize()
            assert len(blocks) == nb and blocks[0].data_ptr() == buf.data_ptr()
            assert bool(torch.isnan(buf[:, nb * C:]).all()) and bool(torch.isfinite(buf[:, :nb * C]).all())
            assert torch.equal(buf[:, :nb * C], again[:, :nb * C])                          # two calls, equal bits
            assert torch.equal(blocks[-1].cpu(), x)              # Xcopy: a bit-exact copy
            assert (invdeg is not None) == ("mean" in want) and (invdeg is None or torch.equal(invdeg.cpu(), inv32))
            for k, blk, arg, arg2 in zip(want, blocks, args, args2):
                assert torch.equal(blk.cpu(), alone[k][0]), (want, k)                       # the bits of the block requested alone
                assert (arg is None) == (k in ("mean", "add"))
                if arg is not None:
                    assert torch.equal(arg.cpu(), alone[k][1]) and torch.equal(arg, arg2), (want, k)
            noarg = ops.gather_stats(g, xd, want=want, want_arg=False, **kw)
            assert all(a is None for a in noarg[1]) and all(torch.equal(u, v) for u, v in zip(noarg[0], blocks))
            # the backward of this subset, from the kernel's own args and invdeg
            op, want64 = {}, dx0.double().clone()
            if "sum" in subset:
                op["ds"] = dsd
                f = h.a[h.mirror]
                if summed == "mean":
                    op["invdeg"] = inv_d
                    f = f * inv32.double()[h.col]
                want64 += _rowsum64(h, f.view(-1, 1) * ds.double()[h.col])
            for k, dm, dmd in (("max", dmx, dmxd), ("min", dmn, dmnd)):
                if k in subset:
                    arg = args[want.index(k)]
                    op["d" + ("mx" if k == "max" else "mn")], op["arg" + ("mx" if k == "max" else "mn")] = dmd, arg
                    hit = arg.cpu().long()[h.col] == h.row.view(-1, 1)
                    want64 += _rowsum64(h, torch.where(hit, dm.double()[h.col], torch.zeros((), dtype=torch.float64)))
            has_root = "sum" in subset
            gw = (1 + has_root) * C
            gbuf = torch.full((n, (gw + 3) // 4 * 4 + 4), float("nan"), device=dev)
            dx, dr = ops.gather_stats_bwd(g, dx0=dx0d, root=has_root, out=gbuf, **op)
            dx_b, dr_b = ops.gather_stats_bwd(g, dx0=dx0d, root=has_root, **op)
            torch.cuda.synchronize()
            assert dx.shape == (n, C) and dx.data_ptr() == gbuf.data_ptr() and (dr is not None) == has_root
            assert bool(torch.isnan(gbuf[:, gw:]).all()) and bool(torch.isfinite(gbuf[:, :gw]).all())
            assert torch.equal(dx, dx_b) and (dr is None or torch.equal(dr, dr_b))          # two calls, equal bits
            e = relerr(dx, want64)
            print("%s C=%d %s dX: rel-L2 %.2e (tolerance %.0e)" % (name, C, "+".join(want), e, GATHER_TOL))
            assert e <= GATHER_TOL, (want, e)
            if has_root:
                assert torch.equal(dr.cpu(), ds)                 # dR: a bit-exact copy
            dx_no0, _ = ops.gather_stats_bwd(g, **op)            # without dX0: a row without entries gets zeros
            assert relerr(dx_no0, want64 - dx0.double()) <= GATHER_TOL and bool((dx_no0.cpu()[empty] == 0).all())
            assert torch.equal(dx.cpu()[empty], dx0[empty])


@pytest.mark.parametrize("C", [3, 8])
def test_ties_go_to_the_first_entry(dev, graphs, host, C):
    """All rows of x equal: every entry ties in both extrema, the first entry in CSR order (the smallest source id) wins, and the
    whole of the gradient lands on it."""
    from dual_dmp_amd import ops
    ei, n = graphs["hub-iso"]
    h = host["hub-iso"]
    empty = h.rowptr[1:] == h.rowptr[:-1]
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(1, C, generator=gen).expand(n, C).contiguous()
    dmx, dmn = torch.randn(n, C, generator=gen), torch.randn(n, C, generator=gen)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    (mx, mn), (amx, amn), _ = ops.gather_stats(g, x.to(dev), want=("max", "min"))
    dx, _ = ops.gather_stats_bwd(g, dmx=dmx.to(dev), argmx=amx, dmn=dmn.to(dev), argmn=amn)
    ne = ~empty
    first = torch.full((n,), n, dtype=torch.int64).scatter_reduce(0, h.row, h.col, "amin")
    first[empty] = -1
    for v, a in ((mx, amx), (mn, amn)):
        assert torch.equal(v.cpu()[ne], x[ne]) and torch.equal(a.cpu().long(), first.view(-1, 1).expand(-1, C))
    want = torch.zeros((n, C), dtype=torch.float64).index_add_(0, first[ne], (dmx.double() + dmn.double())[ne])
    assert relerr(dx, want) <= GATHER_TOL


def test_bad_arguments_are_refused(dev, graphs):
    from dual_dmp_amd import ops
    ei, n = graphs["grid"]
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    plain = ops.graph_for(ei.to(dev), n)                         # not a valued graph
    loops = ops.graph_for(ei.to(dev), n, norm="gat")             # loop handling: a_e no longer counts input edges
    x = torch.randn(n, 8, device=dev)
    for bad in (plain, loops):
        with pytest.raises(ops.DdmpError):
            ops.gather_stats(bad, x)
    with pytest.raises(ops.DdmpError):
        ops.gather_stats(g, x, want=())
    with pytest.raises(ops.DdmpError):
        ops.gather_stats(g, x, want=("mean", "add"))
    with pytest.raises(ops.DdmpError):
        ops.gather_stats(g, x[: n - 1])
    with pytest.raises(ops.DdmpError):
        ops.gather_stats(g, x, root=torch.randn(n, 4, device=dev))
    with pytest.raises(ops.DdmpError):
        ops.gather_stats(g, x, want=("max",), bias=torch.randn(8, device=dev))
    with pytest.raises(ops.DdmpError):
        ops.gather_stats(g, x, want=("mean", "max"), out=torch.empty(n, 12, device=dev))
    with pytest.raises(ops.DdmpError):
        ops.gather_stats(g, x.cpu())
    (s, mx), (_, amx), invdeg = ops.gather_stats(g, x, want=("mean", "max"))
    with pytest.raises(ops.DdmpError):
        ops.gather_stats_bwd(g)
    with pytest.raises(ops.DdmpError):
        ops.gather_stats_bwd(g, dmx=x)                           # dmx without argmx
    with pytest.raises(ops.DdmpError):
        ops.gather_stats_bwd(g, dmx=x, argmx=amx.long())
    with pytest.raises(ops.DdmpError):
        ops.gather_stats_bwd(g, dmx=x, argmx=amx, invdeg=invdeg)                            # invdeg without ds
    with pytest.raises(ops.DdmpError):
        ops.gather_stats_bwd(g, ds=x, dx0=torch.randn(n, 4, device=dev))
    with pytest.raises(ops.DdmpError):
        ops.gather_stats_bwd(g, ds=x, root=True, out=torch.empty(n, 8, device=dev))
    L = ops._lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops._stream()
    y, y2 = torch.empty_like(x), torch.empty_like(x)
    fwd = lambda gh, C=8, ldx=8, mean=0, S=p(y), lds=8, Mx=None, argmx=None: L.ddmp_gather_stats_f32(
        gh, p(x), ldx, C, mean, None, 0, None, S, lds, Mx, 8, argmx, 8, None, 0, None, 0, None, None, 0, st)
    assert fwd(g.handle) == 0
    assert fwd(None) != 0 and fwd(plain.handle) != 0 and fwd(loops.handle) != 0
    assert fwd(g.handle, S=None) != 0                            # nothing requested
    assert fwd(g.handle, S=None, mean=1, Mx=p(y2)) != 0          # mean without S
    assert fwd(g.handle, S=None, argmx=p(amx)) != 0              # an arg without its block
    assert fwd(g.handle, C=0) != 0 and fwd(g.handle, ldx=4) != 0 and fwd(g.handle, lds=4) != 0
    assert fwd(g.handle, S=p(x)) != 0                            # an output aliases X
    bwd = lambda gh, C=8, dS=p(x), ldds=8, dMx=None, argmx=None, dX=p(y), lddx=8: L.ddmp_gather_stats_bwd_f32(
        gh, C, dS, ldds, None, dMx, 8, argmx, 8, None, 0, None, 0, None, 0, dX, lddx, None, 0, st)
    assert bwd(g.handle) == 0
    assert bwd(None) != 0 and bwd(plain.handle) != 0 and bwd(loops.handle) != 0
    assert bwd(g.handle, dS=None) != 0 and bwd(g.handle, dMx=p(y2)) != 0 and bwd(g.handle, C=0) != 0
    assert bwd(g.handle, ldds=4) != 0 and bwd(g.handle, lddx=4) != 0 and bwd(g.handle, dX=p(x)) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the operator
def _record(monkeypatch, masks):
    """Every ``ops.gather_stats`` result from here on, in call order; and the gradients reaching the ambiguous outputs of the
    max / min blocks (``masks``: {"max": bool [n, in], "min": ...}) are zeroed before ``ops.gather_stats_bwd`` runs."""
    from dual_dmp_amd import ops
    seen, fwd, bwd = [], ops.gather_stats, ops.gather_stats_bwd

    def recording(*a, **kw):
        out = fwd(*a, **kw)
        seen.append((tuple(kw.get("want", ("mean",))), out))
        return out

    def masking(g, **kw):
        for key, k in (("dmx", "max"), ("dmn", "min")):
            if kw.get(key) is not None:
                kw[key] = kw[key].masked_fill(masks[k].to(kw[key].device), 0.0)
        return bwd(g, **kw)

    monkeypatch.setattr(ops, "gather_stats", recording)
    monkeypatch.setattr(ops, "gather_stats_bwd", masking)
    return seen


def _run(conv, x, ei, t):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, ei)
    (y * t).sum().backward()
    return [y.detach(), x.grad] + [p.grad for p in conv.parameters()]


@pytest.mark.parametrize("cin,cout", CASES)
@pytest.mark.parametrize("name", ["ico-iso", "grid", "hub-iso"])
@pytest.mark.parametrize("aggr", AGGRS, ids=ids)
def test_operator_matches_the_float64_reference(dev, graphs, monkeypatch, cin, cout, name, aggr):
    from dual_dmp_amd.nn_ops import SAGEConv
    ei, n = graphs[name]
    gen = torch.Generator().manual_seed(n + cin)
    x = torch.randn(n, cin, generator=gen)
    t = torch.randn(n, cout, generator=gen)
    torch.manual_seed(n + cout)
    ref = SAGEConvRef(cin, cout, aggr)
    names = canonical(aggr)
    rms = float(x.double().pow(2).mean().sqrt())
    masks, winners = {}, {}
    for k in names:
        if k in ("max", "min"):
            winners[k], gap, _ = extremum_winners(x.double(), ei, n, k)
            masks[k] = gap < AMB_GAP * rms
            share = float(masks[k].double().mean())
            print("%s (%d, %d) %s: ambiguous share of %s %.3f %% (limit %.0f %%), smallest gap %.1e rms"
                  % (name, cin, cout, ids(aggr), k, 100 * share, 100 * AMB_SHARE, float(gap.min()) / rms))
            assert share <= AMB_SHARE
    ref.on_block = lambda k, b: b.register_hook(lambda grad, k=k: grad.masked_fill(masks[k], 0.0)) if k in masks else None
    want = _run(ref, x.double(), ei, t.double())
    seen = _record(monkeypatch, masks)
    conv = SAGEConv(cin, cout, aggr=aggr).to(dev)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    got = _run(conv, x.to(dev), ei.to(dev), t.to(dev))
    assert len(seen) == 1 and seen[0][0] == names
    for k, arg in zip(names, seen[0][1][1]):
        if k in masks:
            assert torch.equal(arg.cpu().long()[~masks[k]], winners[k][~masks[k]]), k
    assert len(got) == len(want) == 5
    for k, a, b in zip(("y", "dx", "dW_l", "db", "dW_r"), got, want):
        assert a.shape == b.shape, k
        e = relerr(a, b)
        print("%s: rel-L2 %.2e (tolerance %.0e)" % (k, e, OP_TOL))
        assert e <= OP_TOL, (k, e)


@pytest.mark.parametrize("kw", [dict(normalize=True), dict(root_weight=False), dict(bias=False), dict(root_weight=False, bias=False)],
                         ids=lambda kw: "+".join(sorted(kw)))
@pytest.mark.parametrize("aggr,cin,cout", [("mean", 16, 4), ("mean", 8, 32), (["mean", "max"], 8, 32)], ids=str)
def test_options_match_the_float64_reference(dev, graphs, monkeypatch, kw, aggr, cin, cout):
    from dual_dmp_amd.nn_ops import SAGEConv
    ei, n = graphs["grid-iso"]
    gen = torch.Generator().manual_seed(n + cin)
    x, t = torch.randn(n, cin, generator=gen), torch.randn(n, cout, generator=gen)
    torch.manual_seed(5)
    ref = SAGEConvRef(cin, cout, aggr, **kw)
    masks = {}
    if "max" in aggr:
        gap = extremum_winners(x.double(), ei, n, "max")[1]
        masks["max"] = gap < AMB_GAP * float(x.double().pow(2).mean().sqrt())
        assert float(masks["max"].double().mean()) <= AMB_SHARE
    ref.on_block = lambda k, b: b.register_hook(lambda grad, k=k: grad.masked_fill(masks[k], 0.0)) if k in masks else None
    want = _run(ref, x.double(), ei, t.double())
    _record(monkeypatch, masks)
    conv = SAGEConv(cin, cout, aggr=aggr, **kw).to(dev)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    got = _run(conv, x.to(dev), ei.to(dev), t.to(dev))
    assert len(got) == len(want) == 2 + len(list(conv.parameters()))
    for a, b in zip(got, want):
        e = relerr(a, b)
        print("%s: rel-L2 %.2e (tolerance %.0e)" % (tuple(a.shape), e, OP_TOL))
        assert a.shape == b.shape and e <= OP_TOL, e


def test_no_grad_forward_keeps_no_arg_and_two_runs_give_the_same_bits(dev, graphs, monkeypatch):
    from dual_dmp_amd.nn_ops import SAGEConv
    ei, n = graphs["hub"]
    eid = ei.to(dev)
    seen = _record(monkeypatch, {"max": torch.zeros((), dtype=torch.bool), "min": torch.zeros((), dtype=torch.bool)})
    for cin, cout in CASES:
        torch.manual_seed(1)
        conv = SAGEConv(cin, cout, aggr=["add", "max", "min"]).to(dev)
        x, t = torch.randn(n, cin, device=dev), torch.randn(n, cout, device=dev)
        del seen[:]
        with torch.no_grad():
            y0 = conv(x, eid)
        a = [v.clone() for v in _run(conv, x, eid, t)]
        b = _run(conv, x, eid, t)
        assert all(arg is None for arg in seen[0][1][1]) and seen[1][1][1][1] is not None and torch.equal(y0, a[0])
        for k, u, v in zip(("y", "dx", "dW_l", "db", "dW_r"), a, b):
            assert torch.equal(u, v), (cin, cout, k)


# ------------------------------------------------------------------------------------------------ 3. training
class _Net(torch.nn.Module):
    def __init__(self, make):
        super().__init__()
        self.conv1, self.conv2, self.act = make(3, 16), make(16, 3), torch.nn.LeakyReLU(0.2)

    def forward(self, x, ei):
        return self.conv2(self.act(self.conv1(x, ei)), ei)


def test_two_layer_net_follows_the_reference_for_five_sgd_steps(dev, graphs):
    """Free-running: both nets start from the same parameters and take their own five SGD steps; the loss and the whole
    parameter vector are compared at every step."""
    from dual_dmp_amd.nn_ops import SAGEConv
    ei, n = graphs["ico"]
    gen = torch.Generator().manual_seed(n)
    x, target = torch.randn(n, 3, generator=gen), torch.randn(n, 3, generator=gen)
    torch.manual_seed(3)
    ref = _Net(lambda i, o: SAGEConvRef(i, o, ["mean", "max"]))
    net = _Net(lambda i, o: SAGEConv(i, o, aggr=["mean", "max"])).to(dev)
    net.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    o_ref, o_net = torch.optim.SGD(ref.parameters(), lr=0.05), torch.optim.SGD(net.parameters(), lr=0.05)
    xd, eid, td = x.to(dev), ei.to(dev), target.to(dev)
    cat = lambda m: torch.cat([p.detach().reshape(-1).double().cpu() for _, p in sorted(m.named_parameters())])
    for step in range(5):
        o_ref.zero_grad()
        l_ref = ((ref(x.double(), ei) - target.double()) ** 2).mean()
        l_ref.backward()
        o_ref.step()
        o_net.zero_grad()
        l_net = ((net(xd, eid) - td) ** 2).mean()
        l_net.backward()
        o_net.step()
        l_net, l_ref = l_net.item(), l_ref.item()
        el, ep = abs(l_net - l_ref) / l_ref, relerr(cat(net), cat(ref))
        print("step %d: loss %.6f rel %.2e, parameters rel-L2 %.2e (tolerance %.0e)" % (step, l_ref, el, ep, OP_TOL))
        assert el <= OP_TOL and ep <= OP_TOL, (step, el, ep)

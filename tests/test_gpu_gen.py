"""GENConv on the GPU: the per-channel softmax gather and its one-launch backward (``ops.gather_softmax`` /
``ops.gather_softmax_bwd``) and the drop-in against the float64 edge-list reference (tests/gen_ref.py) on the graphs of
test_gpu_gat.py: the icosphere (ragged last chunk), the open grid (boundary) and the hub graph (one 1200-entry row), with duplicate
edges and explicit loops on top, and the ``-iso`` variants with one more node without any edge.

Tolerance policy, every comparison against the float64 reference:
* y, dh, dx and the parameter gradients: the project's operator tolerance, rel-L2 <= 1e-5;
* lse, dt_rows (and dh at the offset column) have no project tolerance: the yardstick is the float32 CPU evaluation of the same
  reference against its float64 evaluation on the same inputs, the bound 4x that and not below FLOOR (test_gpu_gat.py's policy).
  Both figures are printed."""
import numpy as np
import pytest
import torch

import edge_weight_route_worker as W
import oracle_jobs as OJ
from gen_ref import GENConvRef, kernel_reference
from test_gpu_gat import FLOOR, OP_TOL, bound, graphs  # noqa: F401  (the graphs fixture)

pytestmark = pytest.mark.gpu
relerr = W.relerr

WIDTHS = [3, 4, 20, 32, 36, 128]        # 3: the scalar kernels; 36: a ragged q loop (9 float4 over 8 lanes); 128: four q steps
SETTINGS = [(1.0, 1e-7), (1.0, None), (-0.7, 1e-7), (-0.7, None)]         # (t, msg_eps)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _inputs(n, C, seed, offset=0.0):
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(n, C, generator=gen) + offset
    return h, torch.randn(n, C, generator=gen), torch.randn(n, C, generator=gen)


def _empty_rows(ei, n):
    return torch.from_numpy(np.bincount(ei[1].numpy(), minlength=n) == 0)


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("name", ["ico", "grid", "hub", "ico-iso", "grid-iso", "hub-iso"])
@pytest.mark.parametrize("C", WIDTHS)
def test_kernels_match_the_reference(dev, graphs, name, C):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    h, root, dout = _inputs(n, C, n + C)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    empty = _empty_rows(ei, n)
    assert bool(empty.any()) == name.endswith("-iso")
    hd, rd, dd = h.to(dev), root.to(dev), dout.to(dev)
    for t, eps in SETTINGS:
        ref = kernel_reference(h, root, dout, ei, n, t, eps, torch.float64)
        r32 = kernel_reference(h, root, dout, ei, n, t, eps, torch.float32)
        assert abs(float(ref["dt"]) - float(ref["dt_rows"].sum())) <= 1e-9 * float(ref["dt_rows"].abs().sum())
        y, lse = ops.gather_softmax(g, hd, t, msg_eps=eps, root=rd)
        dh, dr, dtr = ops.gather_softmax_bwd(g, dd, hd, y - rd, lse, t, msg_eps=eps, root=True, want_dt=True)
        y2, lse2 = ops.gather_softmax(g, hd, t, msg_eps=eps, root=rd)
        dh2, dr2, dtr2 = ops.gather_softmax_bwd(g, dd, hd, y - rd, lse, t, msg_eps=eps, root=True, want_dt=True)
        y0, none = ops.gather_softmax(g, hd, t, msg_eps=eps, want_lse=False)
        torch.cuda.synchronize()
        assert none is None
        for a, b in ((y, y2), (lse, lse2), (dh, dh2), (dr, dr2), (dtr, dtr2)):
            assert torch.equal(a, b)                              # two runs give the same bits
        got = dict(y=y.cpu(), lse=lse.cpu(), dh=dh.cpu(), dt_rows=dtr.cpu())
        for k in ("y", "dh"):
            e = relerr(got[k], ref[k])
            print("%s C=%d t=%g eps=%s %s: rel-L2 %.2e (tolerance %.0e)" % (name, C, t, eps, k, e, OP_TOL))
            assert e <= OP_TOL, (k, t, eps, e)
        e = relerr(y0.cpu(), ref["y"] - root.double())
        assert e <= OP_TOL, ("y without root", e)
        for k in ("lse", "dt_rows"):
            e, yard = relerr(got[k], ref[k]), relerr(r32[k], ref[k])
            print("%s C=%d t=%g eps=%s %s: rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (name, C, t, eps, k, e, yard, bound(yard)))
            assert e <= bound(yard), (k, t, eps, e, yard)
        assert torch.equal(dr.cpu(), dout)                        # droot is dout
        if bool(empty.any()):                                     # an empty row: y IS its root row, lse 0, dh 0
            assert torch.equal(got["y"][empty], root[empty]) and bool((got["lse"][empty] == 0).all())
            assert bool((got["dh"][empty] == 0).all()) and bool((got["dt_rows"][empty] == 0).all()) and bool((y0.cpu()[empty] == 0).all())
        # root="add": dout joins dh after the mask
        dha, none, _ = ops.gather_softmax_bwd(g, dd, hd, y - rd, lse, t, msg_eps=eps, root="add")
        assert none is None and relerr(dha.cpu(), ref["dh"] + dout.double()) <= OP_TOL


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_online_rescale_on_the_hub_row(dev, graphs, sign):
    """h[j] = +j/8, then -j/8, along the source id at t = 4: the 1200-entry row's maximum arrives in its last, then in its first
    batch, and the terms far from it underflow (e^{-4 * 150}).  den >= 1: lse is not below the row's largest t m."""
    from dual_dmp_amd import ops
    ei, n = graphs["hub"]
    C, t = 8, 4.0
    h = (sign * torch.arange(n, dtype=torch.float32) / 8).view(-1, 1).repeat(1, C).contiguous()
    _, root, dout = _inputs(n, C, 5)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    ref = kernel_reference(h, None, dout, ei, n, t, None, torch.float64)
    r32 = kernel_reference(h, None, dout, ei, n, t, None, torch.float32)
    y, lse = ops.gather_softmax(g, h.to(dev), t)
    torch.cuda.synchronize()
    y, lse = y.cpu(), lse.cpu()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(lse).all())
    top = torch.full((n, C), -float("inf"), dtype=torch.float64).scatter_reduce(0, ei[1].view(-1, 1).expand(-1, C), t * h.double()[ei[0]], "amax")
    assert bool(torch.isfinite(top).all())                        # (every row of the hub graph has entries)
    slack = 4 * 2.0 ** -24 * top.abs()                            # lse = t K + (mx + log den): a few float32 roundings at the size of lse
    assert bool((lse.double() >= top - slack).all())
    e = relerr(y, ref["y"])
    el, yl = relerr(lse, ref["lse"]), relerr(r32["lse"], ref["lse"])
    print("hub sign %+d: y rel-L2 %.2e (tolerance %.0e), lse rel-L2 %.2e (yardstick %.2e, bound %.2e)" % (sign, e, OP_TOL, el, yl, bound(yl)))
    assert e <= OP_TOL and el <= bound(yl)
    # t = 0 is the mean
    y0, _ = ops.gather_softmax(g, h.to(dev), 0.0, want_lse=False)
    (mean,), _, _ = ops.gather_stats(g, h.to(dev), want=("mean",))
    e = relerr(y0, mean)
    print("hub sign %+d: t = 0 against gather_stats mean: rel-L2 %.2e" % (sign, e))
    assert e <= OP_TOL


@pytest.mark.parametrize("name", ["ico", "hub"])
def test_offset_column(dev, graphs, name):
    """h = 1000 + N(0, 1), no msg_eps, t = 1.  y: rel-L2 <= OP_TOL, and every element within ONE float32 ulp at 1000 (2^-14) of the
    reference -- the sums run over m - (the row's first message), so only the final addition rounds at the column's offset.  dh by the
    yardstick rule: the backward's m - y at magnitude 1000 is limited by the stored float32 y (and p by the stored float32 lse), both
    half an ulp at 1000 against a spread of 1, which no float32 evaluation of this formula avoids."""
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    C, t = 8, 1.0
    h, _, dout = _inputs(n, C, 11, offset=1000.0)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    ref = kernel_reference(h, None, dout, ei, n, t, None, torch.float64)
    r32 = kernel_reference(h, None, dout, ei, n, t, None, torch.float32)
    y, lse = ops.gather_softmax(g, h.to(dev), t)
    dh, _, _ = ops.gather_softmax_bwd(g, dout.to(dev), h.to(dev), y, lse, t)
    torch.cuda.synchronize()
    e, worst = relerr(y, ref["y"]), float((y.cpu().double() - ref["y"]).abs().max())
    centred = relerr(y.cpu().double() - 1000.0, ref["y"] - 1000.0)
    print("%s offset column: y rel-L2 %.2e (tolerance %.0e), max |error| %.2e (one ulp %.2e), rel-L2 of y - 1000: %.2e"
          % (name, e, OP_TOL, worst, 2.0 ** -14, centred))
    assert e <= OP_TOL and worst <= 2.0 ** -14
    e, yard = relerr(dh, ref["dh"]), relerr(r32["dh"], ref["dh"])
    print("%s offset column: dh rel-L2 %.2e, float32 CPU yardstick %.2e, bound %.2e" % (name, e, yard, bound(yard)))
    assert e <= bound(yard), (e, yard)


def test_column_blocks_and_aliasing(dev, graphs):
    """H and the root as column blocks of one packed buffer, the outputs into column blocks of NaN-filled buffers: the bits of the
    contiguous calls, untouched columns stay NaN; an output that aliases an input is refused."""
    from dual_dmp_amd import ops
    ei, n = graphs["hub-iso"]
    C, t, eps = 20, 0.9, 1e-7
    h, root, dout = (v.to(dev) for v in _inputs(n, C, 3))
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    y, lse = ops.gather_softmax(g, h, t, msg_eps=eps, root=root)
    dh, dr, dtr = ops.gather_softmax_bwd(g, dout, h, y - root, lse, t, msg_eps=eps, root=True, want_dt=True)
    packed = torch.cat([h, root, torch.zeros(n, 4, device=dev)], 1)
    ybuf = torch.full((n, 2 * C + 4), float("nan"), device=dev)
    y2, lse2 = ops.gather_softmax(g, packed[:, :C], t, msg_eps=eps, root=packed[:, C:2 * C], out=ybuf[:, C:2 * C])
    gbuf = torch.full((n, 2 * C + 8), float("nan"), device=dev)
    yp = torch.cat([torch.zeros(n, 4, device=dev), y - root], 1)
    dh2, dr2, dtr2 = ops.gather_softmax_bwd(g, dout, packed[:, :C], yp[:, 4:], lse2, t, msg_eps=eps, root=True, want_dt=True, out=gbuf)
    torch.cuda.synchronize()
    assert y2.data_ptr() == ybuf[:, C:].data_ptr() and dh2.data_ptr() == gbuf.data_ptr() and dr2.data_ptr() == gbuf[:, C:].data_ptr()
    for a, b in ((y, y2), (lse, lse2), (dh, dh2), (dr, dr2), (dtr, dtr2)):
        assert torch.equal(a, b)
    assert bool(torch.isnan(ybuf[:, :C]).all()) and bool(torch.isnan(ybuf[:, 2 * C:]).all()) and bool(torch.isnan(gbuf[:, 2 * C:]).all())
    with pytest.raises(ops.DdmpError):
        ops.gather_softmax(g, h, t, out=h)
    with pytest.raises(ops.DdmpError):
        ops.gather_softmax(g, h, t, root=root, out=root)
    with pytest.raises(ops.DdmpError):
        ops.gather_softmax_bwd(g, dout, h, y, lse, t, out=dout)
    with pytest.raises(ops.DdmpError):
        ops.gather_softmax_bwd(g, dout, h, y, lse, t, out=lse)
    with pytest.raises(ops.DdmpError):
        ops.gather_softmax(g, h, float("nan"))
    with pytest.raises(ops.DdmpError):
        ops.gather_softmax(g, h, 1.0, msg_eps=-1.0)
    with pytest.raises(ops.DdmpError):
        ops.gather_softmax(g, h, 1.0, root=root[:, :C - 1])


# ------------------------------------------------------------------------------------------------ 2. index width
def _rows_forward(rowptr, col, rows, fetch, t, eps):
    """y' and lse of ``rows`` in float64 from the rows of H alone (``fetch``: row ids -> float64 CPU rows of H), on a graph without
    duplicate edges -> (y', lse, the rows' entries as (local row index, source id))."""
    cnt = rowptr[rows + 1] - rowptr[rows]
    ent = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in rows])
    src = col[ent]
    loc = torch.from_numpy(np.repeat(np.arange(len(rows)), cnt))
    uniq = np.unique(src)
    H = fetch(uniq)
    m = H if eps is None else torch.relu(H) + eps
    me = m[torch.from_numpy(np.searchsorted(uniq, src))]
    C = me.shape[1]
    z = t * me
    mx = torch.full((len(rows), C), -float("inf"), dtype=torch.float64).scatter_reduce(0, loc.view(-1, 1).expand(-1, C), z, "amax")
    ex = torch.exp(z - mx[loc])
    den = torch.zeros((len(rows), C), dtype=torch.float64).index_add_(0, loc, ex)
    num = torch.zeros((len(rows), C), dtype=torch.float64).index_add_(0, loc, ex * me)
    return num / den, mx + torch.log(den), loc, src


def test_offsets_beyond_2_31_bytes(dev):
    """1,100,000-node vertex graph of a torus with H and the root as the LAST two 128-column blocks of one [N, 512] float32 buffer
    (2.25e9 bytes > 2^31).  Forward and backward once; y, lse and dh of 600 sampled rows (the last rows among them) are recomputed
    in float64 on the CPU from their two-ring neighbourhoods and compared at the operator tolerance."""
    from dual_dmp_amd import ops, synth
    C, t, eps = 128, 0.8, 1e-7
    v, f = synth.torus(1100, 1000)
    n = len(v)
    assert n == 1100000 and n * 512 * 4 > 2 ** 31
    f = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // n, key % n])).contiguous()
    tab = ops.csr_build_valued_host(ei.numpy(), n, 0)
    rowptr, col = tab["rowptr"].astype(np.int64), tab["col"].astype(np.int64)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(7)
    buf = torch.randn(n, 512, device=dev)
    h, root = buf[:, 256:384], buf[:, 384:]
    dout = torch.randn(n, C, device=dev)
    y, lse = ops.gather_softmax(g, h, t, msg_eps=eps, root=root)
    yp = y - root
    dh, _, _ = ops.gather_softmax_bwd(g, dout, h, yp, lse, t, msg_eps=eps)
    torch.cuda.synchronize()
    rng = np.random.default_rng(0)
    s0 = np.unique(np.concatenate([rng.choice(n - 10, 590, replace=False), np.arange(n - 10, n)]))
    assert len(s0) == 600
    fetch = lambda src: (lambda r: src[torch.from_numpy(r).to(dev)].double().cpu())
    y0, l0, loc, srcs = _rows_forward(rowptr, col, s0, fetch(h), t, eps)
    rows0 = torch.from_numpy(s0).to(dev)
    e_y = relerr(y[rows0], y0 + root[rows0].double().cpu())
    e_l = relerr(lse[rows0], l0)
    # backward of the rows s0: the structure is symmetric and has no duplicates, so row j's entries are the rows i it feeds
    s1 = np.unique(srcs)
    y1, l1, _, _ = _rows_forward(rowptr, col, s1, fetch(h), t, eps)
    at = torch.from_numpy(np.searchsorted(s1, srcs))
    hj = fetch(h)(s0)
    mj = (torch.relu(hj) + eps)[loc]
    gd = torch.exp(t * mj - l1[at]) * fetch(dout)(s1)[at]
    s = torch.zeros((len(s0), C), dtype=torch.float64).index_add_(0, loc, gd)
    r = torch.zeros((len(s0), C), dtype=torch.float64).index_add_(0, loc, gd * (mj - y1[at]))
    dh0 = torch.where(hj > 0, s + t * r, torch.zeros((), dtype=torch.float64))
    e_d = relerr(dh[rows0], dh0)
    print("1.1M nodes, blocks of a [N, 512] buffer: y rel-L2 %.2e, lse %.2e, dh %.2e over %d sampled rows (tolerance %.0e)"
          % (e_y, e_l, e_d, len(s0), OP_TOL))
    assert e_y <= OP_TOL and e_l <= OP_TOL and e_d <= OP_TOL


# ------------------------------------------------------------------------------------------------ 3. the operator
# The ReLUs (the message's and the MLP's) have a step for a gradient: where the float64 reference has a ReLU argument within
# RELU_MARGIN of 0, a float32 evaluation may land on the other side and ONE gradient element then differs by its whole size (about
# 1 / sqrt(elements) = 2e-3 of the norm here), whatever the kernels do.  The arguments are O(1) sums of at most 80 float32 products
# behind a normalisation: their float32 error is a few 1e-7, far below the margin.  The gradient tests therefore draw their
# parameters from the first seed at which the reference's smallest |ReLU argument| clears the margin.
RELU_MARGIN = 1e-5
DIMS = [(16, 16), (12, 32), (40, 8), (3, 6)]
MODES = {"plain": {}, "learn_t": dict(learn_t=True, t=0.7), "msg_norm": dict(msg_norm=True, learn_msg_scale=True),
         "layer": dict(norm="layer"), "nonorm": dict(norm=None), "bias": dict(bias=True)}


def _run(conv, x, ei, t):
    x = x.clone().requires_grad_(True)
    y = conv(x, ei)
    (y * t).sum().backward()
    out = {"y": y.detach(), "dx": x.grad}
    out.update({k: p.grad for k, p in conv.named_parameters() if p.requires_grad})
    return out


@pytest.mark.parametrize("name", ["hub", "ico-iso"])
@pytest.mark.parametrize("cin,cout", DIMS)
@pytest.mark.parametrize("mode", list(MODES))
def test_operator_matches_the_float64_reference(dev, graphs, name, cin, cout, mode):
    """Output, dx and every parameter gradient at OP_TOL.  Two quantities have no relative error of their own:
    ``aggr_module.t.grad`` is a sum over all rows and channels of terms of both signs that may cancel, so its error is held against
    the size of what is summed: |error| <= 1e-5 * sum_j |dt_rows_ref[j]|; ``mlp.0.bias.grad`` with ``bias=True`` and
    ``norm="batch"`` is zero in exact arithmetic (BatchNorm removes a constant), so its error is taken relative to the norm of its
    sibling ``mlp.1.bias.grad`` (as ``lin_key.bias`` in test_gpu_transformer.py).  ``lin_dst.bias.grad`` is a third of the same kind,
    for the same reason and under the same rule: ``lin_dst.bias`` is a constant added to every row of ``out``, ``mlp.0`` turns it into
    a constant per hidden unit, BatchNorm removes it (the reference's own value is 1e-16 of its sibling's).

    ``msg_norm.scale.grad`` is held to OP_TOL like every other gradient although it is one scalar whose N x C terms cancel about a
    thousand to one (ico-iso at (12, 32): sum |terms| / |sum| = 1200): the operator evaluates its BatchNorm in float64 and, where
    the scale is learnt, runs the MLP's GEMMs in the strict mode for it (1.2e-5 before, 1.3e-6 with both)."""
    from dual_dmp_amd.nn_ops import GENConv
    ei, n = graphs[name]
    gen = torch.Generator().manual_seed(n + cin + cout)
    x, t = torch.randn(n, cin, generator=gen), torch.randn(n, cout, generator=gen)
    for attempt in range(200):
        torch.manual_seed(cin * 13 + cout + 1000 * attempt)
        conv = GENConv(cin, cout, **MODES[mode]).to(dev)
        ref = GENConvRef(cin, cout, **MODES[mode]).load_from(conv)
        want = _run(ref, x.double(), ei, t.double())
        if ref.relu_margin() > RELU_MARGIN:
            break
    assert ref.relu_margin() > RELU_MARGIN
    print("%s (%d, %d) %s: parameters from torch.manual_seed(%d) (draw %d), smallest |ReLU argument| %.2e"
          % (name, cin, cout, mode, cin * 13 + cout + 1000 * attempt, attempt, ref.relu_margin()))
    got = _run(conv, x.to(dev), ei.to(dev), t.to(dev))
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want)
    for k in want:
        if k == "aggr_module.t":
            scale = float(ref.dt_rows_of_last_backward(ei).abs().sum())
            e = abs(float(got[k]) - float(want[k])) / scale
            what = "|error| / sum |dt_rows|"
        elif k in ("mlp.0.bias", "lin_dst.bias") and mode == "bias":
            e = float((got[k].double().cpu() - want[k]).norm() / want["mlp.1.bias"].norm())
            what = "error / |mlp.1.bias.grad|"
        else:
            e, what = relerr(got[k], want[k]), "rel-L2"
        print("%s (%d, %d) %s %s: %s %.2e (tolerance %.0e)" % (name, cin, cout, mode, k, what, e, OP_TOL))
        assert e <= OP_TOL, (k, e)


def test_no_grad_forward_and_two_runs_give_the_same_bits(dev, graphs):
    from dual_dmp_amd.nn_ops import GENConv
    ei, n = graphs["hub-iso"]
    torch.manual_seed(2)
    conv = GENConv(12, 32, learn_t=True).to(dev)
    x, eid = torch.randn(n, 12, device=dev), ei.to(dev)
    a, b = _run(conv, x, eid, torch.ones(n, 32, device=dev)), None
    conv.zero_grad()
    b = _run(conv, x, eid, torch.ones(n, 32, device=dev))
    with torch.no_grad():
        y0 = conv(x, eid)
    torch.cuda.synchronize()
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(y0, a["y"]) and not y0.requires_grad


class _TwoLayer(torch.nn.Module):
    def __init__(self, make):
        super().__init__()
        self.c1, self.c2 = make(8, 16), make(16, 16)
        self.out = torch.nn.Linear(16, 3)

    def forward(self, x, ei):
        h = self.c1(x, ei)
        self.pre = h.detach()                                     # (the argument of the ReLU between the layers)
        return self.out(self.c2(torch.relu(h), ei))


def test_three_sgd_steps_follow_the_reference(dev, graphs):
    """Three SGD steps at equal parameters (the float64 reference is loaded from the GPU model before every step): loss and gradient
    within OP_TOL."""
    from dual_dmp_amd.nn_ops import GENConv
    ei, n = graphs["ico"]
    gen = torch.Generator().manual_seed(4)
    x, target = torch.randn(n, 8, generator=gen), torch.randn(n, 3, generator=gen)
    xd, td, eid = x.to(dev), target.to(dev), ei.to(dev)
    for attempt in range(200):
        torch.manual_seed(4 + 1000 * attempt)
        net = _TwoLayer(lambda i, o: GENConv(i, o, learn_t=True)).to(dev)
        opt = torch.optim.SGD(net.parameters(), lr=1e-2)
        steps = []
        for step in range(3):
            r = _TwoLayer(lambda i, o: GENConvRef(i, o, learn_t=True)).double()
            r.c1.load_from(net.c1), r.c2.load_from(net.c2)
            r.out.load_state_dict({k: v.detach().cpu().double() for k, v in net.out.state_dict().items()})
            l64 = ((r(x.double(), ei) - target.double()) ** 2).mean()
            l64.backward()
            g64 = torch.cat([p.grad.reshape(-1) for p in r.parameters()])
            opt.zero_grad()
            loss = ((net(xd, eid) - td) ** 2).mean()
            loss.backward()
            g = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
            steps.append((float(loss.detach()), abs(float(loss.detach()) - float(l64.detach())) / float(l64.detach()), relerr(g, g64),
                          min(r.c1.relu_margin(), r.c2.relu_margin(), float(r.pre.abs().min()))))
            opt.step()
        if min(s[3] for s in steps) > RELU_MARGIN:               # (see RELU_MARGIN: no ReLU of any of the three steps sits on its step)
            break
    assert min(s[3] for s in steps) > RELU_MARGIN
    print("parameters from torch.manual_seed(%d) (draw %d), smallest |ReLU argument| of the three steps %.2e"
          % (4 + 1000 * attempt, attempt, min(s[3] for s in steps)))
    for step, (loss, el, eg, _) in enumerate(steps):
        print("step %d: loss %.6f rel %.2e, gradient rel-L2 %.2e (tolerance %.0e)" % (step, loss, el, eg, OP_TOL))
        assert el <= OP_TOL and eg <= OP_TOL, (step, el, eg)


def test_modular_posnet_runs_with_conv_gen(dev):
    from dual_dmp_amd.networks import PosNet
    from dual_dmp_amd.nn_ops import GENConv
    gt, noisy, smooth, data = OJ.case("ico3")
    torch.manual_seed(6)
    net = PosNet(dev, fused=False, conv="gen")
    assert all(isinstance(getattr(net, "conv%d" % i), GENConv) for i in range(1, 13))
    net.train()
    o = net(data)
    assert o.shape == (len(noisy.vs), 3) and bool(torch.isfinite(o).all())
    o.backward(torch.randn(len(noisy.vs), 3, device=dev))
    for name, p in net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name

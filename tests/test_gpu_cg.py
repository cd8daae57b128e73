"""CGConv on the GPU: the crystal-gate kernels (two per-channel gates with a learned edge term + gather + root, the two backward
launches that recompute the gates, the rows' shares of the edge weights' gradient) and the drop-in against the float64 edge-list
reference (tests/cg_ref.py) on the graphs of test_gpu_gat.py: the icosphere (ragged last chunk), the open grid (boundary) and the hub
graph (one 1200-entry row: many batches), with duplicate edges -- every copy with its own attributes -- and explicit loops on top,
and the "-iso" variants for an empty row.  No self loops are added anywhere.

Tolerance policy (that of test_gpu_gat.py), every comparison against the float64 reference: y, dAf, dAs, dBf, dBs, the column sums
of the partials, dx and the parameter gradients hold the project's operator tolerance, rel-L2 <= 1e-5; the float32 CPU evaluation of
the same reference is printed beside every figure.  The elementwise case has its own bound, derived at the test.  The training
loop's loss has no project tolerance: ``bound(yardstick)`` of test_gpu_gat.py."""
import numpy as np
import pytest
import torch

from cg_ref import CGConvRef, cg_core
from test_gpu_gat import OP_TOL, bound, dev, graphs, relerr  # noqa: F401  (dev, graphs: the fixtures)

pytestmark = pytest.mark.gpu

# scalar kernels | one float4, 7 idle lanes | two | exactly one q step | ragged q loop | two q steps
WIDTHS = [3, 4, 8, 32, 40, 64]
DIMS = [0, 1, 3, 8]
KEYS = ("y", "daf", "das", "dbf", "dbs", "de")


# ------------------------------------------------------------------------------------------------ 1. the kernels
def make_operands(n, C, dim, n_edges, seed):
    """(the four blocks, root, dout), (attr, ef, es) -- None without attributes."""
    gen = torch.Generator().manual_seed(seed)
    mats = tuple(torch.randn(n, C, generator=gen) for _ in range(6))
    if dim == 0:
        return mats, (None, None, None)
    return mats, (torch.randn(n_edges, dim, generator=gen), torch.randn(dim, C, generator=gen) * 0.5,
                  torch.randn(dim, C, generator=gen) * 0.5)


def kernel_reference(mats, edge, ei, mean, dtype):
    """Everything the kernels produce, from the edge-list reference in ``dtype`` with the blocks, the attributes and the transposed
    edge weights as inputs; "de": [dEf^T ; dEs^T], [2 dim, C]."""
    af, as_, bf, bs = (t.to(dtype).requires_grad_(True) for t in mats[:4])
    root, dout = mats[4].to(dtype), mats[5].to(dtype)
    attr, ef, es = (None if t is None else t.to(dtype) for t in edge)
    if attr is not None:
        ef.requires_grad_(True), es.requires_grad_(True)
    y = cg_core(af, as_, bf, bs, ei, attr, ef, es, "mean" if mean else "add") + root
    (y * dout).sum().backward()
    out = dict(y=y.detach(), daf=af.grad, das=as_.grad, dbf=bf.grad, dbs=bs.grad)
    if attr is not None:
        out["de"] = torch.cat([ef.grad, es.grad])
    return out


def kernel_run(ops, g, mats, edge, mean):
    af, as_, bf, bs, root, dout = mats
    attr, ef, es = edge
    kw = dict(attr=attr, ef=ef, es=es, mean=mean)
    got = dict(y=ops.cgate_fwd(g, af, as_, bf, bs, root=root, **kw))
    got["daf"], got["das"], parts = ops.cgate_bwd_row(g, dout, af, as_, bf, bs, **kw)
    got["dbf"], got["dbs"] = ops.cgate_bwd_node(g, dout, af, as_, bf, bs, **kw)
    if attr is not None:
        got["parts"], got["de"] = parts, ops.gatv2_datt(parts, 2 * attr.shape[1])
    else:
        assert parts is None
    torch.cuda.synchronize()
    return got


def check_kernels(tag, got, ref, r32):
    for key in KEYS:
        if key not in ref:
            continue
        e = relerr(got[key], ref[key])
        print("%s %s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)" % (tag, key, e, OP_TOL, relerr(r32[key], ref[key])))
        assert e <= OP_TOL, (key, e)


def run_case(dev, ei, n, C, dim, mean, seed, tag):
    from dual_dmp_amd import ops
    mats, edge = make_operands(n, C, dim, ei.shape[1], seed)
    ref = kernel_reference(mats, edge, ei, mean, torch.float64)
    r32 = kernel_reference(mats, edge, ei, mean, torch.float32)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    got = kernel_run(ops, g, tuple(t.to(dev) for t in mats), tuple(None if t is None else t.to(dev) for t in edge), mean)
    check_kernels(tag, got, ref, r32)
    return mats, got


@pytest.mark.parametrize("name", ["ico", "grid", "hub", "grid-iso", "hub-iso"])
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("dim", DIMS)
def test_kernels_match_the_reference(dev, graphs, name, C, dim):
    ei, n = graphs[name]
    mats, got = run_case(dev, ei, n, C, dim, False, n + C + dim, "%s C=%d dim=%d" % (name, C, dim))
    empty = torch.from_numpy(np.bincount(ei[1].numpy(), minlength=n) == 0)
    assert bool(empty.any()) == name.endswith("-iso")
    if empty.any():
        assert torch.equal(got["y"].cpu()[empty], mats[4][empty])                       # the init exactly, bit for bit
        for key in ("daf", "das", "dbf", "dbs") + (("parts",) if dim else ()):
            assert not got[key].cpu()[empty].any(), key


# ------------------------------------------------------------------------------------------------ 2. duplicates
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("dim", [0, 3])
@pytest.mark.parametrize("mean", [False, True])
def test_duplicate_edges_with_their_own_attributes_and_one_directional_duplicates(dev, graphs, C, dim, mean):
    """"grid" (which has two-directional duplicates already) plus one-directional duplicates of existing edges: the structure stays
    symmetric, the multiplicities do not.  The node side has to read the MIRRORED entry -- its multiplicity (dim = 0) or its span
    of input edges (dim = 3); every copy of an edge carries attributes of its own; the mean divides by the input edges."""
    from dual_dmp_amd import ops
    ei, n = graphs["grid"]
    ei = torch.cat([ei, ei[:, 100:107], ei[:, 100:103], ei[:, 300:304]], 1).contiguous()
    t = ops.csr_build_valued_host(ei.numpy(), n, 0)
    a = ops.valued_values_host(t, None, 0)[0]
    assert int((a != a[t["mirror"]]).sum()) >= 10 and int(a.max()) >= 3                 # asymmetric indeed
    run_case(dev, ei, n, C, dim, mean, C + dim, "grid+asym C=%d dim=%d mean=%d" % (C, dim, mean))


@pytest.mark.parametrize("dim", [0, 3])
def test_mean_is_add_over_the_number_of_input_edges(dev, graphs, dim):
    from dual_dmp_amd import ops
    ei, n = graphs["hub-iso"]
    mats, edge = make_operands(n, 8, dim, ei.shape[1], 5)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    md, ed = tuple(t.to(dev) for t in mats), tuple(None if t is None else t.to(dev) for t in edge)
    add, mean = kernel_run(ops, g, md, ed, False), kernel_run(ops, g, md, ed, True)
    cnt = torch.from_numpy(np.bincount(ei[1].numpy(), minlength=n)).double().clamp(min=1).unsqueeze(1)
    root = mats[4].double()
    assert int(cnt.max()) >= 1200
    assert relerr(mean["y"].double().cpu() - root, (add["y"].double().cpu() - root) / cnt) <= OP_TOL
    for key in ("daf", "das") + (("parts",) if dim else ()):
        assert relerr(mean[key], add[key].double().cpu() / cnt) <= OP_TOL, key


# ------------------------------------------------------------------------------------------------ 3. elementwise accuracy
@pytest.mark.parametrize("C,dim", [(64, 0), (64, 1), (3, 1)])
def test_every_element_is_accurate_over_the_whole_range_of_both_gates(dev, C, dim):
    """512 disjoint pairs 2k <-> 2k+1: every node has exactly one incoming edge, so y is ONE product sigmoid(F) softplus(S) per
    element.  F and S sit on a grid over [-30, 30] and are formed EXACTLY in float32 -- block values that are multiples of 1/8 up
    to 15 (dim = 0) or 13 (dim = 1: attributes that are multiples of 1/4 up to 1 times edge weights that are multiples of 1/4 up to
    4 add a multiple of 1/16 up to 4) -- so the float64 reference sees the same arguments; the four corners (+-30, +-30) are put
    there by hand.  Bound, per element, relative to the float64 value: 1e-5 -- the hardware exponent's rounding leaves
    |x| 2^-24 <= 1.8e-6 in each gate at |x| = 30, plus a few ulps of the reciprocals, the series and the product.  softplus(S) ~
    exp(S) for S -> -30: a ``log(1 + exp(S))`` returns 0 there (exp(S) < 2^-24) and misses the bound by 100 % of the element."""
    from dual_dmp_amd import ops
    n = 1024
    k = torch.arange(0, n, 2)
    ei = torch.stack([torch.cat([k, k + 1]), torch.cat([k + 1, k])]).contiguous()    # edge t < 512: 2t -> 2t+1; 512 + t: 2t+1 -> 2t
    gen = torch.Generator().manual_seed(C + dim)
    grid = lambda lo, hi, step, *s: torch.randint(lo, hi + 1, s, generator=gen).float() * step
    lim = 13.0 if dim else 15.0
    af, as_, bf, bs = (grid(-int(lim * 8), int(lim * 8), 0.125, n, C) for _ in range(4))
    attr = ef = es = None
    if dim:
        attr, ef, es = grid(-4, 4, 0.25, n, dim), grid(-16, 16, 0.25, dim, C), grid(-16, 16, 0.25, dim, C)
        ef[0, 0], es[0, 0], ef[0, 1], es[0, 1] = 4.0, 4.0, 4.0, -4.0
    # the corners: node 0 (fed by node 1 through edge 512) takes (+30, +30) in channel 0 and (+30, -30) in channel 1, node 2 (fed
    # by node 3 through edge 513) the opposite signs
    for r, sgn in ((0, 1.0), (1, -1.0)):
        i, j = 2 * r, 2 * r + 1
        af[i, :2], bf[j, :2] = sgn * lim, sgn * lim
        as_[i, 0], bs[j, 0], as_[i, 1], bs[j, 1] = sgn * lim, sgn * lim, -sgn * lim, -sgn * lim
        if dim:
            attr[512 + r] = sgn
    dd = lambda t: None if t is None else t.double()
    ref = cg_core(dd(af), dd(as_), dd(bf), dd(bs), ei, dd(attr), dd(ef), dd(es))
    r32 = cg_core(af, as_, bf, bs, ei, attr, ef, es)
    pf = af[ei[1]] + bf[ei[0]] + (attr @ ef if dim else 0.0)
    ps = as_[ei[1]] + bs[ei[0]] + (attr @ es if dim else 0.0)
    assert float(pf.max()) == 30 and float(pf.min()) == -30 and float(ps.max()) == 30 and float(ps.min()) == -30
    assert float(ref.min()) > 1e-30 and float(ref[0, 1]) < 1e-12 and float(ref[2, 0]) < 1e-25    # no underflow; the (F, -30) corners
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    mv = lambda t: None if t is None else t.to(dev)
    y = ops.cgate_fwd(g, mv(af), mv(as_), mv(bf), mv(bs), attr=mv(attr), ef=mv(ef), es=mv(es)).double().cpu()
    err = ((y - ref).abs() / ref).max()
    e32 = ((r32.double() - ref).abs() / ref).max()
    print("C=%d dim=%d: max relative error per element %.2e (bound 1e-5; float32 CPU %.2e), F in [%g, %g], S in [%g, %g]"
          % (C, dim, err, e32, pf.min(), pf.max(), ps.min(), ps.max()))
    assert bool(torch.isfinite(y).all()) and float(err) <= 1e-5


# ------------------------------------------------------------------------------------------------ 4. saturation
@pytest.mark.parametrize("C,dim", [(3, 0), (40, 3)])
def test_saturated_gates_stay_finite(dev, graphs, C, dim):
    """One row in eight of the A blocks and of the B blocks times 60: gate arguments of a few hundred either way, where exp
    overflows.  Every output is finite and the operator tolerance holds (the error norms are carried by the unsaturated rows)."""
    from dual_dmp_amd import ops
    ei, n = graphs["hub"]
    mats, edge = make_operands(n, C, dim, ei.shape[1], C + 1)
    mats[0][::8] *= 60
    mats[1][::8] *= 60
    mats[2][3::8] *= 60
    mats[3][3::8] *= 60
    assert float((mats[0][ei[1]] + mats[2][ei[0]]).abs().max()) > 100 and float((mats[1][ei[1]] + mats[3][ei[0]]).abs().max()) > 100
    ref = kernel_reference(mats, edge, ei, False, torch.float64)
    r32 = kernel_reference(mats, edge, ei, False, torch.float32)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    got = kernel_run(ops, g, tuple(t.to(dev) for t in mats), tuple(None if t is None else t.to(dev) for t in edge), False)
    for key, val in got.items():
        assert bool(torch.isfinite(val).all()), key
    check_kernels("hub saturated C=%d dim=%d" % (C, dim), got, ref, r32)


# ------------------------------------------------------------------------------------------------ 5. layouts
@pytest.mark.parametrize("C,dim", [(8, 3), (8, 0), (3, 3)])
def test_column_blocks_misaligned_views_and_aliasing(dev, graphs, C, dim):
    """The four blocks as column blocks of a packed [Af | As | Bf | Bs] buffer, outputs into column blocks of one NaN-prefilled
    gradient buffer, give the bits of the contiguous calls; the same operands as views that start 4 bytes off a 16-byte boundary
    take the scalar kernels and agree to tolerance; an output that is one of the inputs (or another output) raises."""
    from dual_dmp_amd import ops
    ei, n = graphs["ico-iso"]
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    mats, edge = make_operands(n, C, dim, ei.shape[1], 3)
    root, dout = mats[4].to(dev), mats[5].to(dev)
    attr, ef, es = (None if t is None else t.to(dev) for t in edge)
    kw = dict(attr=attr, ef=ef, es=es)
    buf = torch.cat(mats[:4], 1).to(dev)
    blk = tuple(buf[:, i * C:(i + 1) * C] for i in range(4))
    con = tuple(t.contiguous() for t in blk)
    y = ops.cgate_fwd(g, *blk, root=root, **kw)
    assert torch.equal(y, ops.cgate_fwd(g, *con, root=root, **kw))
    assert torch.equal(ops.cgate_fwd(g, *con, **kw), ops.cgate_fwd(g, *con, root=torch.zeros_like(root), **kw))
    gbuf = torch.full((n, 5 * C), float("nan"), device=dev)
    gb = tuple(gbuf[:, i * C:(i + 1) * C] for i in range(5))
    daf, das, parts = ops.cgate_bwd_row(g, dout, *blk, out_f=gb[0], out_s=gb[1], **kw)
    dbf, dbs = ops.cgate_bwd_node(g, dout, *blk, out_f=gb[2], out_s=gb[3], out_r=gb[4], **kw)
    daf2, das2, parts2 = ops.cgate_bwd_row(g, dout, *con, **kw)
    dbf2, dbs2 = ops.cgate_bwd_node(g, dout, *con, **kw)
    for i, want in enumerate((daf2, das2, dbf2, dbs2, dout)):                            # the root block's gradient is dOut
        assert torch.equal(gb[i], want), i
    assert daf.data_ptr() == gbuf.data_ptr() and dbs.data_ptr() == gb[3].data_ptr()
    assert (parts is None) == (dim == 0) and (dim == 0 or torch.equal(parts, parts2))
    assert ops.cgate_bwd_row(g, dout, *con, want_parts=False, **kw)[2] is None
    # 4 bytes off: the scalar route
    off = torch.empty((n, 4 * C + 1), device=dev)
    off[:, 1:] = buf
    mis = tuple(off[:, 1 + i * C:1 + (i + 1) * C] for i in range(4))
    assert mis[0].data_ptr() % 16 == 4 and torch.equal(mis[2], blk[2])
    tol = 1e-6                                                   # two float32 evaluations of the same sums in the same order
    assert relerr(ops.cgate_fwd(g, *mis, root=root, **kw), y) <= tol
    daf3, das3, parts3 = ops.cgate_bwd_row(g, dout, *mis, **kw)
    dbf3, dbs3 = ops.cgate_bwd_node(g, dout, *mis, **kw)
    for u, v in ((daf3, daf2), (das3, das2), (dbf3, dbf2), (dbs3, dbs2)) + (((parts3, parts2),) if dim else ()):
        assert relerr(u, v) <= tol
    # aliasing
    for t in con + (root,):
        with pytest.raises(ops.DdmpError):
            ops.cgate_fwd(g, *con, root=root, out=t, **kw)
    for t in con + (dout,):
        for name in ("out_f", "out_s"):
            with pytest.raises(ops.DdmpError):
                ops.cgate_bwd_row(g, dout, *con, **{name: t}, **kw)
            with pytest.raises(ops.DdmpError):
                ops.cgate_bwd_node(g, dout, *con, **{name: t}, **kw)
        with pytest.raises(ops.DdmpError):
            ops.cgate_bwd_node(g, dout, *con, out_r=t, **kw)
    o = torch.empty_like(root)
    with pytest.raises(ops.DdmpError):
        ops.cgate_bwd_row(g, dout, *con, out_f=o, out_s=o, **kw)
    for pair in (dict(out_f=o, out_s=o), dict(out_f=o, out_r=o), dict(out_s=o, out_r=o)):
        with pytest.raises(ops.DdmpError):
            ops.cgate_bwd_node(g, dout, *con, **pair, **kw)
    with pytest.raises(ops.DdmpError):
        ops.cgate_fwd(g, con[0], con[1], con[2], con[3][:, :C - 1], **kw)               # widths differ
    if dim:
        with pytest.raises(ops.DdmpError):
            ops.cgate_fwd(g, *con, attr=attr[:-1].contiguous(), ef=ef, es=es)           # one row per input edge
    if dim and dim != C:
        with pytest.raises(ops.DdmpError):
            ops.cgate_fwd(g, *con, attr=attr, ef=ef.t().contiguous(), es=es)            # [dim, C], transposed
        with pytest.raises(ops.DdmpError):
            ops.cgate_fwd(g, *con, attr=torch.zeros(ei.shape[1], 9, device=dev), ef=torch.zeros(9, C, device=dev),
                          es=torch.zeros(9, C, device=dev))                              # dim > CG_MAX_DIM


# ------------------------------------------------------------------------------------------------ 6. reproducibility
@pytest.mark.parametrize("C,dim", [(40, 3), (64, 0), (3, 8)])
def test_two_runs_give_the_same_bits(dev, graphs, C, dim):
    from dual_dmp_amd import ops
    ei, n = graphs["hub"]
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    mats, edge = make_operands(n, C, dim, ei.shape[1], 1)
    md, ed = tuple(t.to(dev) for t in mats), tuple(None if t is None else t.to(dev) for t in edge)
    a = {k: v.clone() for k, v in kernel_run(ops, g, md, ed, True).items()}
    b = kernel_run(ops, g, md, ed, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 7. the operator
PNAMES = ("lin_f.weight", "lin_f.bias", "lin_s.weight", "lin_s.bias", "bn.weight", "bn.bias")


def _operator_run(conv, x, ei, attr, t):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, ei) if attr is None else conv(x, ei, attr)
    (y * t).sum().backward()
    have = dict(conv.named_parameters())
    return dict([("y", y.detach()), ("dx", x.grad)] + [("d " + k, have[k].grad) for k in PNAMES if k in have])


@pytest.mark.parametrize("C", [8, 40])
@pytest.mark.parametrize("dim,aggr,batch_norm", [(0, "add", False), (3, "add", False), (0, "mean", True), (3, "mean", True)])
@pytest.mark.parametrize("name", ["ico", "hub-iso"])
def test_operator_matches_the_float64_reference(dev, graphs, C, dim, aggr, batch_norm, name):
    from dual_dmp_amd.nn_ops import CGConv
    ei, n = graphs[name]
    torch.manual_seed(C + dim)
    conv = CGConv(C, dim=dim, aggr=aggr, batch_norm=batch_norm)
    if batch_norm:
        with torch.no_grad():
            conv.bn.weight.uniform_(0.5, 1.5)                    # (ones and zeros at initialisation)
            conv.bn.bias.uniform_(-0.5, 0.5)
    gen = torch.Generator().manual_seed(n)
    x, t = torch.randn(n, C, generator=gen), torch.randn(n, C, generator=gen)
    attr = torch.randn(ei.shape[1], dim, generator=gen) if dim else None
    refs = {dtype: CGConvRef(C, dim=dim, aggr=aggr, batch_norm=batch_norm, dtype=dtype).load_from(conv)
            for dtype in (torch.float64, torch.float32)}
    conv.to(dev)
    got = _operator_run(conv, x.to(dev), ei.to(dev), None if attr is None else attr.to(dev), t.to(dev))
    r64, r32 = (_operator_run(refs[dtype], x.to(dtype), ei, None if attr is None else attr.to(dtype), t.to(dtype))
                for dtype in (torch.float64, torch.float32))
    assert list(got) == list(r64) and len(got) == 6 + 2 * batch_norm and all(v is not None for v in got.values())
    for key in got:
        assert got[key].shape == r64[key].shape, key
        e = relerr(got[key], r64[key])
        print("%s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)" % (key, e, OP_TOL, relerr(r32[key], r64[key])))
        assert e <= OP_TOL, (key, e)
    if batch_norm:                                               # the running statistics after one training-mode call
        for key in ("running_mean", "running_var"):
            e = relerr(getattr(conv.bn, key), getattr(refs[torch.float64].bn, key))
            print("bn.%s: rel-L2 %.2e (tolerance %.0e; float32 CPU %.2e)"
                  % (key, e, OP_TOL, relerr(getattr(refs[torch.float32].bn, key), getattr(refs[torch.float64].bn, key))))
            assert e <= OP_TOL, (key, e)
        assert int(conv.bn.num_batches_tracked) == 1
    elif name == "hub-iso":
        assert torch.equal(got["y"][-1].cpu(), x[-1])            # the node without incoming edges: x_i, bit for bit


def test_unused_parameters_keep_no_gradient(dev, graphs):
    from dual_dmp_amd.nn_ops import CGConv
    ei, n = graphs["grid"]
    torch.manual_seed(2)
    conv = CGConv(8, dim=2).to(dev)
    conv.lin_s.weight.requires_grad_(False)
    conv.lin_f.bias.requires_grad_(False)
    x = torch.randn(n, 8, device=dev)
    conv(x, ei.to(dev), torch.randn(ei.shape[1], 2, device=dev)).sum().backward()
    assert x.grad is None and conv.lin_s.weight.grad is None and conv.lin_f.bias.grad is None
    assert conv.lin_f.weight.grad is not None and conv.lin_s.bias.grad is not None


# ------------------------------------------------------------------------------------------------ 8. training
class _TwoLayer(torch.nn.Module):
    def __init__(self, mk):
        super().__init__()
        self.c1, self.c2 = mk(), mk()

    def forward(self, x, ei, attr):
        return self.c2(torch.tanh(self.c1(x, ei, attr)), ei, attr)


def test_twenty_sgd_steps_follow_the_float64_reference(dev, graphs):
    """Free-running: the GPU net, the float64 reference and the float32 CPU reference start from the same parameters and take their
    own 20 SGD steps of a two-layer net (C = 8, dim = 3, mean) regressing a fixed target on "grid".  The yardstick is the float32
    CPU reference's relative loss deviation from the float64 one; a single step's deviation is one draw of a quantity that changes
    sign along the run, so the yardstick is its maximum over the 20 steps, and every step's GPU deviation has to stay within
    ``bound(yardstick)``."""
    from dual_dmp_amd.nn_ops import CGConv
    ei, n = graphs["grid"]
    gen = torch.Generator().manual_seed(4)
    x, target = torch.randn(n, 8, generator=gen), torch.randn(n, 8, generator=gen)
    attr = torch.randn(ei.shape[1], 3, generator=gen)
    torch.manual_seed(4)
    net = _TwoLayer(lambda: CGConv(8, dim=3, aggr="mean"))
    nets = {"gpu": net, "f64": _TwoLayer(lambda: CGConvRef(8, dim=3, aggr="mean")),
            "f32": _TwoLayer(lambda: CGConvRef(8, dim=3, aggr="mean", dtype=torch.float32))}
    for k in ("f64", "f32"):
        nets[k].c1.load_from(net.c1), nets[k].c2.load_from(net.c2)
    net.to(dev)
    data = {"gpu": (x.to(dev), ei.to(dev), attr.to(dev), target.to(dev)), "f64": (x.double(), ei, attr.double(), target.double()),
            "f32": (x, ei, attr, target)}
    losses = {k: [] for k in nets}
    for k, m in nets.items():
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        xx, ee, aa, tt = data[k]
        for step in range(20):
            opt.zero_grad()
            loss = ((m(xx, ee, aa) - tt) ** 2).mean()
            loss.backward()
            opt.step()
            losses[k].append(float(loss.detach()))
    l64 = np.array(losses["f64"])
    eg, e32 = np.abs(np.array(losses["gpu"]) - l64) / l64, np.abs(np.array(losses["f32"]) - l64) / l64
    yard = float(e32.max())
    for step in range(20):
        print("step %d: loss %.6f, rel %.2e (float32 CPU %.2e; yardstick %.2e, bound %.2e)"
              % (step, l64[step], eg[step], e32[step], yard, bound(yard)))
    assert l64[-1] < l64[0] and losses["gpu"][-1] < losses["gpu"][0]
    assert float(eg.max()) <= bound(yard), (float(eg.max()), yard)

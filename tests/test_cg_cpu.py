"""CGConv: everything that can be checked without a GPU -- the two float64 references (tests/cg_ref.py) against each other, the host
side of ``nn_ops._CGConvFn`` / ``CGConv`` over torch restatements of the kernels (tests/cg_ops_stub.py), the ``mult[mirror]`` use of
the node side, parameter names / shapes / initialisation, the refusals, the call sequence and the declarations of the three entry
points."""
import math

import pytest
import torch

import cg_ops_stub
from cg_ref import CGConvRef, cg_core, cg_messages_dense, cg_messages_edge_list


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def small_graph():
    """12 nodes: a ring 0 .. 10 (both directions), chords, duplicate edges (3 -> 4 three times and 4 -> 3 once, 7 <-> 8 twice
    each -- every copy carries its own attributes), an explicit loop on node 5, and node 11 without any edge."""
    ring = [(k, (k + 1) % 11) for k in range(11)]
    und = ring + [(0, 5), (2, 9)]
    e = und + [(b, a) for a, b in und] + [(3, 4), (3, 4), (7, 8), (8, 7), (5, 5)]
    return torch.tensor(e, dtype=torch.long).t().contiguous(), 12


@pytest.fixture(scope="module")
def mesh():
    """An open grid, both directions of every edge, no duplicates."""
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    v, f = synth.open_grid(6, 5)
    e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
    return torch.cat([e, e[[1, 0]]], 1).contiguous(), len(v)


def _lin(C, dim, bias, seed):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=gen, dtype=torch.float64) * 0.5).requires_grad_(True)
    return mk(C, 2 * C + dim), mk(C) if bias else None, mk(C, 2 * C + dim), mk(C) if bias else None


@pytest.mark.parametrize("dim", [0, 3])
@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("bias", [True, False])
def test_the_two_references_agree_in_float64(mesh, dim, aggr, bias):
    ei, n = mesh
    gen = torch.Generator().manual_seed(dim + 5)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    a = torch.randn(ei.shape[1], dim, generator=gen, dtype=torch.float64) if dim else None
    p = _lin(5, dim, bias, 3)
    t = torch.randn(n, 5, generator=gen, dtype=torch.float64)
    leaves = [x] + [q for q in p if q is not None]
    outs, grads = [], []
    for fn in (cg_messages_edge_list, cg_messages_dense):
        y = fn(x, ei, a, *p, aggr)
        outs.append(y)
        grads.append(torch.autograd.grad((y * t).sum(), leaves))
    assert relerr(outs[0], outs[1]) < 1e-12
    for u, v in zip(*grads):
        assert relerr(u, v) < 1e-12
    # the block form the kernels take is the same function
    C = 5
    wf, bf, ws, bs = (None if q is None else q.detach() for q in p)
    xd = x.detach()
    af, as_ = xd @ wf[:, :C].t() + (0 if bf is None else bf), xd @ ws[:, :C].t() + (0 if bs is None else bs)
    y = cg_core(af, as_, xd @ wf[:, C:2 * C].t(), xd @ ws[:, C:2 * C].t(), ei, a, wf[:, 2 * C:].t() if dim else None,
                ws[:, 2 * C:].t() if dim else None, aggr)
    assert relerr(y, outs[0]) < 1e-12


def test_the_reference_on_a_graph_done_by_hand():
    """Node 1 feeds node 0 twice with different attributes, node 2 has no incoming edge: the two gates, the learned edge term and
    the residual, written out."""
    x = torch.tensor([[1.0], [2.0], [-1.0]], dtype=torch.float64)
    ei = torch.tensor([[1, 1, 0], [0, 0, 1]])
    attr = torch.tensor([[0.5], [-1.0], [2.0]], dtype=torch.float64)
    conv = CGConvRef(1, dim=1)
    with torch.no_grad():
        conv.lin_f.weight.copy_(torch.tensor([[1.0, -1.0, 2.0]]))
        conv.lin_f.bias.fill_(0.25)
        conv.lin_s.weight.copy_(torch.tensor([[0.5, 1.0, -1.0]]))
        conv.lin_s.bias.fill_(-0.5)
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))
    sp = lambda v: math.log1p(math.exp(v))
    m = lambda xi, xj, a: sig(xi - xj + 2 * a + 0.25) * sp(0.5 * xi + xj - a - 0.5)
    y = conv(x, ei, attr)
    want = torch.tensor([[1.0 + m(1, 2, 0.5) + m(1, 2, -1.0)], [2.0 + m(2, 1, 2.0)], [-1.0]], dtype=torch.float64)
    assert torch.allclose(y, want, atol=1e-14)
    mean = CGConvRef(1, dim=1, aggr="mean").load_from(conv)(x, ei, attr)
    assert torch.allclose(mean[0], (want[0] - 1.0) / 2 + 1.0, atol=1e-14) and torch.equal(mean[2], x[2])


PNAMES = ("lin_f.weight", "lin_f.bias", "lin_s.weight", "lin_s.bias", "bn.weight", "bn.bias")


def _operator_run(conv, x, ei, attr, t):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, ei) if attr is None else conv(x, ei, attr)
    (y * t).sum().backward()
    have = dict(conv.named_parameters())
    return dict([("y", y.detach()), ("dx", x.grad)] + [("d " + k, have[k].grad) for k in PNAMES if k in have])


@pytest.mark.parametrize("dim", [0, 3])
@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("batch_norm", [False, True])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("C", [5, 8])
def test_the_drop_in_over_the_stub_equals_the_reference(monkeypatch, dim, aggr, batch_norm, bias, C):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", cg_ops_stub)
    monkeypatch.setattr(nn_ops, "_need_gpu", lambda *a, **k: None)       # (the stub runs on CPU tensors)
    ei, n = small_graph()
    torch.manual_seed(C + dim)
    conv = nn_ops.CGConv(C, dim=dim, aggr=aggr, batch_norm=batch_norm, bias=bias)
    if batch_norm:
        with torch.no_grad():
            conv.bn.weight.uniform_(0.5, 1.5)
            conv.bn.bias.uniform_(-0.5, 0.5)
    ref = CGConvRef(C, dim=dim, aggr=aggr, batch_norm=batch_norm, bias=bias).load_from(conv)
    gen = torch.Generator().manual_seed(7)
    x, t = torch.randn(n, C, generator=gen), torch.randn(n, C, generator=gen)
    attr = torch.randn(ei.shape[1], dim, generator=gen) if dim else None
    if dim:
        assert not torch.equal(attr[-5], attr[-4])                       # the duplicates 3 -> 4 carry different attributes
    del cg_ops_stub.calls[:]
    got = _operator_run(conv, x, ei, attr, t)
    assert cg_ops_stub.calls == ["graph_for", "cgate_fwd" + ("" if batch_norm else "+root"),
                                 "cgate_bwd_row" + ("+parts" if dim else ""), "cgate_bwd_node"] + (["gatv2_datt"] if dim else [])
    want = _operator_run(ref, x.double(), ei, None if attr is None else attr.double(), t.double())
    assert list(got) == list(want) and len(got) == 4 + 2 * bias + 2 * batch_norm
    for k in got:
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float32, k
        assert relerr(got[k], want[k]) <= 1e-5, (k, relerr(got[k], want[k]))
    if not batch_norm:
        assert torch.equal(got["y"][11], x[11])                          # the node without edges: x_i, bit for bit
    else:
        assert relerr(conv.bn.running_mean, ref.bn.running_mean) <= 1e-5 and relerr(conv.bn.running_var, ref.bn.running_var) <= 1e-5
    if dim:                                                              # float64 attributes are rounded once
        assert torch.equal(_operator_run(conv, x, ei, attr.double(), t)["d lin_f.weight"], got["d lin_f.weight"])


@pytest.mark.parametrize("dim", [0, 2])
def test_the_node_side_reads_the_mirrored_entry(dim):
    """3 -> 4 three times against 4 -> 3 once: the node side with ``mult[e]`` in place of ``mult[mirror[e]]`` is a different number
    (dim == 0); with attributes the stub's node side must agree with the autograd gradient of the reference."""
    ei, n = small_graph()
    g = cg_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    assert bool((g.a != g.a[g.mirror]).any())
    gen = torch.Generator().manual_seed(2)
    af, as_, bf, bs, dout = (torch.randn(n, 4, generator=gen) for _ in range(5))
    attr = torch.randn(ei.shape[1], dim, generator=gen) if dim else None
    ef, es = (torch.randn(dim, 4, generator=gen) for _ in range(2)) if dim else (None, None)
    for mean in (False, True):
        leaves = [t.double().requires_grad_(True) for t in (af, as_, bf, bs)]
        dd = lambda t: None if t is None else t.double()
        y = cg_core(*leaves, ei, dd(attr), dd(ef), dd(es), "mean" if mean else "add")
        _, _, gbf, gbs = torch.autograd.grad((y * dout.double()).sum(), leaves)
        dbf, dbs = cg_ops_stub.cgate_bwd_node(g, dout, af, as_, bf, bs, attr, ef, es, mean=mean)
        assert relerr(dbf, gbf) < 1e-6 and relerr(dbs, gbs) < 1e-6
        if dim == 0:
            a = g.a
            g.a = a[g.mirror]                                            # mirror is an involution: the stub now reads mult[e]
            bad_f, bad_s = cg_ops_stub.cgate_bwd_node(g, dout, af, as_, bf, bs, mean=mean)
            g.a = a
            assert relerr(bad_f, gbf) > 1e-3 and relerr(bad_s, gbs) > 1e-3


def test_state_dict_keys_shapes_and_init():
    from dual_dmp_amd.nn_ops import CGConv
    torch.manual_seed(0)
    conv = CGConv(40, dim=3)
    sd = conv.state_dict()
    assert sorted(sd) == ["lin_f.bias", "lin_f.weight", "lin_s.bias", "lin_s.weight"]
    assert sorted(n for n, _ in conv.named_parameters()) == sorted(sd) and conv.bn is None
    a = 1.0 / math.sqrt(83)
    for k in ("lin_f", "lin_s"):
        assert sd[k + ".weight"].shape == (40, 83) and sd[k + ".bias"].shape == (40,)
        for leaf in (".weight", ".bias"):
            v = sd[k + leaf]
            assert v.abs().max() <= a and v.abs().max() > 0.9 * a, k + leaf
        assert abs(float(sd[k + ".weight"].mean())) < 0.1 * a
    assert not torch.equal(sd["lin_f.weight"], sd["lin_s.weight"])
    assert (conv.channels, conv.dim, conv.aggr, conv.batch_norm) == (40, 3, "add", False)
    nob = CGConv(8, bias=False)
    assert nob.lin_f.bias is None and nob.lin_s.bias is None and sorted(nob.state_dict()) == ["lin_f.weight", "lin_s.weight"]
    assert nob.lin_f.weight.shape == (8, 16)
    bn = CGConv(8, dim=2, aggr="mean", batch_norm=True)
    assert isinstance(bn.bn, torch.nn.BatchNorm1d) and bn.bn.num_features == 8
    assert sorted(bn.state_dict()) == sorted(["lin_f.weight", "lin_f.bias", "lin_s.weight", "lin_s.bias", "bn.weight", "bn.bias",
                                              "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"])
    for aggr in ("add", "sum", "mean"):
        assert CGConv(4, aggr=aggr).aggr == aggr
    conv2 = CGConv(40, dim=3)
    conv2.load_state_dict(sd)
    assert torch.equal(conv2.lin_s.weight, sd["lin_s.weight"])
    ref = CGConvRef(8, dim=2, aggr="mean", batch_norm=True, dtype=torch.float32).load_from(bn)
    assert sorted(ref.state_dict()) == sorted(bn.state_dict()) and torch.equal(ref.lin_f.bias, bn.lin_f.bias)
    assert [tuple(v.shape) for _, v in sorted(ref.state_dict().items())] == [tuple(v.shape) for _, v in sorted(bn.state_dict().items())]
    assert "40, dim=3" in repr(conv)
    before = conv.lin_f.weight.detach().clone()
    conv.reset_parameters()
    assert not torch.equal(conv.lin_f.weight, before) and conv.lin_f.weight.abs().max() <= a


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import CGConv

    class Trap:
        DdmpError = ops.DdmpError
        CG_MAX_DIM = ops.CG_MAX_DIM

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    assert ops.CG_MAX_DIM == 8
    for bad in ((4, 4), [4, 4]):
        with pytest.raises(ValueError):
            CGConv(bad)
    for bad in (-1, 9, 2.0, None, True):
        with pytest.raises(ValueError, match="dim"):
            CGConv(4, dim=bad)
    for aggr in ("max", "min", "mul", None):
        with pytest.raises(ValueError, match="aggr"):
            CGConv(4, aggr=aggr)
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    attr = torch.rand(2, 3)
    conv, plain = CGConv(4, dim=3), CGConv(4)
    with pytest.raises(ValueError):
        conv((x, x), ei, attr)
    with pytest.raises(ValueError):
        conv(x, ei)                                              # edge_attr missing with dim > 0
    with pytest.raises(ValueError):
        conv(x, ei, None)
    with pytest.raises(ValueError):
        plain(x, ei, attr)                                       # edge_attr given with dim == 0
    for bad in (torch.rand(2, 2), torch.rand(3, 3), torch.rand(2), torch.rand(2, 3, 1)):
        with pytest.raises(ValueError):
            conv(x, ei, bad)
    for dt in (torch.float16, torch.bfloat16, torch.int64):
        with pytest.raises(ValueError):
            conv(x, ei, attr.to(dt))
    with pytest.raises(ValueError, match="edge_attr"):
        conv(x, ei, attr.clone().requires_grad_(True))           # no silent None gradient
    with pytest.raises(ValueError, match="bf16"):
        plain(x.to(torch.bfloat16), ei)
    for bad in (torch.randn(6, 5), torch.randn(6), torch.randn(2, 6, 4)):
        with pytest.raises(ValueError, match="shape"):
            plain(bad, ei)
    with pytest.raises(ValueError, match="no CPU fallback"):
        plain(x, ei)                                             # CPU tensors
    with pytest.raises(ValueError, match="no CPU fallback"):
        conv(x, ei, attr)
    with pytest.raises(ValueError, match="no CPU fallback"):
        conv(x, ei, attr.double())


def test_the_modular_nets_do_not_take_the_operator():
    """It cannot change width: ``_CONVS`` stays as it is."""
    from dual_dmp_amd import networks
    from dual_dmp_amd.networks import PosNet
    assert not any("cg" in str(k).lower() for k in networks._CONVS)
    for name in ("cg", "cgconv"):
        with pytest.raises(ValueError):
            PosNet(torch.device("cpu"), fused=False, conv=name)


def test_one_gemm_of_each_kind_three_launches_and_nothing_saved_per_edge(monkeypatch):
    from dual_dmp_amd import nn_ops
    seen = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(cg_ops_stub, name)
            if not name.startswith(("gemm_", "cgate_", "colsum", "gatv2_datt", "feast_dc")):
                return fn

            def wrapped(*a, **k):
                seen.append(name)
                return fn(*a, **k)
            return wrapped

    monkeypatch.setattr(nn_ops, "ops", Counting())
    ei, n = small_graph()
    g = cg_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    wf, bf, ws, bs = (q.detach().float().requires_grad_(True) for q in _lin(8, 3, True, 5))
    x = torch.randn(n, 8, requires_grad=True)
    attr = torch.randn(ei.shape[1], 3)
    y = nn_ops._CGConvFn.apply(x, wf, bf, ws, bs, attr, g, 3, False, True)
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    # padded x [12, 8], packed weight [32, 8], row buffer [12, 32], attributes [E, 3], the two transposed edge blocks [3, 8]
    assert sorted(tuple(t.shape) for t in saved) == sorted([(n, 8), (32, 8), (n, 32), (ei.shape[1], 3), (3, 8), (3, 8)])
    assert not any(t.dim() == 2 and t.shape[0] in (g.nnz, ei.shape[1]) and t.shape[1] >= 8 for t in saved)   # nothing C-wide per edge
    y.sum().backward()
    # one GEMM, three launches, the column sums (the two lin biases: C = 8 is a width ops.colsum takes; the partials), one wgrad, one dgrad
    assert seen == ["gemm_nt", "cgate_fwd", "cgate_bwd_row", "cgate_bwd_node", "colsum", "colsum", "gatv2_datt", "gemm_tn", "gemm_nn"]
    assert x.grad.shape == (n, 8) and wf.grad.shape == (8, 19) and bf.grad.shape == (8,)
    # a frozen lin_s and an x without gradient
    del seen[:]
    ws2, bs2 = ws.detach(), bs.detach()
    nn_ops._CGConvFn.apply(x.detach(), wf, bf, ws2, bs2, attr, g, 3, True, False).sum().backward()
    assert seen == ["gemm_nt", "cgate_fwd", "cgate_bwd_row", "cgate_bwd_node", "colsum", "gatv2_datt", "gemm_tn"]
    # dim == 0: no partials, no column sum of them
    del seen[:]
    w0 = [q.detach().float().requires_grad_(True) for q in _lin(8, 0, True, 6)]
    nn_ops._CGConvFn.apply(x, *w0, None, g, 0, False, True).sum().backward()
    assert seen == ["gemm_nt", "cgate_fwd", "cgate_bwd_row", "cgate_bwd_node", "colsum", "colsum", "gemm_tn", "gemm_nn"]


def test_the_three_entry_points_are_declared():
    from dual_dmp_amd import _lib, ops
    protos = _lib.parse_header()
    want = {"ddmp_cgate_fwd_f32": 20, "ddmp_cgate_bwd_row_f32": 23, "ddmp_cgate_bwd_node_f32": 24}
    for name, nargs in want.items():
        assert name in protos and len(protos[name][1]) == nargs and protos[name][0] == "int", name
    assert "#define DDMP_ABI_VERSION 3" in " ".join(open(_lib.HEADER).read().split())
    for name in ("cgate_fwd", "cgate_bwd_row", "cgate_bwd_node"):
        assert callable(getattr(ops, name))
    from dual_dmp_amd.nn_ops import CGConv, _CGConvFn  # noqa: F401

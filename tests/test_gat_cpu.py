"""GATConv: everything that can be checked without a GPU -- the two float64 references against each other, the host side of
``nn_ops._GATConvFn`` over torch restatements of the kernels (tests/gat_ops_stub.py), parameter names / shapes / initialisation,
the refusals, the modular nets' ``conv="gat"`` and the multiplicity claim the coalesced softmax rests on."""
import math

import numpy as np
import pytest
import torch

import gat_ops_stub
from gat_ref import GATConvRef, dense_gat, gat_edge_list, gat_edges


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _with_extras(ei):
    """Duplicates and explicit loops (two on node 5) on top of a mesh, as test_set_values_equals_host_restatement_bit_for_bit adds
    them."""
    extra = torch.tensor([[3, 9, 5, 5, 40], [9, 3, 5, 5, 40]])
    dup = ei[:, :50]
    return torch.cat([ei, extra, dup, dup[[1, 0]]], 1).contiguous()


@pytest.fixture(scope="module")
def meshes():
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    for name, (v, f) in (("ico", synth.icosphere(2)), ("grid", synth.open_grid(9, 7))):
        e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
        out[name] = (_with_extras(torch.cat([e, e[[1, 0]]], 1)), len(v))
    return out


def _params(cin, cout, heads, concat, seed, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=gen, dtype=torch.float64) * 0.5).to(dtype).requires_grad_(True)
    return mk(heads * cout, cin), mk(1, heads, cout), mk(1, heads, cout), mk(heads * cout if concat else cout)


@pytest.mark.parametrize("name", ["ico", "grid"])
@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("concat", [True, False])
def test_the_two_references_agree_in_float64(meshes, name, loops, heads, concat):
    ei, n = meshes[name]
    gen = torch.Generator().manual_seed(n + heads)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    p = _params(5, 4, heads, concat, 3)
    t = torch.randn(n, heads * 4 if concat else 4, generator=gen, dtype=torch.float64)
    outs, grads = [], []
    for fn in (gat_edge_list, dense_gat):
        y = fn(x, ei, *p, heads, concat, 0.2, loops)
        outs.append(y)
        grads.append(torch.autograd.grad((y * t).sum(), (x,) + p))
    assert relerr(outs[0], outs[1]) < 1e-13
    for a, b in zip(*grads):
        assert relerr(a, b) < 1e-12


CASES = [(3, 3, 2), (16, 4, 8), (5, 6, 3), (8, 8, 1)]           # ragged in / total widths go through _pad_cols


@pytest.mark.parametrize("cin,cout,heads", CASES)
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("loops", [True, False])
def test_gatconv_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, cin, cout, heads, concat, loops):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", gat_ops_stub)
    ei, n = meshes["ico"]
    gen = torch.Generator().manual_seed(cin * 7 + heads)
    x64 = torch.randn(n, cin, generator=gen, dtype=torch.float64)
    p64 = _params(cin, cout, heads, concat, 11)
    t = torch.randn(n, heads * cout if concat else cout, generator=gen, dtype=torch.float64)
    xr = x64.clone().requires_grad_(True)
    yr = gat_edge_list(xr, ei, *p64, heads, concat, 0.2, loops)
    gr = torch.autograd.grad((yr * t).sum(), (xr,) + p64)
    x = x64.float().requires_grad_(True)
    p = tuple(q.detach().float().requires_grad_(True) for q in p64)
    g = gat_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=loops)
    y = nn_ops._GATConvFn.apply(x, p[0], p[1], p[2], p[3], g, heads, concat, 0.2)
    gs = torch.autograd.grad((y * t.float()).sum(), (x,) + p)
    assert y.shape == yr.shape and relerr(y, yr) < 1e-5
    for a, b, nm in zip(gs, gr, ("dx", "dW", "datt_src", "datt_dst", "db")):
        assert a.shape == b.shape, nm
        assert relerr(a, b) < 1e-5, (nm, relerr(a, b))


def test_parameter_names_shapes_and_init():
    from dual_dmp_amd.nn_ops import GATConv
    torch.manual_seed(0)
    conv = GATConv(40, 24, heads=3)
    assert conv.lin_dst is conv.lin_src
    sd = conv.state_dict()
    assert list(sd) == ["att_src", "att_dst", "bias", "lin_src.weight", "lin_dst.weight"]
    assert [n for n, _ in conv.named_parameters()] == ["att_src", "att_dst", "bias", "lin_src.weight"]
    assert sd["lin_src.weight"].shape == (72, 40) and sd["att_src"].shape == (1, 3, 24) and sd["att_dst"].shape == (1, 3, 24)
    assert sd["bias"].shape == (72,) and not sd["bias"].any()
    a, b = math.sqrt(6.0 / (40 + 72)), math.sqrt(6.0 / (3 + 24))
    w = sd["lin_src.weight"]
    assert w.abs().max() <= a and w.abs().max() > 0.9 * a and abs(float(w.mean())) < 0.1 * a
    for t in (sd["att_src"], sd["att_dst"]):
        assert t.abs().max() <= b and t.abs().max() > 0.8 * b
    assert GATConv(40, 24, heads=3, concat=False).bias.shape == (24,)
    assert GATConv(40, 24, bias=False).bias is None
    conv2 = GATConv(40, 24, heads=3)
    conv2.load_state_dict(sd)
    assert torch.equal(conv2.lin_dst.weight, w)


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import GATConv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    with pytest.raises(ValueError):
        GATConv((4, 4), 8)
    with pytest.raises(ValueError):
        GATConv(4, 8, edge_dim=2)
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    conv = GATConv(4, 8, heads=2)
    for kw in (dict(edge_attr=torch.randn(2, 3)), dict(size=(6, 6)), dict(return_attention_weights=True)):
        with pytest.raises(ValueError):
            conv(x, ei, **kw)
    with pytest.raises(ValueError):
        conv((x, x), ei)
    with pytest.raises(ValueError):
        conv(x.to(torch.bfloat16), ei)
    drop = GATConv(4, 8, dropout=0.5)
    with pytest.raises(ValueError):
        drop(x, ei)
    with pytest.raises(ops.DdmpError):
        conv(x, ei)                                              # a CPU x: no CPU fallback
    with pytest.raises(ops.DdmpError):
        drop.eval()(x, ei)                                       # dropout in eval mode is the identity: only the CPU x is refused
    with pytest.raises(ValueError):
        ops.graph_for(ei, 6, norm="gat", edge_weight=torch.ones(2))


def test_modular_nets_take_conv_gat():
    from dual_dmp_amd.networks import NormalNet, PosNet
    from dual_dmp_amd.nn_ops import GATConv
    from dual_dmp_amd.engine import POS_WIDTHS
    net = PosNet(torch.device("cpu"), fused=False, conv="gat", heads=4)
    convs = [getattr(net, "conv%d" % i) for i in range(1, 13)]
    assert all(isinstance(c, GATConv) for c in convs)
    assert [(c.in_channels, c.out_channels * c.heads, c.heads) for c in convs] == [(POS_WIDTHS[i], POS_WIDTHS[i + 1], 4) for i in range(12)]
    assert "conv1.lin_src.weight" in net.state_dict() and "conv12.att_dst" in net.state_dict()
    assert isinstance(NormalNet(torch.device("cpu"), fused=False, conv="gat", heads=2).conv1, GATConv)
    for mk in (PosNet, NormalNet):
        with pytest.raises(ValueError):
            mk(torch.device("cpu"), fused=True, conv="gat", heads=4)
        with pytest.raises(ValueError):
            mk(torch.device("cpu"), fused=False, conv="gat", heads=3)      # 32 is not divisible by 3
        with pytest.raises(ValueError):
            mk(torch.device("cpu"), fused=False, conv="gatv2")


@pytest.mark.parametrize("loops", [True, False])
def test_coalesced_multiplicities_equal_the_reference_edge_counts(meshes, loops):
    """A softmax over a multiset equals the softmax with a_e exp(z_e) terms: a_e must be the number of reference edges per
    (target, source), and 1 on every loop entry under GV_LOOPS -- also on node 5, which has two explicit loops."""
    from dual_dmp_amd import ops
    ei, n = meshes["grid"]
    flags = ops.GV_LOOPS if loops else 0
    t = ops.csr_build_valued_host(ei.numpy(), n, flags)
    a = ops.valued_values_host(t, None, flags)[0]
    src, dst = gat_edges(ei, n, loops)
    cnt = np.zeros((n, n))
    np.add.at(cnt, (dst.numpy(), src.numpy()), 1.0)
    rows = np.repeat(np.arange(n), np.diff(t["rowptr"]))
    assert len(a) == int((cnt > 0).sum())                        # one entry per (target, source) pair of the reference
    assert np.array_equal(a, cnt[rows, t["col"]])
    assert a.max() >= 2                                          # (the duplicates are there)
    if loops:
        assert np.all(a[rows == t["col"]] == 1.0) and int((rows == t["col"]).sum()) == n
    else:
        assert cnt[5, 5] == 2 and a[(rows == 5) & (t["col"] == 5)] == 2.0
    m = t["mirror"]
    assert np.array_equal(rows[m], t["col"]) and np.array_equal(t["col"][m], rows)


def test_graph_for_gat_never_calls_set_values_and_has_its_own_key(monkeypatch):
    from dual_dmp_amd import ops
    made = []

    class G:
        valued, values_key = 0, None

        def set_values(self, *a, **k):
            raise AssertionError("set_values on an attention graph")

    def fake(edge_index, num_nodes, norm="gcn", valued=None):
        made.append((norm, valued))
        return G()

    monkeypatch.setattr(ops.Graph, "from_edge_index", staticmethod(fake))
    monkeypatch.setattr(ops, "_graph_cache", {})
    ei = torch.tensor([[0, 1], [1, 0]])
    g1 = ops.graph_for(ei, 2, norm="gat")
    g2 = ops.graph_for(ei, 2, norm="gat")
    g3 = ops.graph_for(ei, 2, norm="gat", add_self_loops=False)
    g4 = ops.graph_for(ei, 2, add_self_loops=False, normalize=False)      # a GCNConv graph with the same flags (0)
    assert g1 is g2 and g3 is not g1 and g4 is not g3
    assert made == [("gcn", ops.GV_LOOPS), ("gcn", 0), ("gcn", 0)]
    assert g1.values_key == ("ones",)

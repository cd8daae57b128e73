"""FeaStConv: everything that can be checked without a GPU -- the two float64 references against each other, the host side of
``nn_ops._FeaStConvFn`` over torch restatements of the kernels (tests/feast_ops_stub.py), the heads = 1 special case against a
plain mean aggregation, parameter names / shapes / initialisation, the refusals, and the modular nets' ``conv="feast"``."""
import math

import pytest
import torch

import feast_ops_stub
from feast_ref import FeaStConvRef, dense_feast, feast_edge_list, feast_edges


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _with_extras(ei):
    """Duplicates and explicit loops (two on node 5) on top of a mesh, as test_gat_cpu.py adds them."""
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


def _params(cin, cout, heads, seed, dtype=torch.float64):
    """(lin.weight, u.weight, c, bias), each requiring grad."""
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=gen, dtype=torch.float64) * 0.5).to(dtype).requires_grad_(True)
    return mk(heads * cout, cin), mk(heads, cin), mk(heads), mk(cout)


@pytest.mark.parametrize("name", ["ico", "grid"])
@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("heads", [1, 3])
def test_the_two_references_agree_in_float64(meshes, name, loops, heads):
    ei, n = meshes[name]
    gen = torch.Generator().manual_seed(n + heads)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    p = _params(5, 4, heads, 3)
    t = torch.randn(n, 4, generator=gen, dtype=torch.float64)
    outs, grads = [], []
    for fn in (feast_edge_list, dense_feast):
        y = fn(x, ei, *p, heads, loops)
        outs.append(y)
        grads.append(torch.autograd.grad((y * t).sum(), (x,) + p, allow_unused=True))
    assert relerr(outs[0], outs[1]) < 1e-13
    for a, b, nm in zip(*grads, ("dx", "dW", "du", "dc", "db")):
        if heads == 1 and nm in ("du", "dc"):                    # a softmax over one head is constant: both are zero (or unused)
            for v in (a, b):
                assert v is None or float(v.abs().max()) < 1e-12
            continue
        assert relerr(a, b) < 1e-12, (nm, relerr(a, b))


CASES = [(3, 3, 2), (16, 4, 8), (5, 6, 3), (8, 8, 1)]           # ragged in / packed widths go through the padding


@pytest.mark.parametrize("cin,cout,heads", CASES)
@pytest.mark.parametrize("loops", [True, False])
def test_feastconv_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, cin, cout, heads, loops):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", feast_ops_stub)
    ei, n = meshes["ico"]
    gen = torch.Generator().manual_seed(cin * 7 + heads)
    x64 = torch.randn(n, cin, generator=gen, dtype=torch.float64)
    p64 = _params(cin, cout, heads, 11)
    t = torch.randn(n, cout, generator=gen, dtype=torch.float64)
    xr = x64.clone().requires_grad_(True)
    yr = feast_edge_list(xr, ei, *p64, heads, loops)
    gr = torch.autograd.grad((yr * t).sum(), (xr,) + p64)
    x = x64.float().requires_grad_(True)
    p = tuple(q.detach().float().requires_grad_(True) for q in p64)
    g = feast_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=loops)
    del feast_ops_stub.calls[:]
    y = nn_ops._FeaStConvFn.apply(x, p[0], p[1], p[2], p[3], g, heads)
    gs = torch.autograd.grad((y * t.float()).sum(), (x,) + p)
    assert feast_ops_stub.calls == ["feast_fwd", "feast_bwd_edge", "feast_bwd_node", "feast_dc"]
    assert y.shape == yr.shape == (n, cout) and relerr(y, yr) < 1e-5
    scale = float(gr[1].norm())                                  # heads = 1: du and dc are zero, compared in absolute terms
    for a, b, nm in zip(gs, gr, ("dx", "dW", "du", "dc", "db")):
        assert a.shape == b.shape, nm
        if heads == 1 and nm in ("du", "dc"):
            assert float(b.abs().max()) < 1e-12 and float(a.double().norm()) <= 1e-5 * scale, nm
        else:
            assert relerr(a, b) < 1e-5, (nm, relerr(a, b))


@pytest.mark.parametrize("loops", [True, False])
def test_one_head_is_the_plain_mean_aggregation(meshes, loops):
    ei, n = meshes["grid"]
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(n, 6, generator=gen, dtype=torch.float64)
    w, u, c, b = (q.detach() for q in _params(6, 4, 1, 9))
    src, dst = feast_edges(ei, n, loops)
    h = x @ w.t()
    cnt = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(len(dst), dtype=torch.float64))
    mean = torch.zeros((n, 4), dtype=torch.float64).index_add_(0, dst, h[src]) / cnt.clamp(min=1).unsqueeze(1) + b
    assert relerr(feast_edge_list(x, ei, w, u, c, b, 1, loops), mean) < 1e-14
    assert relerr(dense_feast(x, ei, w, u, c, b, 1, loops), mean) < 1e-14
    g = feast_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=loops)
    buf = torch.cat([h, x @ u.t()], 1).float()
    y, beta = feast_ops_stub.feast_fwd(g, buf[:, :4], buf[:, 4:5], c.float(), 1, bias=b.float())
    assert relerr(y, mean) < 1e-6
    assert torch.allclose(torch.zeros(n, dtype=torch.float64).index_add_(0, g.row, beta.double()[:, 0]), (cnt > 0).double(), atol=1e-6)


def test_parameter_names_shapes_and_init():
    from dual_dmp_amd.nn_ops import FeaStConv
    torch.manual_seed(0)
    conv = FeaStConv(40, 24, heads=3)
    sd = conv.state_dict()
    assert list(sd) == ["c", "bias", "lin.weight", "u.weight"]
    assert [n for n, _ in conv.named_parameters()] == ["c", "bias", "lin.weight", "u.weight"]
    assert sd["lin.weight"].shape == (72, 40) and sd["u.weight"].shape == (3, 40) and sd["c"].shape == (3,)
    assert sd["bias"].shape == (24,)
    a = 1.0 / math.sqrt(40)
    for t, frac in ((sd["lin.weight"], 0.95), (sd["u.weight"], 0.8)):
        assert t.abs().max() <= a and t.abs().max() > frac * a and abs(float(t.mean())) < 0.2 * a
    big = FeaStConv(8, 4096, heads=4)                            # normal(0, 0.1) on c and bias
    assert abs(float(big.bias.detach().std()) - 0.1) < 0.01 and abs(float(big.bias.detach().mean())) < 0.01
    assert float(big.c.detach().abs().max()) < 1.0 and bool(big.c.detach().abs().sum() > 0)
    assert FeaStConv(40, 24, bias=False).bias is None
    assert FeaStConv(40, 24, heads=2, aggr="mean").heads == 2
    conv2 = FeaStConv(40, 24, heads=3)
    conv2.load_state_dict(sd)
    assert torch.equal(conv2.u.weight, sd["u.weight"])
    ref = FeaStConvRef(40, 24, heads=3)
    assert sorted(n for n, _ in ref.named_parameters()) == sorted(sd)
    assert [tuple(p.shape) for _, p in sorted(ref.named_parameters())] == [tuple(sd[k].shape) for k in sorted(sd)]


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import FeaStConv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    with pytest.raises(ValueError):
        FeaStConv((4, 4), 8)
    for aggr in ("add", "max", "sum"):
        with pytest.raises(ValueError):
            FeaStConv(4, 8, aggr=aggr)
    for heads in (0, -1, 2.0):
        with pytest.raises(ValueError):
            FeaStConv(4, 8, heads=heads)
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    conv = FeaStConv(4, 8, heads=2)
    with pytest.raises(ValueError):
        conv((x, x), ei)
    with pytest.raises(ValueError):
        conv(x.to(torch.bfloat16), ei)
    with pytest.raises(ValueError):
        conv(torch.randn(6, 5), ei)
    with pytest.raises(ValueError):
        conv(torch.randn(6), ei)
    with pytest.raises(ops.DdmpError):
        conv(x, ei)                                              # a CPU x: no CPU fallback


def test_modular_nets_take_conv_feast():
    from dual_dmp_amd.networks import NormalNet, PosNet
    from dual_dmp_amd.nn_ops import FeaStConv
    from dual_dmp_amd.engine import NORM_WIDTHS, POS_WIDTHS
    for mk, widths in ((PosNet, POS_WIDTHS), (NormalNet, NORM_WIDTHS)):
        net = mk(torch.device("cpu"), fused=False, conv="feast", heads=4)
        convs = [getattr(net, "conv%d" % i) for i in range(1, 13)]
        assert all(isinstance(c, FeaStConv) for c in convs)
        assert [(c.in_channels, c.out_channels, c.heads) for c in convs] == [(widths[i], widths[i + 1], 4) for i in range(12)]
        names = [n for n, _ in net.named_parameters()]
        for i in (1, 12):
            for leaf in ("lin.weight", "u.weight", "c", "bias"):
                assert "conv%d.%s" % (i, leaf) in names
        assert len([n for n in names if n.startswith("conv")]) == 12 * 4
        assert net.conv3.lin.weight.shape == (4 * widths[3], widths[2]) and net.conv3.u.weight.shape == (4, widths[2])
        assert isinstance(mk(torch.device("cpu"), fused=False, conv="feast", heads=3).conv1, FeaStConv)      # no divisibility rule
        with pytest.raises(ValueError):
            mk(torch.device("cpu"), fused=True, conv="feast", heads=4)
        for bad in ("sage", "gatv2", "feastnet", "FEAST"):
            with pytest.raises(ValueError) as info:
                mk(torch.device("cpu"), fused=False, conv=bad)
            assert "feast" in str(info.value)


def test_the_default_net_is_unchanged():
    """conv="gcn" stays the default: the reference's names, and the same RNG draws whether or not it is spelled out."""
    from dual_dmp_amd.networks import PosNet
    from dual_dmp_amd.nn_ops import GCNConv
    torch.manual_seed(2)
    net = PosNet("cpu", fused=False)
    torch.manual_seed(2)
    again = PosNet("cpu", fused=False, conv="gcn", heads=4)      # heads is not a GCN option: no draw depends on it
    names = [n for n, _ in net.named_parameters()]
    assert names[:2] == ["conv1.bias", "conv1.lin.weight"] and names[-1] == "bn12.bias" and len(names) == 12 * 2 + 4 + 12 * 2
    assert all(isinstance(getattr(net, "conv%d" % i), GCNConv) for i in range(1, 13))
    for (n1, p1), (n2, p2) in zip(net.named_parameters(), again.named_parameters()):
        assert n1 == n2 and torch.equal(p1, p2)
    assert sum(p.numel() for p in net.parameters()) == 749955

"""ResGatedGraphConv: everything that can be checked without a GPU -- the host side of ``nn_ops._ResGatedFn`` over torch
restatements of the kernels (tests/resgated_ops_stub.py) against the float64 edge-list reference (tests/resgated_ref.py),
parameter names / shapes / initialisation, the refusals, the modular nets' ``conv="resgated"`` and the declarations of the new
entry points."""
import math

import pytest
import torch

import resgated_ops_stub
from resgated_ref import ResGatedGraphConvRef, resgated_core, resgated_edge_list
from test_gat_cpu import relerr


@pytest.fixture(scope="module")
def meshes():
    """name -> (edge_index, n): "grid" a small open grid, both directions of every edge; "iso" the same with one more node
    without any edge (an empty row); "asym" the grid with ASYMMETRIC multiplicities: a few edges a -> b twice or three times
    while b -> a stays single (the structure stays symmetric)."""
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    v, f = synth.open_grid(9, 7)
    e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
    ei = torch.cat([e, e[[1, 0]]], 1).contiguous()
    n = len(v)
    asym = torch.cat([ei, ei[:, :5], ei[:, 2:4]], 1).contiguous()
    return {"grid": (ei, n), "iso": (ei, n + 1), "asym": (asym, n)}


def _params(cin, cout, root, bias, seed, dtype=torch.float64):
    """-> (wk, bk, wq, bq, wv, bv, ws, bias); None where the configuration has none."""
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=gen, dtype=torch.float64) * 0.5).to(dtype).requires_grad_(True)
    kqv = (mk(cout, cin), mk(cout), mk(cout, cin), mk(cout), mk(cout, cin), mk(cout))
    return kqv + (mk(cout, cin) if root else None, mk(cout) if bias else None)


def _grads(y, t, leaves):
    return torch.autograd.grad((y * t).sum(), [p for p in leaves if p is not None])


NAMES = ("dx", "dW_k", "db_k", "dW_q", "db_q", "dW_v", "db_v", "dW_s", "db")


def test_the_reference_on_a_graph_done_by_hand():
    """Node 1 feeds node 0 twice, node 2 feeds it once, node 2 has no incoming edge: the gate per channel, the duplicates, the
    skip and the bias, written out."""
    x = torch.tensor([[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]], dtype=torch.float64)
    ei = torch.tensor([[1, 1, 2], [0, 0, 0]])
    eye, zero = torch.eye(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    y = resgated_edge_list(x, ei, eye, zero, eye, zero, eye, zero, 2 * eye, zero + 1)
    sig = lambda a: 1.0 / (1.0 + math.exp(-a))
    m0 = torch.tensor([2 * sig(1.0) * 0.0 + sig(2.0) * 1.0, 2 * sig(2.0) * 2.0 + sig(1.0) * 1.0], dtype=torch.float64)
    assert torch.allclose(y[0], m0 + 2 * x[0] + 1, atol=1e-15) and torch.equal(y[1:], 2 * x[1:] + 1)
    assert torch.equal(resgated_core(x, x, x, ei)[1:], torch.zeros(2, 2, dtype=torch.float64))


@pytest.mark.parametrize("name", ["grid", "iso", "asym"])
@pytest.mark.parametrize("root", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("cin,cout", [(5, 3), (6, 8)])
def test_resgated_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, name, root, bias, cin, cout):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", resgated_ops_stub)
    ei, n = meshes[name]
    gen = torch.Generator().manual_seed(cin * 7 + cout)
    x64 = torch.randn(n, cin, generator=gen, dtype=torch.float64)
    p64 = _params(cin, cout, root, bias, 11)
    t = torch.randn(n, cout, generator=gen, dtype=torch.float64)
    xr = x64.clone().requires_grad_(True)
    yr = resgated_edge_list(xr, ei, *p64)
    gr = _grads(yr, t, (xr,) + p64)
    x = x64.float().requires_grad_(True)
    p = tuple(None if q is None else q.detach().float().requires_grad_(True) for q in p64)
    g = resgated_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    if name == "asym":
        assert bool((g.a != g.a[g.mirror]).any())                # the multiplicities are NOT symmetric
    del resgated_ops_stub.calls[:]
    y = nn_ops._ResGatedFn.apply(x, *p, g)
    gs = _grads(y, t.float(), (x,) + p)
    assert resgated_ops_stub.calls == ["rgate_fwd" + ("+skip" if root else "") + ("+bias" if bias else ""), "rgate_bwd_row",
                                       "rgate_bwd_node" + ("+skip" if root else "")]
    assert y.shape == yr.shape and relerr(y, yr) < 1e-5
    if name == "iso":                                            # the node without incoming edges: lin_skip(x_i) + bias
        want = (x64[-1] @ p64[6].detach().t() if root else 0.0) + (p64[7].detach() if bias else 0.0)
        assert float((y[-1].detach().double() - want).abs().max()) < 1e-5
    names = [nm for nm, q in zip(NAMES, (x,) + p) if q is not None]
    assert len(gs) == len(gr) == len(names)
    for a, b, nm in zip(gs, gr, names):
        assert a.shape == b.shape, nm
        assert relerr(a, b) < 1e-5, (nm, relerr(a, b))


def test_the_stub_reads_the_mirrored_multiplicity(meshes):
    """The node side with ``mult[e]`` in place of ``mult[mirror[e]]`` is a different number on the asymmetric graph -- what the
    "asym" case above is for."""
    ei, n = meshes["asym"]
    g = resgated_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    gen = torch.Generator().manual_seed(2)
    k, q, v, dout = (torch.randn(n, 4, generator=gen) for _ in range(4))
    dq, dv = resgated_ops_stub.rgate_bwd_node(g, dout, k, q, v)
    a = g.a
    g.a = a[g.mirror]                                            # mirror is an involution: the stub now reads mult[e]
    dq2, dv2 = resgated_ops_stub.rgate_bwd_node(g, dout, k, q, v)
    g.a = a
    assert relerr(dq2, dq) > 1e-3 and relerr(dv2, dv) > 1e-3


def test_the_function_makes_one_gemm_of_each_kind_and_saves_nothing_per_entry(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    seen = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(resgated_ops_stub, name)
            if not name.startswith(("gemm_", "rgate_")):
                return fn

            def wrapped(*a, **k):
                seen.append(name)
                return fn(*a, **k)
            return wrapped

    monkeypatch.setattr(nn_ops, "ops", Counting())
    ei, n = meshes["grid"]
    g = resgated_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    p = tuple(q.detach().float().requires_grad_(True) for q in _params(6, 4, True, True, 5))
    x = torch.randn(n, 6, requires_grad=True)
    y = nn_ops._ResGatedFn.apply(x, *p, g)
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 3 and all(t.shape[0] in (n, 16) for t in saved)     # padded x, packed weight [16, 8], row buffer
    assert not any(t.shape[0] == g.nnz for t in saved)
    y.sum().backward()
    assert seen == ["gemm_nt", "rgate_fwd", "rgate_bwd_row", "rgate_bwd_node", "gemm_tn", "gemm_nn"]


def test_needs_input_grad_is_respected(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", resgated_ops_stub)
    ei, n = meshes["grid"]
    g = resgated_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    p = list(q.detach().float().requires_grad_(True) for q in _params(6, 4, True, True, 5))
    p[1] = p[1].detach()                                         # lin_key.bias frozen
    p[6] = p[6].detach()                                         # lin_skip.weight frozen
    x = torch.randn(n, 6)                                        # no gradient for x
    nn_ops._ResGatedFn.apply(x, *p, g).sum().backward()
    assert x.grad is None and p[1].grad is None and p[6].grad is None
    assert all(p[i].grad is not None for i in (0, 2, 3, 4, 5, 7))


def test_parameter_names_shapes_and_init():
    from dual_dmp_amd.nn_ops import ResGatedGraphConv
    torch.manual_seed(0)
    conv = ResGatedGraphConv(40, 24)
    sd = conv.state_dict()
    assert sorted(sd) == sorted(["lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight",
                                 "lin_value.bias", "lin_skip.weight", "bias"])
    for k in ("lin_key", "lin_query", "lin_value"):
        assert sd[k + ".weight"].shape == (24, 40) and sd[k + ".bias"].shape == (24,)
    assert sd["lin_skip.weight"].shape == (24, 40) and conv.lin_skip.bias is None
    assert sd["bias"].shape == (24,) and not sd["bias"].any()
    a = 1.0 / math.sqrt(40)
    for k, v in sd.items():
        if k != "bias":
            assert v.abs().max() <= a and v.abs().max() > 0.8 * a, k
    assert abs(float(sd["lin_key.weight"].mean())) < 0.1 * a
    assert not torch.equal(sd["lin_key.weight"], sd["lin_query.weight"])
    assert isinstance(conv.act, torch.nn.Sigmoid) and conv.root_weight
    noroot = ResGatedGraphConv(40, 24, root_weight=False)
    assert noroot.lin_skip is None and "lin_skip.weight" not in noroot.state_dict() and noroot.bias is not None
    nob = ResGatedGraphConv(40, 24, bias=False)
    assert nob.bias is None and "bias" not in nob.state_dict() and nob.lin_key.bias is not None and nob.lin_skip is not None
    assert sorted(ResGatedGraphConv(4, 8, act=torch.nn.Sigmoid(), aggr="add").state_dict()) == sorted(sd)
    conv2 = ResGatedGraphConv(40, 24)
    conv2.load_state_dict(sd)
    assert torch.equal(conv2.lin_value.weight, sd["lin_value.weight"]) and torch.equal(conv2.lin_skip.weight, sd["lin_skip.weight"])
    ref = ResGatedGraphConvRef(40, 24, dtype=torch.float32).load_from(conv)
    assert sorted(ref.state_dict()) == sorted(sd) and torch.equal(ref.lin_query.bias, conv.lin_query.bias)
    assert "40, 24" in repr(conv) and "root_weight=True" in repr(conv)
    with torch.no_grad():
        conv.bias.fill_(1.0)
    before = conv.lin_value.weight.detach().clone()
    conv.reset_parameters()
    assert not torch.equal(conv.lin_value.weight, before) and conv.lin_value.weight.abs().max() <= a
    assert not conv.bias.any()


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import ResGatedGraphConv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    with pytest.raises(ValueError):
        ResGatedGraphConv((4, 4), 8)
    for act in (torch.nn.ReLU(), torch.sigmoid, None, torch.nn.Sigmoid):
        with pytest.raises(ValueError, match="Sigmoid"):
            ResGatedGraphConv(4, 8, act=act)
    for aggr in ("mean", "max", None):
        with pytest.raises(ValueError, match="aggr"):
            ResGatedGraphConv(4, 8, aggr=aggr)
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    conv = ResGatedGraphConv(4, 8)
    with pytest.raises(ValueError):
        conv((x, x), ei)
    with pytest.raises(ValueError, match="bf16"):
        conv(x.to(torch.bfloat16), ei)
    for bad in (torch.randn(6, 5), torch.randn(6), torch.randn(2, 6, 4)):
        with pytest.raises(ValueError, match="shape"):
            conv(bad, ei)
    with pytest.raises(ValueError, match="no CPU fallback"):
        conv(x, ei)                                              # a CPU x


def test_modular_nets_take_conv_resgated():
    from dual_dmp_amd.engine import NORM_WIDTHS, POS_WIDTHS
    from dual_dmp_amd.networks import NormalNet, PosNet
    from dual_dmp_amd.nn_ops import ResGatedGraphConv
    for mk, widths in ((PosNet, POS_WIDTHS), (NormalNet, NORM_WIDTHS)):
        net = mk(torch.device("cpu"), fused=False, conv="resgated")
        convs = [getattr(net, "conv%d" % i) for i in range(1, 13)]
        assert all(isinstance(c, ResGatedGraphConv) and c.root_weight and c.bias is not None for c in convs)
        assert [(c.in_channels, c.out_channels) for c in convs] == [(widths[i], widths[i + 1]) for i in range(12)]
        sd = net.state_dict()
        for i in (1, 12):
            for leaf in ("lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight",
                         "lin_value.bias", "lin_skip.weight", "bias"):
                assert "conv%d.%s" % (i, leaf) in sd
        assert len([k for k in sd if k.startswith("conv")]) == 12 * 8
        assert net.conv3.lin_skip.weight.shape == (widths[3], widths[2])
        with pytest.raises(ValueError):
            mk(torch.device("cpu"), fused=True, conv="resgated")
        for bad in ("gatv2", "sage"):
            with pytest.raises(ValueError) as info:
                mk(torch.device("cpu"), fused=False, conv=bad)
            for name in ("gcn", "cheb", "gat", "feast", "edge", "gmm", "transformer", "resgated"):
                assert "'%s'" % name in str(info.value)


def test_the_new_entry_points_are_declared():
    from dual_dmp_amd import _lib, ops
    protos = _lib.parse_header()
    want = {"ddmp_rgate_fwd_f32": 14, "ddmp_rgate_bwd_row_f32": 13, "ddmp_rgate_bwd_node_f32": 17}
    for name, nargs in want.items():
        assert name in protos and len(protos[name][1]) == nargs and protos[name][0] == "int", name
    assert "#define DDMP_ABI_VERSION 3" in " ".join(open(_lib.HEADER).read().split())
    for name in ("rgate_fwd", "rgate_bwd_row", "rgate_bwd_node"):
        assert callable(getattr(ops, name))
    from dual_dmp_amd.nn_ops import ResGatedGraphConv, _ResGatedFn  # noqa: F401

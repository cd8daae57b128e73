"""TransformerConv: everything that can be checked without a GPU -- the two float64 references against each other, the host side
of ``nn_ops._TransformerConvFn`` over torch restatements of the kernels (tests/transformer_ops_stub.py), parameter names / shapes
/ initialisation, the refusals, the modular nets' ``conv="transformer"`` and the declarations of the new entry points."""
import math

import pytest
import torch

import transformer_ops_stub
from transformer_ref import TransformerConvRef, dense_transformer, transformer_edge_list
from test_gat_cpu import _with_extras, relerr


@pytest.fixture(scope="module")
def meshes():
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    for name, (v, f) in (("ico", synth.icosphere(2)), ("grid", synth.open_grid(9, 7))):
        e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
        out[name] = (_with_extras(torch.cat([e, e[[1, 0]]], 1)), len(v))
    return out


def _params(cin, cout, heads, concat, beta, root, seed, skip_bias=True, dtype=torch.float64):
    """-> (wq, bq, wk, bk, wv, bv, ws, bs, wb); None where the configuration has none."""
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=gen, dtype=torch.float64) * 0.5).to(dtype).requires_grad_(True)
    hc = heads * cout
    sw = hc if concat else cout
    qkv = (mk(hc, cin), mk(hc), mk(hc, cin), mk(hc), mk(hc, cin), mk(hc))
    ws, bs = (mk(sw, cin), mk(sw) if skip_bias else None) if root else (None, None)
    return qkv + (ws, bs, mk(1, 3 * sw) if beta and root else None)


def _grads(y, t, leaves):
    leaves = [p for p in leaves if p is not None]
    return torch.autograd.grad((y * t).sum(), leaves)


def _graderrs(got, ref):
    """rel-L2 of every gradient in the order (x, wq, bq, wk, bk, ...).  The gradient of ``lin_key.bias`` (index 4) is ZERO in
    exact arithmetic -- the bias adds ``Q[i,h,:] . bk[h,:]`` to every score of row i, and a softmax does not see a constant -- so
    both sides hold rounding noise only: its error is taken relative to the norm of its sibling of the same shape, the gradient of
    ``lin_query.bias`` (index 2)."""
    return [float((a.double() - b.double()).norm() / ((ref[2] if i == 4 else b).double().norm() + 1e-30))
            for i, (a, b) in enumerate(zip(got, ref))]


@pytest.mark.parametrize("name", ["ico", "grid"])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("beta", [True, False])
@pytest.mark.parametrize("root", [True, False])
def test_the_two_references_agree_in_float64(meshes, name, heads, concat, beta, root):
    ei, n = meshes[name]
    gen = torch.Generator().manual_seed(n + heads)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    p = _params(5, 4, heads, concat, beta, root, 3)
    t = torch.randn(n, heads * 4 if concat else 4, generator=gen, dtype=torch.float64)
    outs, grads = [], []
    for fn in (transformer_edge_list, dense_transformer):
        y = fn(x, ei, *p, heads, concat)
        outs.append(y)
        grads.append(_grads(y, t, (x,) + p))
    assert relerr(outs[0], outs[1]) < 1e-13
    assert max(_graderrs(*grads)) < 1e-12
    assert float(grads[0][4].abs().max()) < 1e-12 * float(grads[0][2].abs().max())     # (lin_key.bias: see _graderrs)


def test_the_reference_on_a_graph_done_by_hand():
    """Two nodes feeding node 0 (one of them twice), node 2 without incoming edges: the softmax over the multiset, m = 0 on the
    empty row, the skip and the gate, written out."""
    x = torch.tensor([[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]], dtype=torch.float64)
    ei = torch.tensor([[1, 1, 2], [0, 0, 0]])
    eye, zero = torch.eye(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    wb = torch.tensor([[0.5, -1.0, 0.25, 0.0, 1.0, 2.0]], dtype=torch.float64)
    y = transformer_edge_list(x, ei, eye, zero, eye, zero, eye, zero, 2 * eye, zero + 1, None, 1)
    z1, z2 = 0.0, 1.0 / math.sqrt(2.0)                           # q_0 . k_1, q_0 . k_2, over sqrt(C)
    a2 = math.exp(z2) / (2 * math.exp(z1) + math.exp(z2))
    m0 = (1 - a2) * x[1] + a2 * x[2]
    assert torch.allclose(y[0], m0 + 2 * x[0] + 1, atol=1e-15) and torch.equal(y[1:], 2 * x[1:] + 1)
    yb = transformer_edge_list(x, ei, eye, zero, eye, zero, eye, zero, 2 * eye, zero + 1, wb, 1)
    xr = 2 * x[0] + 1
    b = torch.sigmoid((torch.cat([m0, xr, m0 - xr]) * wb[0]).sum())
    assert torch.allclose(yb[0], b * xr + (1 - b) * m0, atol=1e-15)


CASES = [(3, 3, 2), (16, 4, 8), (5, 6, 3), (8, 8, 1)]           # ragged in / total widths go through the packing's padding
NAMES = ("dx", "dW_q", "db_q", "dW_k", "db_k", "dW_v", "db_v", "dW_s", "db_s", "dW_b")
MODES = [(True, True, False), (False, True, False), (True, False, False), (True, True, True), (False, True, True)]


def _apply(nn_ops, x, p, g, heads, concat):
    """What ``TransformerConv.forward`` does with the function's outputs."""
    out = nn_ops._TransformerConvFn.apply(x, *p[:8], g, heads, concat, p[8] is not None)
    if p[8] is None:
        return out
    m, x_r = out
    b = torch.sigmoid(torch.cat([m, x_r, m - x_r], dim=-1) @ p[8].t())
    return b * x_r + (1 - b) * m


@pytest.mark.parametrize("cin,cout,heads", CASES)
@pytest.mark.parametrize("concat,root,beta", MODES)
@pytest.mark.parametrize("skip_bias", [True, False])
def test_transformerconv_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, cin, cout, heads, concat, root, beta, skip_bias):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", transformer_ops_stub)
    ei, n = meshes["ico"]
    n += 1                                                       # one more node without any edge: an empty row
    gen = torch.Generator().manual_seed(cin * 7 + heads)
    x64 = torch.randn(n, cin, generator=gen, dtype=torch.float64)
    p64 = _params(cin, cout, heads, concat, beta, root, 11, skip_bias=skip_bias)
    t = torch.randn(n, heads * cout if concat else cout, generator=gen, dtype=torch.float64)
    xr = x64.clone().requires_grad_(True)
    yr = transformer_edge_list(xr, ei, *p64, heads, concat)
    gr = _grads(yr, t, (xr,) + p64)
    x = x64.float().requires_grad_(True)
    p = tuple(None if q is None else q.detach().float().requires_grad_(True) for q in p64)
    g = transformer_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    del transformer_ops_stub.calls[:]
    y = _apply(nn_ops, x, p, g, heads, concat)
    gs = _grads(y, t.float(), (x,) + p)
    fused = concat and root and not beta                         # the skip goes through the kernels only there
    assert transformer_ops_stub.calls == (["tconv_fwd+skip", "tconv_bwd_edge", "tconv_bwd_node+skip"] if fused else
                                          ["tconv_fwd", "tconv_bwd_edge", "tconv_bwd_node"])
    assert y.shape == yr.shape and relerr(y, yr) < 1e-5
    names = [nm for nm, q in zip(NAMES, (x,) + p) if q is not None]
    assert len(gs) == len(gr) == len(names)
    for a, b, nm, e in zip(gs, gr, names, _graderrs(gs, gr)):
        assert a.shape == b.shape, nm
        assert e < 1e-5, (nm, e)


def test_the_function_makes_one_gemm_of_each_kind(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    seen = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(transformer_ops_stub, name)
            if not name.startswith(("gemm_", "tconv_")):
                return fn

            def wrapped(*a, **k):
                seen.append(name)
                return fn(*a, **k)
            return wrapped

    monkeypatch.setattr(nn_ops, "ops", Counting())
    ei, n = meshes["grid"]
    g = transformer_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    p = tuple(None if q is None else q.detach().float().requires_grad_(True) for q in _params(6, 4, 2, True, False, True, 5))
    x = torch.randn(n, 6, requires_grad=True)
    y = nn_ops._TransformerConvFn.apply(x, *p[:8], g, 2, True, False)
    y.sum().backward()
    assert seen == ["gemm_nt", "tconv_fwd", "tconv_bwd_edge", "tconv_bwd_node", "gemm_tn", "gemm_nn"]


def test_parameter_names_shapes_and_init():
    from dual_dmp_amd.nn_ops import TransformerConv
    torch.manual_seed(0)
    conv = TransformerConv(40, 24, heads=3, beta=True)
    sd = conv.state_dict()
    assert sorted(sd) == sorted(["lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight",
                                 "lin_value.bias", "lin_skip.weight", "lin_skip.bias", "lin_beta.weight"])
    for k in ("lin_key", "lin_query", "lin_value", "lin_skip"):
        assert sd[k + ".weight"].shape == (72, 40) and sd[k + ".bias"].shape == (72,)
    assert sd["lin_beta.weight"].shape == (1, 216)
    a, b = 1.0 / math.sqrt(40), 1.0 / math.sqrt(216)
    for k, v in sd.items():
        lim = b if k.startswith("lin_beta") else a
        assert v.abs().max() <= lim and v.abs().max() > 0.8 * lim, k
    assert abs(float(sd["lin_key.weight"].mean())) < 0.1 * a
    assert not torch.equal(sd["lin_key.weight"], sd["lin_query.weight"])
    assert conv.lin_edge is None and conv.beta
    mean = TransformerConv(40, 24, heads=3, concat=False, beta=True)
    assert mean.lin_skip.weight.shape == (24, 40) and mean.lin_beta.weight.shape == (1, 72) and mean.lin_key.weight.shape == (72, 40)
    plain = TransformerConv(40, 24, heads=3)
    assert plain.lin_beta is None and plain.lin_edge is None and "lin_beta.weight" not in plain.state_dict()
    nob = TransformerConv(40, 24, bias=False)
    assert nob.lin_skip.bias is None and nob.lin_key.bias is not None and nob.lin_query.bias is not None and nob.lin_value.bias is not None
    noroot = TransformerConv(40, 24, heads=2, root_weight=False, beta=True)
    assert noroot.lin_skip.weight.shape == (48, 40) and noroot.lin_beta is None and not noroot.beta
    conv2 = TransformerConv(40, 24, heads=3, beta=True)
    conv2.load_state_dict(sd)
    assert torch.equal(conv2.lin_value.weight, sd["lin_value.weight"])
    ref = TransformerConvRef(40, 24, heads=3, beta=True, dtype=torch.float32).load_from(conv)
    assert sorted(ref.state_dict()) == sorted(sd) and torch.equal(ref.lin_skip.bias, conv.lin_skip.bias)
    assert "heads=3" in repr(conv)
    before = conv.lin_value.weight.detach().clone()
    conv.reset_parameters()
    assert not torch.equal(conv.lin_value.weight, before) and conv.lin_value.weight.abs().max() <= a


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import TransformerConv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    with pytest.raises(ValueError):
        TransformerConv((4, 4), 8)
    with pytest.raises(ValueError):
        TransformerConv(4, 8, edge_dim=2)
    for heads in (0, -1, 1.5):
        with pytest.raises(ValueError, match="heads"):
            TransformerConv(4, 8, heads=heads)
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    conv = TransformerConv(4, 8, heads=2)
    with pytest.raises(ValueError):
        conv((x, x), ei)
    for kw in (dict(edge_attr=torch.randn(2, 3)), dict(return_attention_weights=True)):
        with pytest.raises(ValueError):
            conv(x, ei, **kw)
    drop = TransformerConv(4, 8, dropout=0.5)
    with pytest.raises(ValueError, match="dropout"):
        drop(x, ei)
    with pytest.raises(ValueError, match="bf16"):
        conv(x.to(torch.bfloat16), ei)
    for bad in (torch.randn(6, 5), torch.randn(6), torch.randn(2, 6, 4)):
        with pytest.raises(ValueError, match="shape"):
            conv(bad, ei)
    with pytest.raises(ValueError, match="no CPU fallback"):
        conv(x, ei)                                              # a CPU x
    with pytest.raises(ValueError, match="no CPU fallback"):
        drop.eval()(x, ei)                                       # dropout in eval mode is the identity: only the CPU x is refused


def test_modular_nets_take_conv_transformer():
    from dual_dmp_amd.engine import NORM_WIDTHS, POS_WIDTHS
    from dual_dmp_amd.networks import NormalNet, PosNet
    from dual_dmp_amd.nn_ops import TransformerConv
    for mk, widths in ((PosNet, POS_WIDTHS), (NormalNet, NORM_WIDTHS)):
        net = mk(torch.device("cpu"), fused=False, conv="transformer", heads=4)
        convs = [getattr(net, "conv%d" % i) for i in range(1, 13)]
        assert all(isinstance(c, TransformerConv) and c.concat and c.root_weight and not c.beta for c in convs)
        assert [(c.in_channels, c.out_channels * c.heads, c.heads) for c in convs] == [(widths[i], widths[i + 1], 4) for i in range(12)]
        sd = net.state_dict()
        for i in (1, 12):
            for leaf in ("lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_value.bias", "lin_skip.weight", "lin_skip.bias"):
                assert "conv%d.%s" % (i, leaf) in sd
        assert len([k for k in sd if k.startswith("conv")]) == 12 * 8
        assert net.conv3.lin_skip.weight.shape == (widths[3], widths[2])
        with pytest.raises(ValueError):
            mk(torch.device("cpu"), fused=True, conv="transformer", heads=4)
        with pytest.raises(ValueError, match="divisible"):
            mk(torch.device("cpu"), fused=False, conv="transformer", heads=3)      # 32 is not divisible by 3
        for bad in ("gatv2", "sage"):
            with pytest.raises(ValueError) as info:
                mk(torch.device("cpu"), fused=False, conv=bad)
            assert "feast" in str(info.value) and "transformer" in str(info.value)


def test_the_new_entry_points_are_declared():
    from dual_dmp_amd import _lib, ops
    protos = _lib.parse_header()
    want = {"ddmp_tconv_fwd_f32": 16, "ddmp_tconv_bwd_edge_f32": 15, "ddmp_tconv_bwd_node_f32": 17}
    for name, nargs in want.items():
        assert name in protos and len(protos[name][1]) == nargs and protos[name][0] == "int", name
    assert "#define DDMP_ABI_VERSION 3" in " ".join(open(_lib.HEADER).read().split())
    for name in ("tconv_fwd", "tconv_bwd_edge", "tconv_bwd_node"):
        assert callable(getattr(ops, name))
    from dual_dmp_amd.nn_ops import TransformerConv, _TransformerConvFn  # noqa: F401

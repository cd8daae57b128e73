"""GATv2Conv: everything that can be checked without a GPU -- the two float64 references against each other, the host side of
``nn_ops._GATv2ConvFn`` over torch restatements of the kernels (tests/gatv2_ops_stub.py), parameter names / shapes /
initialisation, the refusals, the forced branch decisions of the reference and the declarations of the new entry points."""
import math

import pytest
import torch

import gatv2_ops_stub
from gatv2_ref import GATv2ConvRef, dense_gatv2, gatv2_edge_list
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


def _params(cin, cout, heads, concat, seed, share=False, lin_bias=True, bias=True, dtype=torch.float64):
    """-> (wl, bl, wr, br, att, bias); None where the configuration has none."""
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=gen, dtype=torch.float64) * 0.5).to(dtype).requires_grad_(True)
    hc = heads * cout
    wl, bl = mk(hc, cin), mk(hc) if lin_bias else None
    wr, br = (None, None) if share else (mk(hc, cin), mk(hc) if lin_bias else None)
    return wl, bl, wr, br, mk(1, heads, cout), mk(hc if concat else cout) if bias else None


def _grads(y, t, leaves):
    leaves = [p for p in leaves if p is not None]
    return torch.autograd.grad((y * t).sum(), leaves)


@pytest.mark.parametrize("name", ["ico", "grid"])
@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("concat", [True, False])
def test_the_two_references_agree_in_float64(meshes, name, loops, heads, concat):
    ei, n = meshes[name]
    gen = torch.Generator().manual_seed(n + heads)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    for share in (False, True):
        p = _params(5, 4, heads, concat, 3, share=share)
        t = torch.randn(n, heads * 4 if concat else 4, generator=gen, dtype=torch.float64)
        outs, grads = [], []
        for fn in (gatv2_edge_list, dense_gatv2):
            y = fn(x, ei, *p, heads, concat, 0.2, loops)
            outs.append(y)
            grads.append(_grads(y, t, (x,) + p))
        assert relerr(outs[0], outs[1]) < 1e-13
        for a, b in zip(*grads):
            assert relerr(a, b) < 1e-12


CASES = [(3, 3, 2), (16, 4, 8), (5, 6, 3), (8, 8, 1)]           # ragged in / total widths go through the packing's padding
NAMES = ("dx", "dW_l", "db_l", "dW_r", "db_r", "datt", "db")


@pytest.mark.parametrize("cin,cout,heads", CASES)
@pytest.mark.parametrize("concat,loops", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("share,lin_bias", [(False, True), (True, True), (False, False), (True, False)])
def test_gatv2conv_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, cin, cout, heads, concat, loops, share, lin_bias):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", gatv2_ops_stub)
    ei, n = meshes["ico"]
    gen = torch.Generator().manual_seed(cin * 7 + heads)
    x64 = torch.randn(n, cin, generator=gen, dtype=torch.float64)
    p64 = _params(cin, cout, heads, concat, 11, share=share, lin_bias=lin_bias, bias=lin_bias)
    t = torch.randn(n, heads * cout if concat else cout, generator=gen, dtype=torch.float64)
    xr = x64.clone().requires_grad_(True)
    yr = gatv2_edge_list(xr, ei, *p64, heads, concat, 0.2, loops)
    gr = _grads(yr, t, (xr,) + p64)
    x = x64.float().requires_grad_(True)
    p = tuple(None if q is None else q.detach().float().requires_grad_(True) for q in p64)
    g = gatv2_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=loops)
    del gatv2_ops_stub.calls[:]
    y = nn_ops._GATv2ConvFn.apply(x, *p, g, heads, concat, 0.2)
    gs = _grads(y, t.float(), (x,) + p)
    assert gatv2_ops_stub.calls == ["gatv2_fwd", "gatv2_bwd_edge", "gatv2_bwd_node", "gatv2_datt"]
    assert y.shape == yr.shape and relerr(y, yr) < 1e-5
    names = [nm for nm, q in zip(NAMES, (x,) + p) if q is not None]
    assert len(gs) == len(gr) == len(names)
    for a, b, nm in zip(gs, gr, names):
        assert a.shape == b.shape, nm
        assert relerr(a, b) < 1e-5, (nm, relerr(a, b))


def test_backward_skips_what_is_not_asked_for(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", gatv2_ops_stub)
    ei, n = meshes["grid"]
    g = gatv2_ops_stub.graph_for(ei, n, norm="gat")
    wl, bl, wr, br, att, bias = (q.detach().float() for q in _params(4, 4, 2, True, 5))
    x = torch.randn(n, 4, requires_grad=True)
    del gatv2_ops_stub.calls[:]
    y = nn_ops._GATv2ConvFn.apply(x, wl, bl, wr, br, att, bias, g, 2, True, 0.2)
    y.sum().backward()
    assert gatv2_ops_stub.calls == ["gatv2_fwd", "gatv2_bwd_edge", "gatv2_bwd_node"] and x.grad is not None


def test_forced_branch_decisions_replace_the_references_own(meshes):
    """``pos`` equal to the reference's own decisions changes nothing; flipped decisions change the output as the formula says."""
    ei, n = meshes["grid"]
    ref = GATv2ConvRef(4, 3, heads=2)
    x = torch.randn(n, 4, dtype=torch.float64)
    y0, aux = ref(x, ei, full=True)
    y1 = ref(x, ei, pos=aux["own"])
    assert torch.equal(y0, y1)
    y2, aux2 = ref(x, ei, full=True, pos=~aux["own"])
    lu = torch.where(~aux["own"], aux["u"], 0.2 * aux["u"])
    assert torch.allclose(aux2["z"], (lu * ref.att).sum(-1)) and not torch.allclose(y0, y2)


def test_parameter_names_shapes_and_init():
    from dual_dmp_amd.nn_ops import GATv2Conv
    torch.manual_seed(0)
    conv = GATv2Conv(40, 24, heads=3)
    assert conv.lin_l is not conv.lin_r
    sd = conv.state_dict()
    assert sorted(sd) == sorted(["lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias"])
    assert sd["lin_l.weight"].shape == (72, 40) and sd["lin_r.weight"].shape == (72, 40) and sd["att"].shape == (1, 3, 24)
    assert sd["lin_l.bias"].shape == (72,) and sd["lin_r.bias"].shape == (72,)
    assert sd["bias"].shape == (72,) and not sd["bias"].any()
    a, b, c = math.sqrt(6.0 / (40 + 72)), math.sqrt(6.0 / (3 + 24)), 1.0 / math.sqrt(40)
    for w in (sd["lin_l.weight"], sd["lin_r.weight"]):
        assert w.abs().max() <= a and w.abs().max() > 0.9 * a and abs(float(w.mean())) < 0.1 * a
    assert not torch.equal(sd["lin_l.weight"], sd["lin_r.weight"])
    for t in (sd["lin_l.bias"], sd["lin_r.bias"]):
        assert t.abs().max() <= c and t.abs().max() > 0.8 * c
    assert sd["att"].abs().max() <= b and sd["att"].abs().max() > 0.8 * b
    assert GATv2Conv(40, 24, heads=3, concat=False).bias.shape == (24,)
    nob = GATv2Conv(40, 24, bias=False)
    assert nob.bias is None and nob.lin_l.bias is None and nob.lin_r.bias is None
    shared = GATv2Conv(40, 24, heads=3, share_weights=True)
    assert shared.lin_l is shared.lin_r
    assert sorted(shared.state_dict()) == sorted(sd)
    assert [nm for nm, _ in shared.named_parameters()] == ["att", "bias", "lin_l.weight", "lin_l.bias"]
    conv2 = GATv2Conv(40, 24, heads=3)
    conv2.load_state_dict(sd)
    assert torch.equal(conv2.lin_r.weight, sd["lin_r.weight"])
    ref = GATv2ConvRef(40, 24, heads=3, dtype=torch.float32).load_from(conv)
    assert sorted(ref.state_dict()) == sorted(sd) and torch.equal(ref.lin_r.bias, conv.lin_r.bias)


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import GATv2Conv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    with pytest.raises(ValueError):
        GATv2Conv((4, 4), 8)
    with pytest.raises(ValueError):
        GATv2Conv(4, 8, edge_dim=2)
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    conv = GATv2Conv(4, 8, heads=2)
    with pytest.raises(ValueError):
        conv((x, x), ei)
    for kw in (dict(edge_attr=torch.randn(2, 3)), dict(size=(6, 6)), dict(return_attention_weights=True)):
        with pytest.raises(ValueError):
            conv(x, ei, **kw)
    drop = GATv2Conv(4, 8, dropout=0.5)
    with pytest.raises(ValueError, match="dropout"):
        drop(x, ei)
    with pytest.raises(ValueError, match="bf16"):
        conv(x.to(torch.bfloat16), ei)
    with pytest.raises(ValueError, match="no CPU fallback"):
        conv(x, ei)                                              # a CPU x
    with pytest.raises(ValueError, match="no CPU fallback"):
        drop.eval()(x, ei)                                       # dropout in eval mode is the identity: only the CPU x is refused


def test_the_new_entry_points_are_declared():
    from dual_dmp_amd import _lib, ops
    protos = _lib.parse_header()
    want = {"ddmp_gatv2_fwd_f32": 14, "ddmp_gatv2_bwd_edge_f32": 18, "ddmp_gatv2_bwd_node_f32": 16,
            "ddmp_gatv2_datt_workspace_bytes": 3, "ddmp_gatv2_datt_f32": 9}
    for name, nargs in want.items():
        assert name in protos and len(protos[name][1]) == nargs, name
    assert protos["ddmp_gatv2_datt_workspace_bytes"][0] == "size_t"
    assert "#define DDMP_ABI_VERSION 3" in " ".join(open(_lib.HEADER).read().split())
    for name in ("gatv2_fwd", "gatv2_bwd_edge", "gatv2_bwd_node", "gatv2_datt"):
        assert callable(getattr(ops, name))
    from dual_dmp_amd.nn_ops import GATv2Conv, _GATv2ConvFn  # noqa: F401

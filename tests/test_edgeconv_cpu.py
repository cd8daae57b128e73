"""EdgeConv: everything that can be checked without a GPU -- the two float64 references against each other, the host side of
``nn_ops._EdgeConvFn`` over torch restatements of the kernels (tests/edgeconv_ops_stub.py), the activations behind the Linear,
the tie rule, the edgeless node, parameter names, the refusals, and the modular nets' ``conv="edge"``."""
import pytest
import torch
import torch.nn as nn

import edgeconv_ops_stub as stub
from edgeconv_ref import EdgeConvRef, as_dtype, dense_edgeconv, edgeconv_edge_list


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _with_extras(ei):
    """Duplicates and explicit loops (two on node 5) on top of a mesh, as test_feast_cpu.py adds them."""
    extra = torch.tensor([[3, 9, 5, 5, 40], [9, 3, 5, 5, 40]])
    dup = ei[:, :50]
    return torch.cat([ei, extra, dup, dup[[1, 0]]], 1).contiguous()


@pytest.fixture(scope="module")
def meshes():
    """name -> (edge_index, n): n counts one more node than the mesh has -- the last node has no edge at all."""
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    for name, (v, f) in (("ico", synth.icosphere(2)), ("grid", synth.open_grid(9, 7))):
        e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
        out[name] = (_with_extras(torch.cat([e, e[[1, 0]]], 1)), len(v) + 1)
    return out


def _linear(cin, cout, bias, seed, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    lin = nn.Linear(2 * cin, cout, bias=bias, dtype=dtype)
    with torch.no_grad():
        for p in lin.parameters():
            p.copy_((torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.5).to(dtype))
    return lin


def _grads(y, t, x, fn):
    return torch.autograd.grad((y * t).sum(), [x] + list(fn.parameters()))


@pytest.mark.parametrize("name", ["ico", "grid"])
@pytest.mark.parametrize("kind", ["linear", "nobias", "leaky"])
def test_the_two_references_agree_in_float64(meshes, name, kind):
    ei, n = meshes[name]
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    t = torch.randn(n, 4, generator=gen, dtype=torch.float64)
    lin = _linear(5, 4, kind != "nobias", 3)
    fn = nn.Sequential(lin, nn.LeakyReLU(0.2)) if kind == "leaky" else lin
    outs, grads = [], []
    for form in (edgeconv_edge_list, dense_edgeconv):
        y = form(x, ei, fn)
        outs.append(y)
        grads.append(_grads(y, t, x, fn))
    assert outs[0].shape == (n, 4) and relerr(outs[0], outs[1]) <= 1e-12
    assert bool((outs[0][n - 1] == 0).all()) and bool((outs[1][n - 1] == 0).all())       # the edgeless node
    for a, b in zip(*grads):
        assert relerr(a, b) <= 1e-12, relerr(a, b)


CASES = [(3, 3), (16, 4), (5, 6), (8, 8)]                       # ragged in / out widths go through the padding


def _fn_run(monkeypatch, ei, n, fn64, cin, cout, seed, through_module=False):
    """(got, reference): [y, dx, dW, (db)] of the product's host code over the stub in float32 and of the edge-list reference in
    float64, on the same inputs."""
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    gen = torch.Generator().manual_seed(seed)
    x64 = torch.randn(n, cin, generator=gen, dtype=torch.float64)
    t = torch.randn(n, cout, generator=gen, dtype=torch.float64)
    xr = x64.clone().requires_grad_(True)
    yr = edgeconv_edge_list(xr, ei, fn64)
    ref = [yr] + list(_grads(yr, t, xr, fn64))
    fn = as_dtype(fn64, torch.float32)
    x = x64.float().requires_grad_(True)
    g = stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    del stub.calls[:], stub.want_args[:]
    if through_module:
        y = nn_ops.EdgeConv(fn)._core(x, ei)
    else:
        y = nn_ops._edge_conv(x, fn.weight, fn.bias, g)
    got = [y] + list(_grads(y, t.float(), x, fn))
    return got, ref


@pytest.mark.parametrize("cin,cout", CASES)
@pytest.mark.parametrize("bias", [True, False])
def test_edgeconv_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, cin, cout, bias):
    ei, n = meshes["ico"]
    got, ref = _fn_run(monkeypatch, ei, n, _linear(cin, cout, bias, 11), cin, cout, cin * 7 + cout)
    assert stub.calls == ["gather_max", "gather_max_bwd"] and stub.want_args == [True]
    assert len(got) == len(ref) == (4 if bias else 3)
    for a, b, nm in zip(got, ref, ("y", "dx", "dW", "db")):
        assert a.shape == b.shape and a.dtype == torch.float32, nm
        assert relerr(a, b) <= 1e-5, (nm, relerr(a, b))


def test_no_grad_forward_asks_for_no_arg(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    ei, n = meshes["grid"]
    lin = _linear(5, 6, True, 2, torch.float32)
    x = torch.randn(n, 5)
    g = stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    del stub.calls[:], stub.want_args[:]
    with torch.no_grad():
        y0 = nn_ops._edge_conv(x, lin.weight, lin.bias, g)
    y1 = nn_ops._edge_conv(x, lin.weight, lin.bias, g)
    frozen = as_dtype(lin, torch.float32).requires_grad_(False)
    y2 = nn_ops._edge_conv(x, frozen.weight, frozen.bias, g)     # nothing requires a gradient
    y3 = nn_ops._edge_conv(x.clone().requires_grad_(True), frozen.weight, frozen.bias, g)
    assert stub.calls == ["gather_max"] * 4 and stub.want_args == [False, True, False, True]
    assert not y0.requires_grad and y1.requires_grad and not y2.requires_grad and y3.requires_grad
    assert torch.equal(y0, y1) and torch.equal(y0, y2) and torch.equal(y0, y3)


@pytest.mark.parametrize("act", ["leaky", "relu", "identity+leaky"])
def test_activations_behind_the_linear_equal_the_per_edge_reference(meshes, monkeypatch, act):
    ei, n = meshes["grid"]
    tail = {"leaky": [nn.LeakyReLU(0.2)], "relu": [nn.ReLU()], "identity+leaky": [nn.Identity(), nn.LeakyReLU(0.01)]}[act]
    fn64 = nn.Sequential(_linear(5, 6, True, 4), *tail)
    got, ref = _fn_run(monkeypatch, ei, n, fn64, 5, 6, 21, through_module=True)
    assert stub.calls == ["graph_for", "gather_max", "gather_max_bwd"]
    for a, b, nm in zip(got, ref, ("y", "dx", "dW", "db")):
        assert a.shape == b.shape, nm
        assert relerr(a, b) <= 1e-5, (nm, relerr(a, b))


def test_ties_go_to_the_smallest_source_id(meshes):
    """All rows of x equal: every entry of a row ties.  y = A + B, the whole of dG[i] lands on row i's smallest neighbour id."""
    ei, n = meshes["ico"]
    g = stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    gen = torch.Generator().manual_seed(1)
    C = 6
    a = torch.randn(n, C, generator=gen)
    b = torch.randn(1, C, generator=gen).expand(n, C).contiguous()
    dg = torch.randn(n, C, generator=gen)
    y, arg = stub.gather_max(g, b, a=a)
    nonempty = g.rowptr[1:] > g.rowptr[:-1]
    assert int(nonempty.sum()) == n - 1
    first = g.col[g.rowptr[:-1].clamp(max=g.nnz - 1)]            # CSR columns ascend: a row's first entry is its smallest id
    assert torch.equal(y[nonempty], (a + b)[nonempty])
    assert torch.equal(arg[nonempty].long(), first[nonempty].view(-1, 1).expand(-1, C))
    da, db = stub.gather_max_bwd(g, dg, arg)
    assert torch.allclose(db.double().sum(0), dg[nonempty].double().sum(0), atol=1e-5)
    want = torch.zeros((n, C), dtype=torch.float64).index_add_(0, first[nonempty], dg[nonempty].double())
    assert relerr(db, want) <= 1e-6
    assert torch.equal(da[nonempty], dg[nonempty])


def test_the_edgeless_node_gets_zero_and_gives_nothing(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    ei, n = meshes["ico"]
    lin = _linear(5, 8, True, 6, torch.float32)                  # out = 8: the bias gradient goes through colsum
    with torch.no_grad():
        lin.bias.add_(3.0)                                       # an edgeless node must NOT show the bias
    x = torch.randn(n, 5, requires_grad=True)
    g = stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    y = nn_ops._edge_conv(x, lin.weight, lin.bias, g)
    assert bool((y[n - 1] == 0).all()) and float(y.detach()[:n - 1].abs().min()) > 0
    dy = torch.randn(n, 8)
    dy[n - 1] = 1000.0
    dx, dw, db = torch.autograd.grad(y, [x, lin.weight, lin.bias], dy)
    assert bool((dx[n - 1] == 0).all())
    assert relerr(db, dy[:n - 1].double().sum(0)) <= 1e-6
    y2, arg = stub.gather_max(g, torch.randn(n, 8), a=torch.ones(n, 8))
    assert bool((y2[n - 1] == 0).all()) and bool((arg[n - 1] == -1).all())
    da, dbb = stub.gather_max_bwd(g, dy, arg)
    assert bool((da[n - 1] == 0).all()) and bool((dbb[n - 1] == 0).all())


def test_state_dict_keys_and_kept_module():
    from dual_dmp_amd.nn_ops import EdgeConv
    lin = nn.Linear(10, 7)
    conv = EdgeConv(lin)
    assert conv.nn is lin and (conv.in_channels, conv.out_channels, conv.aggr) == (5, 7, "max")
    assert list(conv.state_dict()) == ["nn.weight", "nn.bias"]
    assert [p for p in conv.parameters()][0] is lin.weight
    assert list(EdgeConv(nn.Linear(10, 7, bias=False)).state_dict()) == ["nn.weight"]
    seq = nn.Sequential(nn.Linear(6, 4), nn.LeakyReLU(0.2), nn.Identity(), nn.ReLU())
    conv = EdgeConv(seq, aggr="max")
    assert conv.nn is seq and list(conv.state_dict()) == ["nn.0.weight", "nn.0.bias"]
    ref = EdgeConvRef(seq)
    assert list(ref.state_dict()) == list(conv.state_dict())
    assert [tuple(v.shape) for v in ref.state_dict().values()] == [tuple(v.shape) for v in conv.state_dict().values()]


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import EdgeConv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    mlp = nn.Sequential(nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 8))
    for bad in (mlp, nn.Sequential(nn.Linear(8, 8), nn.Sigmoid()), nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8)),
                nn.Sequential(nn.ReLU(), nn.Linear(8, 8)), nn.Sequential(nn.Linear(8, 8), nn.LeakyReLU(-0.1)),
                nn.Sequential(nn.Linear(8, 8), nn.Tanh()), nn.Sequential(), nn.ReLU(), nn.Linear(7, 8), nn.Bilinear(4, 4, 8),
                nn.Sequential(nn.Linear(7, 8), nn.ReLU()), None, lambda z: z):
        with pytest.raises(ValueError):
            EdgeConv(bad)
    for aggr in ("add", "mean", "sum", "min"):
        with pytest.raises(ValueError):
            EdgeConv(nn.Linear(8, 8), aggr=aggr)
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    conv = EdgeConv(nn.Linear(8, 8))
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
    conv.nn = mlp                                                # edited after construction: refused at the call
    with pytest.raises(ValueError):
        conv(torch.randn(6, 4), ei)


def test_a_non_symmetric_structure_is_refused_by_the_graph(monkeypatch):
    """The backward reads row j's own entries as the rows j feeds: the valued graph refuses a one-directional edge."""
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    conv = nn_ops.EdgeConv(nn.Linear(8, 8))
    del stub.calls[:]
    with pytest.raises(ValueError):
        conv._core(torch.randn(3, 4), torch.tensor([[0, 1, 2], [1, 0, 0]]))
    assert stub.calls == ["graph_for"]


def test_modular_nets_take_conv_edge():
    from dual_dmp_amd.networks import NormalNet, PosNet
    from dual_dmp_amd.nn_ops import EdgeConv
    from dual_dmp_amd.engine import NORM_WIDTHS, POS_WIDTHS
    for mk, widths in ((PosNet, POS_WIDTHS), (NormalNet, NORM_WIDTHS)):
        net = mk(torch.device("cpu"), fused=False, conv="edge")
        convs = [getattr(net, "conv%d" % i) for i in range(1, 13)]
        assert all(isinstance(c, EdgeConv) and type(c.nn) is nn.Linear for c in convs)
        assert [(c.in_channels, c.out_channels) for c in convs] == [(widths[i], widths[i + 1]) for i in range(12)]
        names = [k for k, _ in net.named_parameters()]
        for i in (1, 12):
            for leaf in ("nn.weight", "nn.bias"):
                assert "conv%d.%s" % (i, leaf) in names
        assert len([k for k in names if k.startswith("conv")]) == 12 * 2
        assert net.conv3.nn.weight.shape == (widths[3], 2 * widths[2])
        with pytest.raises(ValueError):
            mk(torch.device("cpu"), fused=True, conv="edge")
        for bad in ("sage", "edgeconv", "EDGE", "dynamic_edge"):
            with pytest.raises(ValueError) as info:
                mk(torch.device("cpu"), fused=False, conv=bad)
            assert "'edge'" in str(info.value)

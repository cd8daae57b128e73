"""GENConv: everything that can be checked without a GPU -- the two float64 references against each other, a graph done by hand, the
limits t = 0 (mean) and t -> inf (max) of the reference, the host side of ``nn_ops._GENConvFn`` / ``_LinearFn`` over torch
restatements of the kernels (tests/gen_ops_stub.py) with its call sequence, parameter names / shapes / initialisation, the refusals,
the modular nets' ``conv="gen"`` and the two declared entry points."""
import os
import re

import pytest
import torch

import gen_ops_stub as stub
from gen_ref import GENConvRef, message, softmax_aggr_dense, softmax_aggr_edge_list
from test_gat_cpu import _with_extras

HOST_TOL = 1e-5
DIMS = [(5, 5), (3, 6), (16, 8), (7, 4)]                         # (in, out)
MODES = {"plain": {}, "learn_t": dict(learn_t=True, t=0.7), "msg_norm": dict(msg_norm=True, learn_msg_scale=True),
         "layer": dict(norm="layer"), "nonorm": dict(norm=None), "bias": dict(bias=True), "three": dict(num_layers=3, t=-0.5)}


def err(a, b):
    """rel-L2 (the gradients that are zero in exact arithmetic have a rule of their own where they occur)."""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def meshes():
    """name -> (edge_index, n): the small icosphere and the open grid with duplicate edges and explicit loops on top
    (``_with_extras``), plus one node without any edge."""
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    for name, (v, f) in (("ico", synth.icosphere(2)), ("grid", synth.open_grid(9, 7))):
        e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
        out[name] = (_with_extras(torch.cat([e, e[[1, 0]]], 1)), len(v) + 1)
    return out


def _grads(mod, x, ei, t, call):
    x = x.clone().requires_grad_(True)
    y = call(mod, x, ei)
    named = [(k, p) for k, p in mod.named_parameters() if p.requires_grad]
    g = torch.autograd.grad((y * t).sum(), [x] + [p for _, p in named])
    return dict(zip(["y", "dx"] + [k for k, _ in named], [y.detach()] + list(g)))


def _inputs(n, cin, cout, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, cin, generator=gen, dtype=torch.float64), torch.randn(n, cout, generator=gen, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", ["ico", "grid"])
@pytest.mark.parametrize("cin,cout", [(5, 5), (3, 6)])
@pytest.mark.parametrize("mode", ["plain", "learn_t", "msg_norm", "layer", "nonorm"])
def test_the_two_references_agree_in_float64(meshes, name, cin, cout, mode):
    ei, n = meshes[name]
    torch.manual_seed(n + cin)
    ref = GENConvRef(cin, cout, **MODES[mode])
    x, t = _inputs(n, cin, cout, n)
    outs = []
    for form in ("edge", "dense"):
        ref.form = form
        outs.append(_grads(ref, x, ei, t, lambda m, x, ei: m(x, ei)))
    assert outs[0]["y"].shape == (n, cout) and ("aggr_module.t" in outs[0]) == (mode == "learn_t")
    for k in outs[0]:
        e = err(outs[0][k], outs[1][k])
        assert e < 1e-12, (k, e)


def test_a_graph_done_by_hand():
    """Two sources into node 0, one of them twice: agg_0 = (2 e^{t m_1} m_1 + e^{t m_3} m_3) / (2 e^{t m_1} + e^{t m_3}); node 2 has
    no edge: out_2 = mlp(x_2)."""
    ei = torch.tensor([[1, 1, 3, 0, 0, 0], [0, 0, 0, 1, 1, 3]])
    torch.manual_seed(0)
    ref = GENConvRef(4, 4, t=0.8, norm=None)
    x = torch.randn(4, 4, dtype=torch.float64)
    m = torch.relu(x) + 1e-7
    w1, w3 = 2 * torch.exp(0.8 * m[1]), torch.exp(0.8 * m[3])
    want0 = (w1 * m[1] + w3 * m[3]) / (w1 + w3) + x[0]
    for form in ("edge", "dense"):
        ref.form = form
        pre = ref.pre_mlp(x, ei)
        assert float((pre[0] - want0).abs().max()) <= 1e-14
        assert torch.equal(pre[2], x[2])                         # no edge: the aggregate is exactly 0
        assert float((pre[1] - (m[0] + x[1])).abs().max()) <= 1e-14          # one source (twice): its message itself
        assert float((ref(x, ei)[2] - ref.mlp(x[2:3])[0]).detach().abs().max()) <= 1e-14
    agg, lse = softmax_aggr_edge_list(m, ei, 4, 0.8, full=True)
    assert float((lse[0] - torch.log(w1 + w3)).abs().max()) <= 1e-14 and bool((lse[2] == 0).all())


@pytest.mark.parametrize("name", ["ico", "grid"])
def test_limits_of_the_reference_mean_at_0_and_max_at_200(meshes, name):
    """t = 0 is the mean of the messages over the edges.  t = 200: with M the row's maximum, gap the distance to its runner-up (the
    largest value below M), spread = M - min over the row's edges and k the number of edges below M: M - agg = sum_{below} p_e
    (M - m_e) and every such p_e <= e^{-200 (M - m_e)} <= e^{-200 gap} (the denominator is >= e^{200 M}), so
    |agg - M| <= k * spread * e^{-200 gap} -- all from the reference's own data.  (Without k the inequality is not a bound: the
    relu puts several edges of a row at the same runner-up value eps, and each of them has the runner-up's weight.)"""
    ei, n = meshes[name]
    x, _ = _inputs(n, 6, 6, 3)
    m = message(x, 1e-7)
    src, dst = ei
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(ei.shape[1], dtype=torch.float64))
    mean = torch.zeros(n, 6, dtype=torch.float64).index_add_(0, dst, m[src]) / deg.clamp(min=1).view(-1, 1)
    for aggr in (softmax_aggr_edge_list, softmax_aggr_dense):
        assert float((aggr(m, ei, n, 0.0) - mean).abs().max()) <= 1e-14
    idx = dst.view(-1, 1).expand(-1, 6)
    ninf = torch.full((n, 6), -float("inf"), dtype=torch.float64)
    mx = ninf.scatter_reduce(0, idx, m[src], "amax")
    mn = (-ninf).scatter_reduce(0, idx, m[src], "amin")
    below = torch.where(m[src] < mx[dst], m[src], torch.full((), -float("inf"), dtype=torch.float64))
    second = ninf.scatter_reduce(0, idx, below, "amax")          # -inf where the whole row sits at its maximum
    has = (deg > 0).view(-1, 1)
    k = torch.zeros((n, 6), dtype=torch.float64).index_add_(0, dst, (m[src] < mx[dst]).double())
    limit = torch.where(has, k * (mx - mn) * torch.exp(-200.0 * (mx - second)), torch.zeros((), dtype=torch.float64))
    agg = softmax_aggr_edge_list(m, ei, n, 200.0)
    diff = torch.where(has, (agg - mx).abs(), agg.abs())
    assert bool((diff <= limit + 4 * 2.0 ** -52 * m.abs().max()).all()), float((diff - limit).max())
    assert bool((agg[~has.view(-1)] == 0).all())


# ------------------------------------------------------------------------------------------------ the host side over the stub
def _guard_index_add(monkeypatch):
    """From here on ``index_add_`` / ``scatter*`` may only run inside the stub's functions (its stand-ins for a kernel's row loop):
    never in the product's host code.  (test_sage_cpu.py's trap.)"""
    inside = [0]
    for name in ("graph_for", "gather_softmax", "gather_softmax_bwd"):
        def wrapped(*a, _f=getattr(stub, name), **kw):
            inside[0] += 1
            try:
                return _f(*a, **kw)
            finally:
                inside[0] -= 1
        monkeypatch.setattr(stub, name, wrapped)
    for name in ("index_add_", "index_add", "scatter_", "scatter", "scatter_add_", "scatter_add", "scatter_reduce_", "scatter_reduce"):
        def guarded(*a, _f=getattr(torch.Tensor, name), _n=name, **kw):
            assert inside[0] > 0, "%s in the product's host code" % _n
            return _f(*a, **kw)
        monkeypatch.setattr(torch.Tensor, name, guarded)


def _host_run(monkeypatch, ei, n, cin, cout, mode, seed):
    """(got, reference): {y, dx, every trained parameter's gradient by name} of the product's host code over the stub and of the
    edge-list reference, both in float64 on the same inputs and parameters."""
    from dual_dmp_amd import nn_ops
    torch.manual_seed(seed)
    conv = nn_ops.GENConv(cin, cout, **MODES[mode]).double()
    ref = GENConvRef(cin, cout, **MODES[mode]).load_from(conv)
    x, t = _inputs(n, cin, cout, seed + 1)
    want = _grads(ref, x, ei, t, lambda m, x, ei: m(x, ei))
    monkeypatch.setattr(nn_ops, "ops", stub)
    _guard_index_add(monkeypatch)
    del stub.calls[:], stub.want_lses[:], stub.roots[:], stub.gemm_modes[:]
    got = _grads(conv, x, ei, t, lambda m, x, ei: m._core(x, ei))
    return got, want


@pytest.mark.parametrize("cin,cout", DIMS)
@pytest.mark.parametrize("mode", list(MODES))
def test_gen_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, cin, cout, mode):
    ei, n = meshes["ico"]
    got, want = _host_run(monkeypatch, ei, n, cin, cout, mode, cin * 7 + cout)
    assert stub.calls.count("gather_softmax") == 1 and stub.calls.count("gather_softmax_bwd") == 1
    assert stub.want_lses == [True]
    # the MLP's GEMMs run in the strict mode exactly where the scale of msg_norm is learnt: two Linears, forward and backward
    assert stub.gemm_modes == ([0] * 4 if mode == "msg_norm" else [])
    fused = mode != "msg_norm"
    assert stub.roots == [fused, ("add" if cin == cout else True) if fused else False]
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float64, k
        ref = want[k]
        if k in ("mlp.0.bias", "lin_dst.bias") and mode == "bias":
            # BatchNorm removes a constant (lin_dst.bias reaches it as one, through mlp.0): these gradients are zero in exact
            # arithmetic; their error is taken relative to their sibling's
            e = float((got[k] - ref).norm() / want["mlp.1.bias"].norm())
        else:
            e = err(got[k], ref)
        assert e <= HOST_TOL, (k, e)


@pytest.mark.parametrize("cin,cout", [(3, 6), (5, 5)])
def test_the_call_sequence(meshes, monkeypatch, cin, cout):
    """in != out: gemm_nt, gather_softmax | the MLP's two gemm_nt, its two (gemm_tn, gemm_nn) | gather_softmax_bwd, gemm_tn,
    gemm_nn.  in == out: the two gather calls are the whole graph part."""
    ei, n = meshes["ico"]
    mlp_fwd, mlp_bwd = ["gemm_nt"] * 2, ["gemm_tn", "gemm_nn"] * 2
    _host_run(monkeypatch, ei, n, cin, cout, "plain", 1)
    if cin != cout:
        assert stub.calls == ["graph_for", "gemm_nt", "gather_softmax"] + mlp_fwd + mlp_bwd + ["gather_softmax_bwd", "gemm_tn", "gemm_nn"]
        assert stub.calls[1:3] + stub.calls[-3:] == ["gemm_nt", "gather_softmax", "gather_softmax_bwd", "gemm_tn", "gemm_nn"]
    else:
        assert stub.calls == ["graph_for", "gather_softmax"] + mlp_fwd + mlp_bwd + ["gather_softmax_bwd"]


def test_no_grad_forward_stores_no_lse(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    ei, n = meshes["grid"]
    conv = nn_ops.GENConv(8, 8, norm=None)
    x = torch.randn(n, 8)
    del stub.calls[:], stub.want_lses[:]
    with torch.no_grad():
        y0 = conv._core(x, ei)
    y1 = conv._core(x.clone().requires_grad_(True), ei)
    assert stub.want_lses == [False, True]
    assert not y0.requires_grad and y1.requires_grad and torch.equal(y0, y1)
    assert "gather_softmax_bwd" not in stub.calls


# ------------------------------------------------------------------------------------------------ the module
def test_parameter_names_shapes_init_and_state_dict():
    from dual_dmp_amd.nn_ops import GENConv
    conv = GENConv(6, 8)
    assert list(conv.state_dict()) == ["lin_src.weight", "lin_dst.weight", "mlp.0.weight", "mlp.1.weight", "mlp.1.bias",
                                       "mlp.1.running_mean", "mlp.1.running_var", "mlp.1.num_batches_tracked", "mlp.4.weight"]
    assert [tuple(conv.state_dict()[k].shape) for k in ("lin_src.weight", "lin_dst.weight", "mlp.0.weight", "mlp.4.weight")] == \
        [(8, 6), (8, 6), (16, 8), (8, 16)]
    assert isinstance(conv.mlp[1], torch.nn.BatchNorm1d) and isinstance(conv.mlp[2], torch.nn.ReLU) and conv.mlp[3].p == 0.0
    # the float64 BatchNorm and the strict GEMMs belong to the one configuration with a learnt msg_norm.scale
    from dual_dmp_amd.nn_ops import _BatchNorm1d64
    for kw, on in ((dict(), False), (dict(msg_norm=True), False), (dict(learn_msg_scale=True), False),
                   (dict(msg_norm=True, learn_msg_scale=True), True)):
        c = GENConv(6, 8, **kw)
        assert type(c.mlp[1]) is (_BatchNorm1d64 if on else torch.nn.BatchNorm1d) and c.mlp[0].strict is on and c.mlp[4].strict is on
    assert list(GENConv(8, 8, norm=None).state_dict()) == ["mlp.0.weight", "mlp.3.weight"]
    full = GENConv(6, 8, learn_t=True, t=0.5, msg_norm=True, bias=True, norm="layer", num_layers=3, expansion=3)
    keys = list(full.state_dict())
    assert sorted(keys) == sorted(["aggr_module.t", "lin_src.weight", "lin_src.bias", "lin_dst.weight", "lin_dst.bias", "mlp.0.weight",
                                   "mlp.0.bias", "mlp.1.weight", "mlp.1.bias", "mlp.4.weight", "mlp.4.bias", "mlp.5.weight", "mlp.5.bias",
                                   "mlp.8.weight", "mlp.8.bias", "msg_norm.scale"])
    assert tuple(full.aggr_module.t.shape) == (1,) and float(full.aggr_module.t.detach()) == 0.5 and full.aggr_module.t.requires_grad
    assert tuple(full.msg_norm.scale.shape) == (1,) and float(full.msg_norm.scale.detach()) == 1.0 and not full.msg_norm.scale.requires_grad
    assert GENConv(4, 4, msg_norm=True, learn_msg_scale=True).msg_norm.scale.requires_grad
    assert isinstance(full.mlp[1], torch.nn.LayerNorm) and full.mlp[4].weight.shape == (24, 24) and full.mlp[8].weight.shape == (8, 24)
    assert isinstance(GENConv(4, 4).aggr_module.t, float) and "aggr_module.t" not in GENConv(4, 4).state_dict()
    ref = GENConvRef(6, 8, learn_t=True, t=0.5, msg_norm=True, bias=True, norm="layer", num_layers=3, expansion=3)
    assert sorted(ref.state_dict()) == sorted(keys)
    assert [tuple(ref.state_dict()[k].shape) for k in keys] == [tuple(full.state_dict()[k].shape) for k in keys]
    # a load_state_dict round trip
    other = GENConv(6, 8, learn_t=True, msg_norm=True, bias=True, norm="layer", num_layers=3, expansion=3)
    other.load_state_dict(full.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), full.state_dict().values()))
    torch.manual_seed(0)
    conv = GENConv(400, 900, bias=True)                          # uniform(+-1/sqrt(fan-in))
    for p, fan in ((conv.lin_src.weight, 400), (conv.lin_dst.weight, 400), (conv.lin_src.bias, 400), (conv.mlp[0].weight, 900),
                   (conv.mlp[4].weight, 1800), (conv.mlp[4].bias, 1800)):
        top = float(p.detach().abs().max())
        assert 0.9 * fan ** -0.5 < top <= fan ** -0.5


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import GENConv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    for kw in (dict(aggr="powermean"), dict(aggr="power"), dict(aggr="softmax_sg"), dict(aggr="mean"), dict(aggr=["softmax"]),
               dict(edge_dim=3), dict(learn_p=True), dict(norm="instance"), dict(norm="graph"), dict(num_layers=0), dict(num_layers=1.5),
               dict(t=float("inf")), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            GENConv(4, 8, **kw)
    with pytest.raises(ValueError):
        GENConv((4, 4), 8)
    with pytest.raises(TypeError):
        GENConv(4, 8, flow="target_to_source")
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    conv = GENConv(4, 8)
    with pytest.raises(ValueError):
        conv((x, x), ei)
    with pytest.raises(ValueError):
        conv(x, ei, edge_attr=torch.randn(2, 3))
    with pytest.raises(ValueError):
        conv(x, ei, size=(6, 6))
    with pytest.raises(ValueError):
        conv(x.to(torch.bfloat16), ei)
    with pytest.raises(ValueError):
        conv(torch.randn(6, 5), ei)
    with pytest.raises(ValueError):
        conv(x, ei)                                              # a CPU x: no CPU fallback
    with pytest.raises(ValueError):
        conv(x, torch.zeros((2, 0), dtype=torch.long))


def test_a_non_symmetric_structure_is_refused_by_the_graph(monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    conv = nn_ops.GENConv(4, 8)
    del stub.calls[:]
    with pytest.raises(ValueError):
        conv._core(torch.randn(3, 4), torch.tensor([[0, 1, 2], [1, 0, 0]]))
    assert stub.calls == ["graph_for"]


def test_ops_scalars_are_checked():
    from dual_dmp_amd import ops
    assert ops._smax_scalars("f", 1, None) == (1.0, 0, 0.0) and ops._smax_scalars("f", -0.7, 1e-7) == (-0.7, 1, 1e-7)
    for t, eps in ((float("nan"), None), (float("inf"), 0.0), (1.0, -1e-7), (1.0, float("inf"))):
        with pytest.raises(ops.DdmpError):
            ops._smax_scalars("f", t, eps)


def test_modular_nets_take_conv_gen():
    from dual_dmp_amd.engine import NORM_WIDTHS, POS_WIDTHS
    from dual_dmp_amd.networks import NormalNet, PosNet
    from dual_dmp_amd.nn_ops import GENConv
    for mk, widths in ((PosNet, POS_WIDTHS), (NormalNet, NORM_WIDTHS)):
        net = mk(torch.device("cpu"), fused=False, conv="gen")
        convs = [getattr(net, "conv%d" % i) for i in range(1, 13)]
        assert all(isinstance(c, GENConv) and isinstance(c.aggr_module.t, float) and c.aggr_module.t == 1.0 for c in convs)
        assert [(c.in_channels, c.out_channels) for c in convs] == [(widths[i], widths[i + 1]) for i in range(12)]
        sd = net.state_dict()
        for i, c in enumerate(convs, 1):
            assert ("conv%d.lin_src.weight" % i in sd) == (c.in_channels != c.out_channels)
            assert "conv%d.mlp.0.weight" % i in sd and "conv%d.mlp.4.weight" % i in sd and "conv%d.mlp.1.running_var" % i in sd
        with pytest.raises(ValueError):
            mk(torch.device("cpu"), fused=True, conv="gen")
        for bad in ("gatv2", "sage"):
            with pytest.raises(ValueError) as info:
                mk(torch.device("cpu"), fused=False, conv=bad)
            for name in ("gcn", "cheb", "gat", "feast", "edge", "gmm", "transformer", "resgated", "spline", "gen"):
                assert "'%s'" % name in str(info.value)


# ------------------------------------------------------------------------------------------------ the header
def test_header_declares_the_two_entry_points_and_abi_3():
    from dual_dmp_amd import _lib
    src = open(_lib.HEADER).read()
    assert re.search(r"#define\s+DDMP_ABI_VERSION\s+3\b", src)
    protos = _lib.parse_header()
    assert "ddmp_gather_softmax_f32" in protos and "ddmp_gather_softmax_bwd_f32" in protos
    names = [a for _, a in protos["ddmp_gather_softmax_f32"][1]]
    assert names == ["g", "H", "ldh", "C", "t", "has_eps", "msg_eps", "R", "ldr", "Y", "ldy", "lse", "ldl", "stream"]
    names = [a for _, a in protos["ddmp_gather_softmax_bwd_f32"][1]]
    assert names == ["g", "C", "dOut", "lddo", "H", "ldh", "Yp", "ldyp", "lse", "ldl", "t", "has_eps", "msg_eps", "add_dout", "dH", "lddh",
                     "dR", "lddr", "dt_rows", "stream"]
    assert os.path.exists(os.path.join(_lib.CSRC, "gsoftmax.hip"))

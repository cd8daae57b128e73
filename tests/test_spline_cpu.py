"""SplineConv: everything that can be checked without a GPU -- the two float64 references against each other, hand-checked basis
values, the host side of ``nn_ops._SplineConvFn`` over torch restatements of the kernels (tests/spline_ops_stub.py), parameter names
/ shapes / initialisation, the refusals, the modular nets' ``conv="spline"`` and the two declared entry points."""
import math

import pytest
import torch

import spline_ops_stub
from spline_ref import SplineConvRef, dense_spline, spline_basis, spline_edge_list


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _with_extras(ei):
    """Duplicates and explicit loops (two on node 5) on top of a mesh, as test_gmm_cpu.py adds them."""
    extra = torch.tensor([[3, 9, 5, 5, 40], [9, 3, 5, 5, 40]])
    dup = ei[:, :50]
    return torch.cat([ei, extra, dup, dup[[1, 0]]], 1).contiguous()


@pytest.fixture(scope="module")
def meshes():
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    for name, (v, f) in (("ico", synth.icosphere(1)), ("grid", synth.open_grid(9, 7))):
        e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
        out[name] = (_with_extras(torch.cat([e, e[[1, 0]]], 1)), len(v))
    return out


def _params(cin, cout, K, seed, root=True, bias=True, dtype=torch.float64):
    """(weight [K, in, out], lin.weight | None, bias | None), each requiring grad."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: (torch.randn(*s, generator=gen, dtype=torch.float64) * 0.5).to(dtype).requires_grad_(True)
    return rn(K, cin, cout), rn(cout, cin) if root else None, rn(cout) if bias else None


def _attr(E, dim, seed, dtype=torch.float64):
    """Pseudo-coordinates uniform in [0, 1]^dim, one draw per input edge (duplicates get different ones); the first rows sit exactly
    on 0, on 1 and on an interior knot of kernel_size 3 / 5."""
    a = torch.rand(E, dim, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    a[0], a[1], a[2], a[3] = 0.0, 1.0, 0.5, 0.25
    return a.to(dtype)


NAMES = ("dx", "dweight", "dlin", "db")
# (dim, kernel_size, is_open_spline)
SPLINES = [(1, 3, True), (2, (2, 3), (True, False)), (3, 2, True), (3, 3, False), (2, 1, True), (3, (4, 1, 2), (False, True, True))]


@pytest.mark.parametrize("name", ["ico", "grid"])
@pytest.mark.parametrize("dim,ks,op", SPLINES)
@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_the_two_references_agree_in_float64(meshes, name, dim, ks, op, aggr):
    ei, n = meshes[name]
    K = math.prod([ks] * dim if isinstance(ks, int) else ks)
    gen = torch.Generator().manual_seed(n + K)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    a = _attr(ei.shape[1], dim, 17)
    assert not torch.equal(a[:50], a[-100:-50])                  # the duplicated edges carry other pseudo-coordinates
    p = _params(5, 4, K, 3)
    t = torch.randn(n, 4, generator=gen, dtype=torch.float64)
    outs, grads = [], []
    for fn in (spline_edge_list, dense_spline):
        y = fn(x, ei, a, *p, ks, op, aggr)
        outs.append(y)
        grads.append(torch.autograd.grad((y * t).sum(), (x,) + p))
    assert relerr(outs[0], outs[1]) < 1e-13
    for u, v, nm in zip(*grads, NAMES):
        assert relerr(u, v) < 1e-12, (nm, relerr(u, v))


def test_hand_checked_basis_values():
    a = lambda *v: torch.tensor(v, dtype=torch.float64).view(-1, 1)
    # dim = 1, kernel_size = 3, open: v = 2 a
    b, k = spline_basis(a(0.25, 1.0, 0.0), 3, True)
    assert k.tolist() == [[0, 1], [2, 0], [0, 1]] and b.tolist() == [[0.5, 0.5], [1.0, 0.0], [1.0, 0.0]]
    # closed: v = 3 a; a = 0.5 -> 1.5 -> blocks (1, 2); a = 0.9 -> 2.7 -> blocks (2, 0): the seam wraps to block 0
    b, k = spline_basis(a(0.5, 0.9, 1.0), 3, False)
    assert k.tolist() == [[1, 2], [2, 0], [0, 1]]
    assert b[0].tolist() == [0.5, 0.5] and torch.allclose(b[1], torch.tensor([0.3, 0.7], dtype=torch.float64), atol=1e-12)
    assert b[2].tolist() == [1.0, 0.0]                           # a = 1 on the closed spline is a = 0
    # dim = 2, kernel_size (3, 4), open: the FIRST coordinate varies fastest -- block = i_0 + 3 i_1
    b, k = spline_basis(torch.tensor([[0.75, 0.5]], dtype=torch.float64), (3, 4), True)       # v = (1.5, 1.5)
    assert k.tolist() == [[1 + 3 * 1, 2 + 3 * 1, 1 + 3 * 2, 2 + 3 * 2]] and b.tolist() == [[0.25] * 4]
    b, k = spline_basis(torch.tensor([[0.0, 1.0]], dtype=torch.float64), (3, 4), True)        # v = (0, 3)
    assert k.tolist() == [[0 + 3 * 3, 1 + 3 * 3, 0, 1]] and b.tolist() == [[1.0, 0.0, 0.0, 0.0]]
    # kernel_size 1: every corner is block 0
    b, k = spline_basis(torch.tensor([[0.3, 0.6]], dtype=torch.float64), 1, True)
    assert k.tolist() == [[0, 0, 0, 0]] and b.tolist() == [[1.0, 0.0, 0.0, 0.0]]
    _, k = spline_basis(torch.tensor([[0.3, 0.6]], dtype=torch.float64), 1, False)
    assert k.tolist() == [[0, 0, 0, 0]]


@pytest.mark.parametrize("dim,ks,op", SPLINES + [(5, 2, True), (4, (2, 3, 1, 2), (True, False, False, True))])
def test_the_weights_of_every_edge_sum_to_one_and_the_stub_basis_is_the_reference_basis(dim, ks, op):
    a = _attr(500, dim, dim)
    b, k = spline_basis(a, ks, op)
    kl = [ks] * dim if isinstance(ks, int) else list(ks)
    assert b.shape == k.shape == (500, 1 << dim)
    assert bool((b >= 0).all()) and torch.allclose(b.sum(1), torch.ones(500, dtype=torch.float64), atol=1e-14)
    assert int(k.min()) >= 0 and int(k.max()) < math.prod(kl)
    bs, kk = spline_ops_stub._basis(a.float(), kl, [op] * dim if isinstance(op, bool) else list(op))
    b32, k32 = spline_basis(a.float().double(), ks, op)
    # (the stub rounds v to float32 as the kernels do: compare the mixed blocks, which are continuous across a knot)
    tab = torch.randn(math.prod(kl), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert torch.allclose((bs * tab[kk]).sum(1), (b32 * tab[k32]).sum(1), atol=1e-5)


CASES = [(3, 3, 1, 3, True), (16, 4, 2, (2, 3), (True, False)), (5, 6, 3, 2, True), (8, 8, 2, 1, True), (4, 5, 3, 3, False)]


@pytest.mark.parametrize("cin,cout,dim,ks,op", CASES)       # (in, out, dim, kernel_size, open): ragged widths go through the padding
@pytest.mark.parametrize("root", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_splineconv_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, cin, cout, dim, ks, op, root, bias, aggr):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", spline_ops_stub)
    ei, n = meshes["ico"]
    kl, ol = nn_ops._spline_sizes(dim, ks, op)
    K = math.prod(kl)
    gen = torch.Generator().manual_seed(cin * 7 + K)
    x64 = torch.randn(n, cin, generator=gen, dtype=torch.float64)
    a32 = _attr(ei.shape[1], dim, 23).float()
    p64 = _params(cin, cout, K, 11, root, bias)
    t = torch.randn(n, cout, generator=gen, dtype=torch.float64)
    xr = x64.clone().requires_grad_(True)
    yr = spline_edge_list(xr, ei, a32.double(), *p64, ks, op, aggr)
    gr = torch.autograd.grad((yr * t).sum(), [xr] + [q for q in p64 if q is not None])
    x = x64.float().requires_grad_(True)
    p = tuple(None if q is None else q.detach().float().requires_grad_(True) for q in p64)
    g = spline_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    del spline_ops_stub.calls[:]
    y = nn_ops._SplineConvFn.apply(x, p[0], p[1], p[2], a32, g, kl, ol, aggr == "mean")
    gs = torch.autograd.grad((y * t.float()).sum(), [x] + [q for q in p if q is not None])
    assert spline_ops_stub.calls == ["spline_fwd", "spline_bwd_node"]
    assert y.shape == yr.shape == (n, cout) and relerr(y, yr) < 1e-5
    names = [nm for nm, q in zip(NAMES, (1,) + p64) if q is not None]
    assert len(names) == len(gs) == len(gr)
    for u, v, nm in zip(gs, gr, names):
        assert u.shape == v.shape and u.dtype == torch.float32, nm
        assert relerr(u, v) < 1e-5, (nm, relerr(u, v))
    # float64 pseudo-coordinates are rounded once
    assert torch.equal(nn_ops._SplineConvFn.apply(x, p[0], p[1], p[2], a32.double(), g, kl, ol, aggr == "mean"), y)


@pytest.mark.parametrize("root", [True, False])
def test_packing_and_unpacking_of_weight_are_exact_on_integer_data(meshes, monkeypatch, root):
    """Integer features, weights and cotangents, basis weights that are multiples of 1/4 (kernel_size 3, open: v = 2 a with a a
    multiple of 1/4) and ``aggr="add"``: every intermediate is an exact float32, so the [K, in, out] <-> [K * out, in] packing, the
    [Hf | R] and [dHf | dR] row buffers and the gradient's way back must reproduce the float64 reference to the last bit."""
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", spline_ops_stub)
    ei, n = meshes["grid"]
    gen = torch.Generator().manual_seed(4)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).double()
    cin, cout, ks, op = 5, 6, (3, 3), (True, True)
    x64, t = ri(-3, 3, n, cin), ri(-2, 2, n, cout)
    a = torch.randint(0, 5, (ei.shape[1], 2), generator=gen).double() / 4
    p64 = (ri(-2, 2, 9, cin, cout).requires_grad_(True), ri(-2, 2, cout, cin).requires_grad_(True) if root else None,
           ri(-2, 2, cout).requires_grad_(True))
    xr = x64.clone().requires_grad_(True)
    yr = spline_edge_list(xr, ei, a, *p64, ks, op, "add")
    gr = torch.autograd.grad((yr * t).sum(), [xr] + [q for q in p64 if q is not None])
    x = x64.float().requires_grad_(True)
    p = tuple(None if q is None else q.detach().float().requires_grad_(True) for q in p64)
    g = spline_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    y = nn_ops._SplineConvFn.apply(x, p[0], p[1], p[2], a.float(), g, ks, op, False)
    gs = torch.autograd.grad((y * t.float()).sum(), [x] + [q for q in p if q is not None])
    assert torch.equal(y.double(), yr)
    for u, v in zip(gs, gr):
        assert u.shape == v.shape and torch.equal(u.double(), v)
    assert float(gr[1].abs().max()) > 0


def test_parameter_names_shapes_and_init():
    from dual_dmp_amd.nn_ops import SplineConv
    torch.manual_seed(0)
    conv = SplineConv(40, 24, dim=3, kernel_size=5)
    sd = conv.state_dict()
    assert sorted(sd) == ["bias", "lin.weight", "weight"]
    assert sorted(n for n, _ in conv.named_parameters()) == ["bias", "lin.weight", "weight"]
    assert sd["weight"].shape == (125, 40, 24) and sd["lin.weight"].shape == (24, 40) and sd["bias"].shape == (24,)
    assert bool((sd["bias"] == 0).all())
    for key, a in (("weight", 1.0 / math.sqrt(40 * 125)), ("lin.weight", 1.0 / math.sqrt(40))):
        t = sd[key]
        assert t.abs().max() <= a and t.abs().max() > 0.95 * a, key
        assert abs(float(t.mean())) < 0.1 * a
    assert (conv.kernel_size, conv.is_open_spline, conv.K, conv.degree, conv.aggr) == ((5, 5, 5), (True, True, True), 125, 1, "mean")
    mixed = SplineConv(4, 8, 2, [2, 3], is_open_spline=[True, False], aggr="add", degree=1)
    assert (mixed.kernel_size, mixed.is_open_spline, mixed.K, mixed.aggr) == ((2, 3), (True, False), 6, "add")
    assert mixed.weight.shape == (6, 4, 8)
    assert SplineConv(4, 8, 5, 2).K == 32 and SplineConv(4, 8, 2, 1).K == 1
    assert SplineConv(40, 24, 3, 5, bias=False).bias is None
    noroot = SplineConv(40, 24, 3, 5, root_weight=False)
    assert noroot.lin is None and sorted(noroot.state_dict()) == ["bias", "weight"]
    conv2 = SplineConv(40, 24, dim=3, kernel_size=5)
    conv2.load_state_dict(sd)
    assert torch.equal(conv2.weight, sd["weight"]) and torch.equal(conv2.lin.weight, sd["lin.weight"])
    ref = SplineConvRef(40, 24, 3, 5)
    assert sorted(n for n, _ in ref.named_parameters()) == sorted(sd)
    assert [tuple(p.shape) for _, p in sorted(ref.named_parameters())] == [tuple(sd[k].shape) for k in sorted(sd)]
    ref.load_from(conv)
    assert torch.equal(ref.weight.float(), conv.weight) and torch.equal(ref.lin.weight.float(), conv.lin.weight)


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import SplineConv

    class Trap:
        DdmpError = ops.DdmpError
        SPLINE_MAX_DIM = ops.SPLINE_MAX_DIM

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    with pytest.raises(ValueError):
        SplineConv((4, 4), 8, 3, 2)
    for degree in (0, 2, 3):
        with pytest.raises(ValueError):
            SplineConv(4, 8, 3, 2, degree=degree)
    for aggr in ("max", "sum", "min", None):
        with pytest.raises(ValueError):
            SplineConv(4, 8, 3, 2, aggr=aggr)
    with pytest.raises(TypeError):
        SplineConv(4, 8, 3, 2, flow="target_to_source")
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            SplineConv(4, 8, bad, 2)
        with pytest.raises(ValueError):
            SplineConv(4, 8, 3, bad)
    with pytest.raises(ValueError):
        SplineConv(4, 8, 6, 2)                                   # dim > 5
    for ks in ((2, 2), (2, 2, 2, 2), (2, 0, 2), (2, 2.0, 2), "222"):
        with pytest.raises(ValueError):
            SplineConv(4, 8, 3, ks)
    for op in (1, None, (True, True), (True, 1, False), "yes"):
        with pytest.raises(ValueError):
            SplineConv(4, 8, 3, 2, is_open_spline=op)
    with pytest.raises(ValueError):
        SplineConv(4, 1 << 12, 3, 16)                            # K * out = 2^24
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    attr = torch.rand(2, 3)
    conv = SplineConv(4, 8, 3, 2)
    with pytest.raises(ValueError):
        conv((x, x), ei, attr)
    with pytest.raises(ValueError):
        conv(x, ei, attr, size=(6, 6))
    with pytest.raises(ValueError):
        conv(x.to(torch.bfloat16), ei, attr)
    with pytest.raises(ValueError):
        conv(torch.randn(6, 5), ei, attr)
    with pytest.raises(ValueError):
        conv(x, ei)                                              # edge_attr missing
    with pytest.raises(ValueError):
        conv(x, ei, None)
    for bad in (torch.rand(2, 2), torch.rand(3, 3), torch.rand(2), torch.rand(2, 3, 1)):
        with pytest.raises(ValueError):
            conv(x, ei, bad)
    for dt in (torch.float16, torch.bfloat16, torch.int64):
        with pytest.raises(ValueError):
            conv(x, ei, attr.to(dt))
    with pytest.raises(ValueError):
        conv(x, ei, attr.clone().requires_grad_(True))           # no silent None gradient
    with pytest.raises(ops.DdmpError):
        conv(x, ei, attr)                                        # CPU tensors: no CPU fallback
    with pytest.raises(ops.DdmpError):
        conv(x, ei, attr.double())


def test_modular_nets_take_conv_spline():
    from dual_dmp_amd.networks import NormalNet, PosNet
    from dual_dmp_amd.nn_ops import SplineConv
    from dual_dmp_amd.engine import NORM_WIDTHS, POS_WIDTHS
    for mk, widths in ((PosNet, POS_WIDTHS), (NormalNet, NORM_WIDTHS)):
        net = mk(torch.device("cpu"), fused=False, conv="spline", K=2)
        convs = [getattr(net, "conv%d" % i) for i in range(1, 13)]
        assert all(isinstance(c, SplineConv) for c in convs)
        assert [(c.in_channels, c.out_channels, c.dim, c.kernel_size) for c in convs] == \
            [(widths[i], widths[i + 1], 3, (2, 2, 2)) for i in range(12)]
        names = [n for n, _ in net.named_parameters()]
        for i in (1, 12):
            for leaf in ("weight", "lin.weight", "bias"):
                assert "conv%d.%s" % (i, leaf) in names
        assert len([n for n in names if n.startswith("conv")]) == 12 * 3
        assert net.conv3.weight.shape == (8, widths[2], widths[3]) and net.conv3.lin.weight.shape == (widths[3], widths[2])
        with pytest.raises(ValueError):
            mk(torch.device("cpu"), fused=True, conv="spline", K=2)
        for bad in ("sage", "splinecnn", "Spline"):
            with pytest.raises(ValueError) as info:
                mk(torch.device("cpu"), fused=False, conv=bad)
            for old in ("gcn", "cheb", "gat", "feast", "edge", "gmm", "transformer", "resgated", "spline"):
                assert "'%s'" % old in str(info.value)


def test_modular_net_pseudo_coordinates_serve_spline_as_they_serve_gmm():
    from types import SimpleNamespace
    from dual_dmp_amd.networks import PosNet
    from dual_dmp_amd.nn_ops import cartesian_pseudo
    net = PosNet(torch.device("cpu"), fused=False, conv="spline", K=2)
    pos, ei = torch.randn(9, 3), torch.randint(0, 9, (2, 30))
    data = SimpleNamespace()
    a = net._pseudo(data, "edge_attr", pos, ei)
    assert torch.equal(a, cartesian_pseudo(pos, ei)) and net._pseudo(data, "edge_attr", pos, ei) is a
    assert not a.requires_grad and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    data.edge_attr = torch.rand(30, 3)
    assert net._pseudo(data, "edge_attr", pos, ei) is data.edge_attr


def test_the_two_entry_points_are_declared():
    from dual_dmp_amd import _lib
    protos = _lib.parse_header()
    for name, nargs in (("ddmp_spline_fwd_f32", 15), ("ddmp_spline_bwd_node_f32", 14)):
        assert name in protos and protos[name][0] == "int" and len(protos[name][1]) == nargs
    assert not any(k.startswith("ddmp_spline_bwd_edge") for k in protos)     # the basis has no parameters: no edge side

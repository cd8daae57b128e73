"""GMMConv: everything that can be checked without a GPU -- the two float64 references against each other, the host side of
``nn_ops._GMMConvFn`` over torch restatements of the kernels (tests/gmm_ops_stub.py), the K = 1 / huge sigma special case against a
plain mean aggregation, parameter names / shapes / initialisation, the refusals, ``cartesian_pseudo`` and the modular nets'
``conv="gmm"``."""
import math

import pytest
import torch

import gmm_ops_stub
from gmm_ref import GMMConvRef, dense_gmm, gmm_edge_list


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
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    for name, (v, f) in (("ico", synth.icosphere(2)), ("grid", synth.open_grid(9, 7))):
        e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
        out[name] = (_with_extras(torch.cat([e, e[[1, 0]]], 1)), len(v))
    return out


def _params(cin, cout, K, dim, seed, root=True, bias=True, dtype=torch.float64):
    """(g, mu, sigma, root.weight | None, bias | None), each requiring grad; mu in [0, 1], sigma in [0.3, 1]."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: (torch.randn(*s, generator=gen, dtype=torch.float64) * 0.5).to(dtype).requires_grad_(True)
    ru = lambda lo, hi, *s: (lo + (hi - lo) * torch.rand(*s, generator=gen, dtype=torch.float64)).to(dtype).requires_grad_(True)
    return rn(cin, K * cout), ru(0.0, 1.0, K, dim), ru(0.3, 1.0, K, dim), rn(cout, cin) if root else None, rn(cout) if bias else None


def _attr(E, dim, seed, dtype=torch.float64):
    """Pseudo-coordinates uniform in [0, 1]^dim, one draw per input edge: duplicates get different ones."""
    return torch.rand(E, dim, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype)


NAMES = ("dx", "dattr", "dg", "dmu", "dsigma", "droot", "db")


@pytest.mark.parametrize("name", ["ico", "grid"])
@pytest.mark.parametrize("K,dim", [(1, 3), (3, 2), (4, 1)])
def test_the_two_references_agree_in_float64(meshes, name, K, dim):
    ei, n = meshes[name]
    gen = torch.Generator().manual_seed(n + K)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    a = _attr(ei.shape[1], dim, 17).requires_grad_(True)
    assert not torch.equal(a[:50], a[-100:-50])                  # the duplicated edges carry other pseudo-coordinates
    p = _params(5, 4, K, dim, 3)
    t = torch.randn(n, 4, generator=gen, dtype=torch.float64)
    outs, grads = [], []
    for fn in (gmm_edge_list, dense_gmm):
        y = fn(x, ei, a, *p, K)
        outs.append(y)
        grads.append(torch.autograd.grad((y * t).sum(), (x, a) + p))
    assert relerr(outs[0], outs[1]) < 1e-13
    for u, v, nm in zip(*grads, NAMES):
        assert relerr(u, v) < 1e-12, (nm, relerr(u, v))


CASES = [(3, 3, 2, 3), (16, 4, 8, 2), (5, 6, 3, 1), (8, 8, 1, 3)]     # (in, out, K, dim): ragged widths go through the padding


@pytest.mark.parametrize("cin,cout,K,dim", CASES)
@pytest.mark.parametrize("root", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_gmmconv_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, cin, cout, K, dim, root, bias):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", gmm_ops_stub)
    ei, n = meshes["ico"]
    gen = torch.Generator().manual_seed(cin * 7 + K)
    x64 = torch.randn(n, cin, generator=gen, dtype=torch.float64)
    a64 = _attr(ei.shape[1], dim, 23)
    p64 = _params(cin, cout, K, dim, 11, root, bias)
    t = torch.randn(n, cout, generator=gen, dtype=torch.float64)
    xr, ar = x64.clone().requires_grad_(True), a64.clone().requires_grad_(True)
    yr = gmm_edge_list(xr, ei, ar, *p64, K)
    gr = torch.autograd.grad((yr * t).sum(), [xr, ar] + [q for q in p64 if q is not None])
    x, a = x64.float().requires_grad_(True), a64.float().requires_grad_(True)
    p = tuple(None if q is None else q.detach().float().requires_grad_(True) for q in p64)
    g = gmm_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    del gmm_ops_stub.calls[:]
    y = nn_ops._GMMConvFn.apply(x, p[0], p[1], p[2], p[3], p[4], a, g, K)
    gs = torch.autograd.grad((y * t.float()).sum(), [x, a] + [q for q in p if q is not None])
    assert gmm_ops_stub.calls == ["gmm_fwd", "gmm_bwd_edge", "gmm_bwd_node", "feast_dc"]
    assert y.shape == yr.shape == (n, cout) and relerr(y, yr) < 1e-5
    names = [nm for nm, q in zip(NAMES, (1, 1) + p64) if q is not None]
    assert len(names) == len(gs) == len(gr)
    for u, v, nm in zip(gs, gr, names):
        assert u.shape == v.shape and u.dtype == torch.float32, nm
        assert relerr(u, v) < 1e-5, (nm, relerr(u, v))
    # without a gradient request for the pseudo-coordinates the edge-side launch is not asked for dattr
    y = nn_ops._GMMConvFn.apply(x, p[0], p[1], p[2], p[3], p[4], a.detach(), g, K)
    seen = []
    monkeypatch.setattr(gmm_ops_stub, "gmm_bwd_edge",
                        lambda *args, _f=gmm_ops_stub.gmm_bwd_edge, **kw: (seen.append(kw.get("want_dattr")), _f(*args, **kw))[1])
    torch.autograd.grad((y * t.float()).sum(), [x])
    assert seen == [False]


def test_float64_pseudo_coordinates_are_rounded_once_and_get_a_float64_gradient(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", gmm_ops_stub)
    ei, n = meshes["grid"]
    g = gmm_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    p = tuple(q.detach().float() for q in _params(4, 4, 2, 3, 5))
    x = torch.randn(n, 4, generator=torch.Generator().manual_seed(1))
    a64 = _attr(ei.shape[1], 3, 9).requires_grad_(True)
    y64 = nn_ops._GMMConvFn.apply(x, *p, a64, g, 2)
    y32 = nn_ops._GMMConvFn.apply(x, *p, a64.detach().float(), g, 2)
    assert torch.equal(y64, y32)
    (da,) = torch.autograd.grad(y64.sum(), [a64])
    assert da.dtype == torch.float64 and da.shape == a64.shape


def test_one_gaussian_with_a_huge_sigma_is_the_plain_mean_aggregation(meshes):
    ei, n = meshes["grid"]
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(n, 6, generator=gen, dtype=torch.float64)
    g = torch.randn(6, 4, generator=gen, dtype=torch.float64)
    a = _attr(ei.shape[1], 3, 2)
    mu, sigma = torch.rand(1, 3, generator=gen, dtype=torch.float64), torch.full((1, 3), 1e12, dtype=torch.float64)
    src, dst = ei
    h = x @ g
    cnt = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(len(dst), dtype=torch.float64))
    mean = torch.zeros((n, 4), dtype=torch.float64).index_add_(0, dst, h[src]) / cnt.clamp(min=1).unsqueeze(1)
    assert relerr(gmm_edge_list(x, ei, a, g, mu, sigma, None, None, 1), mean) < 1e-14
    assert relerr(dense_gmm(x, ei, a, g, mu, sigma, None, None, 1), mean) < 1e-14
    gr = gmm_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    y, w = gmm_ops_stub.gmm_fwd(gr, h.float(), a.float(), mu.float(), sigma.float(), 1)
    assert relerr(y, mean) < 1e-6
    assert torch.allclose(torch.zeros(n, dtype=torch.float64).index_add_(0, gr.row, w.double()[:, 0]), (cnt > 0).double(), atol=1e-6)


def test_parameter_names_shapes_and_init():
    from dual_dmp_amd.nn_ops import GMMConv
    torch.manual_seed(0)
    conv = GMMConv(40, 24, dim=3, kernel_size=5)
    sd = conv.state_dict()
    assert list(sd) == ["g", "mu", "sigma", "bias", "root.weight"]
    assert [n for n, _ in conv.named_parameters()] == ["g", "mu", "sigma", "bias", "root.weight"]
    assert sd["g"].shape == (40, 120) and sd["mu"].shape == (5, 3) and sd["sigma"].shape == (5, 3)
    assert sd["root.weight"].shape == (24, 40) and sd["bias"].shape == (24,)
    assert bool((sd["bias"] == 0).all())
    for key, frac in (("g", 0.95), ("root.weight", 0.95), ("mu", 0.5), ("sigma", 0.5)):
        t = sd[key]
        a = math.sqrt(6.0 / (t.shape[0] + t.shape[1]))           # PyG 'glorot': the fan of the last two dimensions
        assert t.abs().max() <= a and t.abs().max() > frac * a, key
    assert abs(float(sd["g"].mean())) < 0.05 * math.sqrt(6.0 / 160)
    assert GMMConv(40, 24, 3, 5, bias=False).bias is None
    noroot = GMMConv(40, 24, 3, 5, root_weight=False)
    assert noroot.root is None and list(noroot.state_dict()) == ["g", "mu", "sigma", "bias"]
    assert GMMConv(40, 24, 2, 64, aggr="mean", separate_gaussians=False).kernel_size == 64      # 2 K dim = 256 is the limit
    conv2 = GMMConv(40, 24, dim=3, kernel_size=5)
    conv2.load_state_dict(sd)
    assert torch.equal(conv2.sigma, sd["sigma"])
    ref = GMMConvRef(40, 24, 3, 5)
    assert sorted(n for n, _ in ref.named_parameters()) == sorted(sd)
    assert [tuple(p.shape) for _, p in sorted(ref.named_parameters())] == [tuple(sd[k].shape) for k in sorted(sd)]
    ref.load_from(conv)
    assert torch.equal(ref.g.float(), conv.g) and torch.equal(ref.root.weight.float(), conv.root.weight)


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import GMMConv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    with pytest.raises(ValueError):
        GMMConv((4, 4), 8, 3, 2)
    with pytest.raises(ValueError):
        GMMConv(4, 8, 3, 2, separate_gaussians=True)
    for aggr in ("add", "max", "sum"):
        with pytest.raises(ValueError):
            GMMConv(4, 8, 3, 2, aggr=aggr)
    for k in (0, -1, 2.0):
        with pytest.raises(ValueError):
            GMMConv(4, 8, 3, k)
        with pytest.raises(ValueError):
            GMMConv(4, 8, k, 2)
    with pytest.raises(ValueError):
        GMMConv(4, 8, 3, 43)                                     # 2 * 43 * 3 = 258 > 256
    with pytest.raises(ValueError):
        GMMConv(4, 8, 129, 1)
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    attr = torch.rand(2, 3)
    conv = GMMConv(4, 8, 3, 2)
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
    with pytest.raises(ops.DdmpError):
        conv(x, ei, attr)                                        # CPU tensors: no CPU fallback
    with pytest.raises(ops.DdmpError):
        conv(x, ei, attr.double())


def test_cartesian_pseudo_is_the_written_out_formula():
    from dual_dmp_amd.nn_ops import cartesian_pseudo
    gen = torch.Generator().manual_seed(3)
    pos = torch.randn(20, 3, generator=gen, dtype=torch.float64)
    ei = torch.randint(0, 20, (2, 70), generator=gen)
    raw = torch.stack([pos[int(ei[0, t])] - pos[int(ei[1, t])] for t in range(70)])
    assert torch.equal(cartesian_pseudo(pos, ei, norm=False), raw)
    got = cartesian_pseudo(pos, ei)
    assert got.shape == (70, 3) and torch.allclose(got, raw / (2 * raw.abs().max()) + 0.5, rtol=0, atol=1e-15)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 and (float(got.min()) == 0.0 or float(got.max()) == 1.0)
    assert torch.allclose(cartesian_pseudo(pos, ei, max_value=10.0), raw / 20.0 + 0.5, rtol=0, atol=1e-15)
    assert cartesian_pseudo(pos[:, 0], ei).shape == (70, 1)      # 1-D positions: one pseudo-coordinate per edge
    assert cartesian_pseudo(pos.float(), ei).dtype == torch.float32


def test_modular_nets_take_conv_gmm():
    from dual_dmp_amd.networks import NormalNet, PosNet
    from dual_dmp_amd.nn_ops import GMMConv
    from dual_dmp_amd.engine import NORM_WIDTHS, POS_WIDTHS
    for mk, widths in ((PosNet, POS_WIDTHS), (NormalNet, NORM_WIDTHS)):
        net = mk(torch.device("cpu"), fused=False, conv="gmm", K=3)
        convs = [getattr(net, "conv%d" % i) for i in range(1, 13)]
        assert all(isinstance(c, GMMConv) for c in convs)
        assert [(c.in_channels, c.out_channels, c.dim, c.kernel_size) for c in convs] == [(widths[i], widths[i + 1], 3, 3) for i in range(12)]
        names = [n for n, _ in net.named_parameters()]
        for i in (1, 12):
            for leaf in ("g", "mu", "sigma", "root.weight", "bias"):
                assert "conv%d.%s" % (i, leaf) in names
        assert len([n for n in names if n.startswith("conv")]) == 12 * 5
        assert net.conv3.g.shape == (widths[2], 3 * widths[3]) and net.conv3.root.weight.shape == (widths[3], widths[2])
        assert mk(torch.device("cpu"), fused=False, conv="gmm", K=5).conv1.kernel_size == 5
        with pytest.raises(ValueError):
            mk(torch.device("cpu"), fused=True, conv="gmm", K=3)
        for bad in ("sage", "monet", "GMM"):
            with pytest.raises(ValueError) as info:
                mk(torch.device("cpu"), fused=False, conv=bad)
            assert "'gmm'" in str(info.value)


def test_modular_net_pseudo_coordinates_come_from_the_dataset_or_are_cached_on_it():
    from types import SimpleNamespace
    from dual_dmp_amd.networks import PosNet
    from dual_dmp_amd.nn_ops import cartesian_pseudo
    net = PosNet(torch.device("cpu"), fused=False, conv="gmm", K=2)
    pos, ei = torch.randn(9, 3), torch.randint(0, 9, (2, 30))
    data = SimpleNamespace()
    a = net._pseudo(data, "edge_attr", pos, ei)
    assert torch.equal(a, cartesian_pseudo(pos, ei)) and net._pseudo(data, "edge_attr", pos, ei) is a
    assert net._pseudo(data, "edge_attr", pos.clone(), ei) is not a              # other positions: computed again
    z2 = torch.randn(9, 7)
    f = net._pseudo(data, "face_attr", z2, ei, cols=3)
    assert torch.equal(f, cartesian_pseudo(z2[:, :3], ei)) and net._pseudo(data, "face_attr", z2, ei, cols=3) is f
    data.edge_attr = torch.rand(30, 3)
    assert net._pseudo(data, "edge_attr", pos, ei) is data.edge_attr
    assert PosNet(torch.device("cpu"), fused=False, conv="feast")._pseudo(data, "edge_attr", pos, ei) is None

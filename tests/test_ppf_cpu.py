"""PPFConv: everything that can be checked without a GPU -- the two float64 references (tests/ppf_ref.py) against each other and on a
graph done by hand, the host side of ``nn_ops._PPFConvFn`` / ``PPFConv`` over torch restatements of the kernels
(tests/ppf_ops_stub.py), parameter names / shapes / ownership, the refusals, the call sequence, what is saved, the declarations of
the three entry points, ``point_pair_features`` and the nets."""
import math

import pytest
import torch
import torch.nn as nn

import ppf_ops_stub
from ppf_ref import PPFConvRef, ppf_dense, ppf_edge_list, ppf_features


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def small_graph():
    """12 nodes: a ring 0 .. 10 (both directions), chords, duplicate edges (3 -> 4 three times and 4 -> 3 once, 7 <-> 8 twice
    each), an explicit loop on node 5, and node 11 without any edge."""
    ring = [(k, (k + 1) % 11) for k in range(11)]
    und = ring + [(0, 5), (2, 9)]
    e = und + [(b, a) for a, b in und] + [(3, 4), (3, 4), (7, 8), (8, 7), (5, 5)]
    return torch.tensor(e, dtype=torch.long).t().contiguous(), 12


def geometry(n, seed, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    pos = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    nrm = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    return pos.to(dtype), (nrm / nrm.norm(dim=1, keepdim=True)).to(dtype)


def make_local(cin, cout, bias, leaky, gen):
    a = 1.0 / math.sqrt(cin + 4)
    lin = nn.Linear(cin + 4, cout, bias=bias)
    with torch.no_grad():
        for p in lin.parameters():
            p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * a)
    return nn.Sequential(lin, nn.LeakyReLU(0.2)) if leaky else lin


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("cin", [0, 5])
@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("glob", [True, False])
def test_the_two_references_agree_in_float64(cin, loops, glob):
    ei, n = small_graph()
    gen = torch.Generator().manual_seed(cin + 3)
    pos, nrm = geometry(n, 1, torch.float64)
    x = torch.randn(n, cin, generator=gen, dtype=torch.float64, requires_grad=True) if cin else None
    local = nn.Sequential(nn.Linear(cin + 4, 6), nn.LeakyReLU(0.2)).double()
    g_nn = nn.Linear(6, 3).double() if glob else None
    t = torch.randn(n, 3 if glob else 6, generator=gen, dtype=torch.float64)
    leaves = ([x] if cin else []) + list(local.parameters()) + (list(g_nn.parameters()) if glob else [])
    outs, grads = [], []
    for fn in (ppf_edge_list, ppf_dense):
        y = fn(x, pos, nrm, ei, local, g_nn, loops)
        outs.append(y)
        grads.append(torch.autograd.grad((y * t).sum(), leaves))
    assert relerr(outs[0], outs[1]) < 1e-12
    for u, v in zip(*grads):
        assert relerr(u, v) < 1e-12


def test_the_reference_on_a_graph_done_by_hand():
    """Node 0 has a loop (features 0) and receives 1 -> 0 twice (a duplicate); node 1 receives 0 -> 1; node 2 has no incoming
    edge.  Positions on the x axis, normals along z and y: |d| = 2, every angle pi / 2."""
    pos = torch.tensor([[0.0, 0, 0], [2.0, 0, 0], [5.0, 5, 5]], dtype=torch.float64)
    nrm = torch.tensor([[0.0, 0, 1], [0.0, 1, 0], [1.0, 0, 0]], dtype=torch.float64)
    ei = torch.tensor([[0, 1, 1, 0], [0, 0, 0, 1]])
    f = ppf_features(pos, nrm, ei)
    h = math.pi / 2
    assert torch.equal(f[0], torch.zeros(4, dtype=torch.float64))            # the loop: atan2(0, 0) = 0, atan2(0, 1) = 0
    assert torch.allclose(f[1], torch.tensor([2.0, h, h, h], dtype=torch.float64), atol=1e-15) and torch.equal(f[1], f[2])
    assert torch.allclose(f[3], torch.tensor([2.0, h, h, h], dtype=torch.float64), atol=1e-15)
    x = torch.tensor([[1.0], [-3.0], [7.0]], dtype=torch.float64)
    lin = nn.Linear(5, 2).double()
    with torch.no_grad():
        lin.weight.copy_(torch.tensor([[1.0, 0.5, 0, 0, 0], [-1.0, 0, 1.0, 0, 0]]))
        lin.bias.copy_(torch.tensor([0.25, -0.25]))
    y = PPFConvRef(lin, add_self_loops=False)(x, pos, nrm, ei)
    m = lambda xj, ff: [xj + 0.5 * ff[0] + 0.25, -xj + ff[1] - 0.25]
    loop, e10, e01 = m(1.0, [0, 0]), m(-3.0, [2.0, h]), m(1.0, [2.0, h])
    want = torch.tensor([[max(loop[0], e10[0]), max(loop[1], e10[1])], e01, [0.0, 0.0]], dtype=torch.float64)
    assert torch.allclose(y, want, atol=1e-14)
    # add_self_loops: the explicit loop is replaced by one loop per node, node 2 now sees its own loop
    y2 = PPFConvRef(lin, add_self_loops=True)(x, pos, nrm, ei)
    l1, l2 = m(-3.0, [0, 0]), m(7.0, [0, 0])
    want2 = torch.tensor([want[0].tolist(), [max(e01[0], l1[0]), max(e01[1], l1[1])], l2], dtype=torch.float64)
    assert torch.allclose(y2, want2, atol=1e-14)
    assert torch.allclose(ppf_dense(x, pos, nrm, ei, lin, None, True), want2, atol=1e-14)


# ------------------------------------------------------------------------------------------------ the drop-in over the stub
def _operator_run(conv, x, pos, nrm, ei, t):
    x = None if x is None else x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, pos, nrm, ei)
    (y * t).sum().backward()
    return dict([("y", y.detach())] + ([("dx", x.grad)] if x is not None else []) + [("d " + k, p.grad) for k, p in conv.named_parameters()])


@pytest.fixture
def stubbed(monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", ppf_ops_stub)
    monkeypatch.setattr(nn_ops, "_need_gpu", lambda *a, **k: None)           # (the stub runs on CPU tensors)
    del ppf_ops_stub.calls[:], ppf_ops_stub.want_args[:]
    return nn_ops


@pytest.mark.parametrize("cin,cout", [(0, 3), (5, 8), (8, 5)])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("leaky", [False, True])
@pytest.mark.parametrize("glob", [False, True])
@pytest.mark.parametrize("loops", [True, False])
def test_the_drop_in_over_the_stub_equals_the_reference(stubbed, cin, cout, bias, leaky, glob, loops):
    ei, n = small_graph()
    gen = torch.Generator().manual_seed(cin + cout)
    local = make_local(cin, cout, bias, leaky, gen)
    torch.manual_seed(3)
    g_nn = nn.Sequential(nn.Linear(cout, 4), nn.Tanh()) if glob else None
    conv = stubbed.PPFConv(local, g_nn, add_self_loops=loops)
    ref = PPFConvRef(local, g_nn, add_self_loops=loops)
    pos, nrm = geometry(n, 2)
    x = torch.randn(n, cin, generator=gen) if cin else None
    t = torch.randn(n, 4 if glob else cout, generator=gen)
    got = _operator_run(conv, x, pos, nrm, ei, t)
    want = _operator_run(ref, None if x is None else x.double(), pos.double(), nrm.double(), ei, t.double())
    assert list(got) == list(want) and len(got) == 1 + (cin > 0) + 1 + bias + 2 * glob
    for k in got:
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float32, k
        assert relerr(got[k], want[k]) <= 1e-5, (k, relerr(got[k], want[k]))
    if not loops and not glob:
        assert torch.equal(got["y"][11], torch.zeros(cout))                  # the node without edges: 0, no bias
    # float64 geometry is rounded once
    again = _operator_run(conv, x, pos.double(), nrm.double(), ei, t)
    assert all(torch.equal(again[k], got[k]) for k in got)


def test_state_dict_keys_shapes_and_the_users_own_parameters():
    from dual_dmp_amd.nn_ops import PPFConv
    lin = nn.Linear(9, 7)
    conv = PPFConv(lin)
    assert sorted(conv.state_dict()) == ["local_nn.bias", "local_nn.weight"]
    assert conv.local_nn is lin and conv.local_nn.weight is lin.weight and conv.global_nn is None
    assert (conv.in_channels, conv.out_channels, conv.aggr, conv.add_self_loops) == (5, 7, "max", True)
    seq, glob = nn.Sequential(nn.Linear(4, 6, bias=False), nn.ReLU()), nn.Sequential(nn.Linear(6, 2))
    conv2 = PPFConv(seq, glob, add_self_loops=False)
    assert sorted(conv2.state_dict()) == ["global_nn.0.bias", "global_nn.0.weight", "local_nn.0.weight"]
    assert conv2.state_dict()["local_nn.0.weight"].shape == (6, 4) and conv2.in_channels == 0 and not conv2.add_self_loops
    assert [p is q for p, q in zip(conv2.parameters(), list(seq.parameters()) + list(glob.parameters()))] == [True] * 3
    assert PPFConv(lin, aggr="max").aggr == "max"
    before = lin.weight.detach().clone()
    conv.reset_parameters()
    assert not torch.equal(lin.weight, before)
    assert "add_self_loops=True" in repr(conv)


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import PPFConv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    with pytest.raises(ValueError, match="local_nn"):
        PPFConv()
    with pytest.raises(ValueError, match="local_nn"):
        PPFConv(None, nn.Linear(4, 4))
    for bad in (nn.Sequential(nn.Linear(8, 4), nn.Sigmoid()), nn.Sequential(nn.Linear(8, 4), nn.ReLU(), nn.Linear(4, 4)),
                nn.Sequential(nn.ReLU(), nn.Linear(8, 4)), nn.Linear(8, 4).double(), nn.Linear(3, 4), nn.ReLU(),
                nn.Sequential(nn.Linear(8, 4), nn.LeakyReLU(-0.1)), nn.Sequential(nn.Linear(8, 4), nn.BatchNorm1d(4))):
        with pytest.raises(ValueError, match="PPFConv"):
            PPFConv(bad)
    for aggr in ("add", "mean", "min", None):
        with pytest.raises(ValueError, match="aggr"):
            PPFConv(nn.Linear(8, 4), aggr=aggr)
    with pytest.raises(TypeError):
        PPFConv(nn.Linear(8, 4), flow="target_to_source")
    conv, geo = PPFConv(nn.Linear(8, 4)), PPFConv(nn.Linear(4, 4))
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    pos, nrm = torch.randn(6, 3), torch.randn(6, 3)
    with pytest.raises(ValueError, match="tuple"):
        conv((x, x), pos, nrm, ei)
    with pytest.raises(ValueError, match="tuple"):
        conv(x, (pos, pos), nrm, ei)
    with pytest.raises(ValueError, match="tuple"):
        conv(x, pos, (nrm, nrm), ei)
    with pytest.raises(ValueError, match="bf16"):
        conv(x.to(torch.bfloat16), pos, nrm, ei)
    for bad in (torch.randn(6, 2), torch.randn(6), torch.randn(5, 3), torch.randn(6, 3, 1)):
        with pytest.raises(ValueError, match="normal"):
            conv(x, pos, bad, ei)
    for bad in (torch.randn(6, 2), torch.randn(6), torch.randn(6, 3, 1)):
        with pytest.raises(ValueError, match="pos"):
            conv(x, bad, nrm, ei)
    for dt in (torch.float16, torch.bfloat16, torch.int64):
        with pytest.raises(ValueError, match="float32 or float64"):
            conv(x, pos.to(dt), nrm, ei)
        with pytest.raises(ValueError, match="float32 or float64"):
            conv(x, pos, nrm.to(dt), ei)
    with pytest.raises(ValueError, match="pos"):
        conv(x, pos.clone().requires_grad_(True), nrm, ei)                   # no silent None gradient
    with pytest.raises(ValueError, match="normal"):
        conv(x, pos, nrm.clone().requires_grad_(True), ei)
    for bad in (torch.randn(6, 5), torch.randn(6), torch.randn(5, 4), None):
        with pytest.raises(ValueError, match="shape"):
            conv(bad, pos, nrm, ei)
    with pytest.raises(ValueError, match="shape"):
        geo(x, pos, nrm, ei)                                                 # a local_nn of in_features 4 takes x=None
    with pytest.raises(ValueError, match="no CPU fallback"):
        conv(x, pos, nrm, ei)                                                # CPU tensors
    with pytest.raises(ValueError, match="no CPU fallback"):
        geo(None, pos.double(), nrm, ei)
    with pytest.raises(ValueError, match="local_nn"):                        # the user's module edited since
        conv.local_nn = nn.Sequential(nn.Linear(8, 4), nn.Sigmoid())
        conv(x, pos, nrm, ei)


# ------------------------------------------------------------------------------------------------ the call sequence
def test_one_gemm_of_each_kind_two_launches_and_nothing_saved_per_edge(stubbed):
    ei, n = small_graph()
    g = ppf_ops_stub.graph_for(ei, n, norm="gat", add_self_loops=True)
    pos, nrm = geometry(n, 4)
    f = ppf_ops_stub.ppf_entries(g, pos, nrm)
    w = (torch.randn(8, 9) * 0.3).requires_grad_(True)
    b = torch.randn(8).requires_grad_(True)
    x = torch.randn(n, 5, requires_grad=True)
    del ppf_ops_stub.calls[:]
    y = stubbed._PPFConvFn.apply(x, w, b, f, g, True)
    saved = [t for t in y.grad_fn.saved_tensors if t is not None]
    # padded x [12, 8], packed weight [8, 8], arg [12, 8] int32, F [entries, 4]
    assert sorted((tuple(t.shape), str(t.dtype)) for t in saved) == sorted([((n, 8), "torch.float32"), ((8, 8), "torch.float32"),
                                                                             ((n, 8), "torch.int32"), ((g.nnz, 4), "torch.float32")])
    assert not any(t.dim() == 2 and t.shape[0] in (g.nnz, ei.shape[1]) and t.shape[1] >= 8 for t in saved)   # nothing C-wide per edge
    y.sum().backward()
    # C = 8 is a width ops.colsum takes
    assert ppf_ops_stub.calls == ["gemm_nt", "gather_max_attr", "gather_max_attr_bwd", "gatv2_datt", "colsum", "gemm_tn", "gemm_nn"]
    assert x.grad.shape == (n, 5) and w.grad.shape == (8, 9) and b.grad.shape == (8,)
    # x = None: no GEMM of any kind
    del ppf_ops_stub.calls[:]
    w4 = (torch.randn(8, 4) * 0.3).requires_grad_(True)
    y = stubbed._PPFConvFn.apply(None, w4, None, f, g, True)
    assert sorted(tuple(t.shape) for t in y.grad_fn.saved_tensors if t is not None) == sorted([(n, 8), (g.nnz, 4)])
    y.sum().backward()
    assert ppf_ops_stub.calls == ["gather_max_attr", "gather_max_attr_bwd", "gatv2_datt"] and w4.grad.shape == (8, 4)
    # the whole operator with x = None and a bias: still none, and one feature evaluation
    del ppf_ops_stub.calls[:]
    conv = stubbed.PPFConv(nn.Linear(4, 8))
    conv(None, pos, nrm, ei).sum().backward()
    assert ppf_ops_stub.calls == ["graph_for", "ppf_entries", "gather_max_attr", "gather_max_attr_bwd", "gatv2_datt"]
    assert conv.local_nn.bias.grad.shape == (8,) and conv.local_nn.weight.grad.shape == (8, 4)
    # a frozen weight: no partials, no column sum of them
    del ppf_ops_stub.calls[:]
    stubbed._PPFConvFn.apply(x, w.detach(), b, f, g, True).sum().backward()
    assert ppf_ops_stub.calls == ["gemm_nt", "gather_max_attr", "gather_max_attr_bwd", "colsum", "gemm_nn"]


def test_a_no_grad_forward_asks_for_no_arg(stubbed):
    ei, n = small_graph()
    pos, nrm = geometry(n, 5)
    conv = stubbed.PPFConv(nn.Linear(9, 6))
    x = torch.randn(n, 5)
    with torch.no_grad():
        y0 = conv(x, pos, nrm, ei)
    y1 = conv(x, pos, nrm, ei)
    assert ppf_ops_stub.want_args == [False, True] and torch.equal(y0, y1.detach())
    for p in conv.parameters():
        p.requires_grad_(False)
    conv(x, pos, nrm, ei)
    assert ppf_ops_stub.want_args[-1] is False


# ------------------------------------------------------------------------------------------------ declarations, helper, nets
def test_the_three_entry_points_are_declared():
    from dual_dmp_amd import _lib, ops
    protos = _lib.parse_header()
    want = {"ddmp_ppf_entries_f32": 7, "ddmp_gather_max_attr_f32": 11, "ddmp_gather_max_attr_bwd_f32": 11}
    for name, nargs in want.items():
        assert name in protos and len(protos[name][1]) == nargs and protos[name][0] == "int", name
    assert "#define DDMP_ABI_VERSION 3" in " ".join(open(_lib.HEADER).read().split())
    for name in ("ppf_entries", "gather_max_attr", "gather_max_attr_bwd"):
        assert callable(getattr(ops, name))
    from dual_dmp_amd.nn_ops import PPFConv, _PPFConvFn, point_pair_features  # noqa: F401


def test_point_pair_features_equals_the_reference():
    from dual_dmp_amd.nn_ops import point_pair_features
    ei, n = small_graph()
    pos, nrm = geometry(n, 6, torch.float64)
    f = point_pair_features(pos, nrm, ei)
    assert f.shape == (ei.shape[1], 4) and relerr(f, ppf_features(pos, nrm, ei)) < 1e-14
    assert float(f[-1].abs().max()) < 1e-15                                  # the explicit loop on node 5 (n x n under FMA contraction
    #                                                                          is not exactly 0 in torch either; the kernel writes 0)
    # rigid motions leave them alone
    q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0)))
    q = q * torch.sign(torch.det(q))
    moved = point_pair_features(pos @ q.t() + 3.0, nrm @ q.t(), ei)
    assert relerr(moved, f) < 1e-12


def test_the_modular_nets_take_the_operator_on_the_face_graph_only():
    from dual_dmp_amd import networks
    from dual_dmp_amd.networks import NormalNet, PosNet
    assert "ppf" in networks._CONVS and "'ppf'" in networks._CONV_MSG
    with pytest.raises(ValueError, match="normals"):
        PosNet(torch.device("cpu"), fused=False, conv="ppf")
    for net in (PosNet, NormalNet):
        with pytest.raises(ValueError, match="fused=False"):
            net(torch.device("cpu"), fused=True, conv="ppf")
    from dual_dmp_amd.engine import NORM_WIDTHS
    from dual_dmp_amd.nn_ops import PPFConv
    net = NormalNet(torch.device("cpu"), fused=False, conv="ppf")
    for i in range(12):
        layer = getattr(net, "conv%d" % (i + 1))
        assert isinstance(layer, PPFConv) and layer.local_nn.weight.shape == (NORM_WIDTHS[i + 1], NORM_WIDTHS[i] + 4)
    assert "conv3.local_nn.weight" in net.state_dict()

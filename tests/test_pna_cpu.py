"""PNAConv: everything that can be checked without a GPU -- the two float64 references against each other, the host side of
``nn_ops._PNAConvFn`` over torch restatements of the kernels (tests/pna_ops_stub.py) in float64 with its launch counts, parameter
names, ``degree_histogram`` and the scalers' deltas, the edgeless node, the zero-variance rows, the refusals, and the public header.

The host side is pure algebra on top of the two launches (packing, the tower-major buffer, the scalers applied after the post GEMM,
the chain rule of std / var folded into dS / dQ), so in float64 it must agree with the edge-list reference to rounding: <= 1e-10."""
import os
import re

import pytest
import torch

import pna_ops_stub as stub
from pna_ref import PNAConvRef, degree_histogram, deltas, pna_forward, scaler_table
from test_edgeconv_cpu import _with_extras, relerr

HOST_TOL = 1e-10
DIMS = [(3, 4, 1), (8, 8, 2), (12, 10, 2), (16, 32, 4)]          # (in, out, towers)
AGGRS = [["mean", "min", "max", "std"], ["sum", "var"], ["std"], ["max"]]
SCALERS = [["identity", "amplification", "attenuation"], ["linear", "inverse_linear"], ["identity"]]
ids = lambda a: "+".join(a) if isinstance(a, list) else str(a)


def err(a, b):
    """rel-L2, with the reference's norm floored at 1: std and var do not see the pre bias at all (they are shift invariant), so
    with those aggregators alone its gradient is exactly 0 and both sides hold rounding noise of the O(1) terms that cancel."""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / max(float(b.norm()), 1.0))


def with_special_rows(ei, n):
    """On top of a mesh with n nodes: node n is a PENDANT (one edge, to node 0), node n + 1 has three edges, all from node 1 (a row
    whose entries are all the same source), node n + 2 has no edge at all -> (edge_index, n + 3)."""
    extra = torch.tensor([[n, 0, n + 1, 1, n + 1, 1, n + 1, 1], [0, n, 1, n + 1, 1, n + 1, 1, n + 1]])
    return torch.cat([ei, extra], 1).contiguous(), n + 3


@pytest.fixture(scope="module")
def meshes():
    """name -> (edge_index, n): the small icosphere and the open grid with duplicates and two loops on node 5 on top
    (test_edgeconv_cpu.py's recipe), then the pendant node, the one-source node and the edgeless node."""
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    for name, (v, f) in (("ico", synth.icosphere(2)), ("grid", synth.open_grid(9, 7))):
        e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
        out[name] = with_special_rows(_with_extras(torch.cat([e, e[[1, 0]]], 1)), len(v))
    return out


def _ref_and_inputs(ei, n, cin, cout, towers, aggrs, scalers, seed):
    torch.manual_seed(seed)
    ref = PNAConvRef(cin, cout, aggrs, scalers, degree_histogram(ei, n), towers)
    gen = torch.Generator().manual_seed(seed + 1)
    return ref, torch.randn(n, cin, generator=gen, dtype=torch.float64), torch.randn(n, cout, generator=gen, dtype=torch.float64)


def _grads(mod, x, ei, t, call):
    x = x.clone().requires_grad_(True)
    y = call(mod, x, ei)
    names = [k for k, _ in mod.named_parameters()]
    g = torch.autograd.grad((y * t).sum(), [x] + [p for _, p in mod.named_parameters()])
    return dict(zip(["y", "dx"] + names, [y.detach()] + list(g)))


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", ["ico", "grid"])
@pytest.mark.parametrize("aggrs", AGGRS + [["mean", "var", "min"]], ids=ids)
def test_the_two_references_agree_in_float64(meshes, name, aggrs):
    ei, n = meshes[name]
    ref, x, t = _ref_and_inputs(ei, n, 5, 6, 2, aggrs, SCALERS[0], n)
    outs = []
    for form in ("edge", "dense"):
        ref.form = form
        outs.append(_grads(ref, x, ei, t, lambda m, x, ei: m(x, ei)))
    assert outs[0]["y"].shape == (n, 6)
    for k in outs[0]:
        e = err(outs[0][k], outs[1][k])
        assert e <= 1e-10, (k, e)


def test_duplicates_count_in_the_moments_and_not_in_max_and_min(meshes):
    from pna_ref import aggregate_edge_list
    ei, n = meshes["ico"]
    x = torch.randn(n, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    twice = torch.cat([ei, ei[:, :7]], 1)
    for k in ("max", "min"):
        assert torch.equal(aggregate_edge_list(x[ei[0]], ei, n, k), aggregate_edge_list(x[twice[0]], twice, n, k))
    for k in ("sum", "mean", "std", "var"):
        assert not torch.equal(aggregate_edge_list(x[ei[0]], ei, n, k), aggregate_edge_list(x[twice[0]], twice, n, k))


# ------------------------------------------------------------------------------------------------ the host side over the stub
def _guard_index_add(monkeypatch):
    """From here on ``index_add_`` / ``scatter*`` may only run inside the stub's functions (its stand-ins for a kernel's row loop):
    never in the product's host code.  (test_sage_cpu.py's trap.)"""
    inside = [0]
    for name in ("graph_for", "gather_moments", "gather_moments_bwd"):
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


def _host_run(monkeypatch, ei, n, cin, cout, towers, aggrs, scalers, seed):
    """(got, reference): {y, dx, every parameter's gradient by name} of the product's host code over the stub and of the edge-list
    reference, both in float64 on the same inputs and parameters."""
    from dual_dmp_amd import nn_ops
    ref, x, t = _ref_and_inputs(ei, n, cin, cout, towers, aggrs, scalers, seed)
    want = _grads(ref, x, ei, t, lambda m, x, ei: m(x, ei))
    monkeypatch.setattr(nn_ops, "ops", stub)
    _guard_index_add(monkeypatch)
    conv = nn_ops.PNAConv(cin, cout, aggrs, scalers, nn_ops.degree_histogram(ei, n), towers=towers).double()
    conv.load_state_dict(ref.state_dict())
    del stub.calls[:], stub.want_args[:], stub.wants[:]
    got = _grads(conv, x, ei, t, lambda m, x, ei: m._core(x, ei))
    return got, want


@pytest.mark.parametrize("cin,cout,towers", DIMS)
@pytest.mark.parametrize("aggrs", AGGRS, ids=ids)
@pytest.mark.parametrize("scalers", SCALERS, ids=ids)
def test_pna_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, cin, cout, towers, aggrs, scalers):
    ei, n = meshes["ico"]
    got, want = _host_run(monkeypatch, ei, n, cin, cout, towers, aggrs, scalers, cin * 7 + cout)
    # ONE gather launch per direction whatever the number of towers, aggregators and scalers; the GEMMs: pre, x W_x, one per
    # tower, lin -- and their wgrad + dgrad
    assert stub.calls.count("gather_moments") == 1 and stub.calls.count("gather_moments_bwd") == 1
    assert [stub.calls.count(k) for k in ("gemm_nt", "gemm_tn", "gemm_nn")] == [towers + 3] * 3
    assert stub.calls.index("gather_moments") == 2 and stub.calls[:2] == ["graph_for", "gemm_nt"]
    assert stub.wants == [tuple(aggrs)] and stub.want_args == [True]
    assert sorted(got) == sorted(want) and len(got) == 2 + 4 * towers + 2
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == torch.float64, k
        e = err(got[k], want[k])
        assert e <= HOST_TOL, (k, e)


def test_no_grad_forward_asks_for_no_arg(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    ei, n = meshes["grid"]
    conv = nn_ops.PNAConv(8, 8, ["mean", "max", "std"], ["identity", "linear"], nn_ops.degree_histogram(ei, n), towers=2)
    x = torch.randn(n, 8)
    del stub.calls[:], stub.want_args[:]
    with torch.no_grad():
        y0 = conv._core(x, ei)
    y1 = conv._core(x, ei)
    conv.requires_grad_(False)
    y2 = conv._core(x, ei)                                       # nothing requires a gradient
    y3 = conv._core(x.clone().requires_grad_(True), ei)
    assert stub.want_args == [False, True, False, True]
    assert not y0.requires_grad and y1.requires_grad and not y2.requires_grad and y3.requires_grad
    assert torch.equal(y0, y1) and torch.equal(y0, y2) and torch.equal(y0, y3)


def test_the_scaler_table_is_computed_once_per_graph(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    ei, n = meshes["grid"]
    g = stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    delta = deltas(degree_histogram(ei, n))
    a = nn_ops._pna_scaler_table(g, ei, n, ("identity", "amplification", "attenuation", "linear", "inverse_linear"), delta, torch.float64)
    b = nn_ops._pna_scaler_table(g, ei, n, ("identity", "amplification", "attenuation", "linear", "inverse_linear"), delta, torch.float64)
    assert a is b and a.shape == (n, 5)
    assert relerr(a, scaler_table(ei, n, ("identity", "amplification", "attenuation", "linear", "inverse_linear"), delta)) <= 1e-14
    assert float(a[n - 1, 3]) == 1.0 / delta[0]                  # the edgeless node: d = max(0, 1) = 1


def test_the_edgeless_the_pendant_and_the_one_source_node(meshes, monkeypatch):
    """The edgeless node gets post(cat[x_i, 0]); the pendant node (degree 1) and the node whose three edges all come from node 1
    have std = var = 0 exactly and no gradient flows through them."""
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    ei, n = meshes["ico"]
    pend, same, iso = n - 3, n - 2, n - 1
    g = stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    b, r = torch.randn(n, 8) + 5.0, torch.randn(n, 8)
    for moment in ("std", "var"):
        (s, mx, mn, v), (_, amx, amn, _), invdeg, mu = stub.gather_moments(g, b, want=("mean", "max", "min", moment), root=r)
        assert all(bool((t[iso] == 0).all()) for t in (s, mx, mn, v, mu)) and bool((amx[iso] == -1).all()) and bool((amn[iso] == -1).all())
        assert float(invdeg[iso]) == 0.0 and float(invdeg[pend]) == 1.0 and float(invdeg[same]) == float(torch.tensor(1.0) / 3.0)
        assert bool((v[pend] == 0).all()) and bool((v[same] == 0).all()) and float(v[:pend].min()) > 0
        assert torch.equal(mu[pend], b[0]) and relerr(mu[same], b[1]) <= 1e-7 and torch.equal(mx[pend], b[0] + r[pend])
    for aggrs in (["std"], ["var"], ["mean", "std"]):
        conv = nn_ops.PNAConv(4, 4, aggrs, ["identity", "amplification"], nn_ops.degree_histogram(ei, n)).double()
        x = torch.randn(n, 4, dtype=torch.float64, requires_grad=True)
        y = conv._core(x, ei)
        p = conv.post_nns[0][0]
        want = x[iso].detach() @ p.weight.detach()[:, :4].t() + p.bias.detach()
        assert relerr(y[iso], want @ conv.lin.weight.detach().t() + conv.lin.bias.detach()) <= 1e-12
        dy = torch.zeros(n, 4, dtype=torch.float64)
        dy[[pend, same, iso]] = 1000.0
        dx, = torch.autograd.grad(y, [x], dy)
        if aggrs != ["mean", "std"]:                             # std = var = 0 there: only the x columns of the post weight carry a gradient
            keep = torch.ones(n, dtype=torch.bool)
            keep[[pend, same, iso]] = False
            if aggrs == ["std"]:
                assert bool((dx[keep] == 0).all())               # G = 0 at std = 0: nothing at all flows
            else:                                                # var: 2 dVar (B[j] - mu) with mu = B[j] up to float64 rounding
                assert float(dx[keep].abs().max()) <= 1e-9
            root = dy @ conv.lin.weight.detach() @ p.weight.detach()[:, :4]
            assert relerr(dx[[pend, same, iso]], root[[pend, same, iso]]) <= 1e-12


# ------------------------------------------------------------------------------------------------ the module
def test_parameter_names_shapes_and_state_dict(meshes):
    from dual_dmp_amd.nn_ops import PNAConv
    deg = torch.tensor([0, 3, 5, 2])
    conv = PNAConv(6, 8, ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"], deg, towers=2)
    keys = ["pre_nns.0.0.weight", "pre_nns.0.0.bias", "pre_nns.1.0.weight", "pre_nns.1.0.bias", "post_nns.0.0.weight",
            "post_nns.0.0.bias", "post_nns.1.0.weight", "post_nns.1.0.bias", "lin.weight", "lin.bias"]
    assert list(conv.state_dict()) == keys
    assert [tuple(v.shape) for v in conv.state_dict().values()] == [(6, 12), (6,), (6, 12), (6,), (4, 78), (4,), (4, 78), (4,), (8, 8), (8,)]
    ref = PNAConvRef(6, 8, ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"], deg, towers=2)
    assert list(ref.state_dict()) == keys
    assert [tuple(v.shape) for v in ref.state_dict().values()] == [tuple(v.shape) for v in conv.state_dict().values()]
    assert (conv.in_channels, conv.out_channels, conv.towers, conv.F_in, conv.F_out) == (6, 8, 2, 6, 4)
    torch.manual_seed(0)
    conv = PNAConv(16, 400, ["mean"], ["identity"], deg)         # uniform(+-1/sqrt(fan-in))
    for p, fan in ((conv.pre_nns[0][0].weight, 32), (conv.post_nns[0][0].weight, 32), (conv.lin.weight, 400), (conv.lin.bias, 400)):
        top = float(p.detach().abs().max())
        assert 0.9 * fan ** -0.5 < top <= fan ** -0.5


def test_degree_histogram_and_the_deltas_on_a_hand_checked_graph():
    from dual_dmp_amd.nn_ops import PNAConv, degree_histogram as hist
    # in-degrees: node 0 <- 1, 2, 2 (a duplicate) = 3; node 1 <- 0 = 1; node 2 <- 0, 0 = 2; node 3 = 0
    ei = torch.tensor([[1, 2, 2, 0, 0, 0], [0, 0, 0, 1, 2, 2]])
    h = hist(ei, 4)
    assert h.dtype == torch.int64 and h.tolist() == [1, 1, 1, 1] and degree_histogram(ei, 4).tolist() == [1, 1, 1, 1]
    conv = PNAConv(4, 4, ["mean"], ["identity"], h)
    import math
    assert abs(conv.avg_deg["lin"] - (0 + 1 + 2 + 3) / 4) <= 1e-15
    assert abs(conv.avg_deg["log"] - (math.log(1) + math.log(2) + math.log(3) + math.log(4)) / 4) <= 1e-15
    assert deltas(h) == (conv.avg_deg["lin"], conv.avg_deg["log"])
    sc = scaler_table(ei, 4, ["amplification", "attenuation", "linear", "inverse_linear"], deltas(h))
    d = torch.tensor([3.0, 1.0, 2.0, 1.0], dtype=torch.float64)  # the edgeless node counts as degree 1
    assert relerr(sc[:, 0], torch.log(d + 1) / conv.avg_deg["log"]) <= 1e-15 and relerr(sc[:, 3], 1.5 / d) <= 1e-15
    assert relerr(sc[:, 0] * sc[:, 1], torch.ones(4)) <= 1e-15 and relerr(sc[:, 2] * sc[:, 3], torch.ones(4)) <= 1e-15


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import PNAConv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    deg = torch.tensor([0, 3, 5, 2])
    ok = dict(aggregators=["mean", "std"], scalers=["identity"], deg=deg)
    for kw in (dict(edge_dim=3), dict(pre_layers=2), dict(post_layers=2), dict(divide_input=True), dict(towers=3), dict(towers=0),
               dict(aggregators=["median"]), dict(aggregators=["mean", "lstm"]), dict(aggregators=[]), dict(aggregators="mean"),
               dict(aggregators=["max", "max"]), dict(aggregators=["mean", "sum"]), dict(aggregators=["std", "var"]),
               dict(aggregators=["add"]), dict(scalers=[]), dict(scalers=["exponential"]), dict(scalers=["identity", "identity"]),
               dict(scalers=None), dict(deg=torch.zeros(4)), dict(deg=None)):
        with pytest.raises(ValueError):
            PNAConv(4, 8, **{**ok, **kw})
    with pytest.raises(ValueError):
        PNAConv((4, 4), 8, **ok)
    with pytest.raises(TypeError):
        PNAConv(4, 8, flow="target_to_source", **ok)
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    conv = PNAConv(4, 8, towers=2, **ok)
    with pytest.raises(ValueError):
        conv((x, x), ei)
    with pytest.raises(ValueError):
        conv(x, ei, edge_attr=torch.randn(2, 3))
    with pytest.raises(ValueError):
        conv(x.to(torch.bfloat16), ei)
    with pytest.raises(ValueError):
        conv(torch.randn(6, 5), ei)
    with pytest.raises(ValueError):
        conv(torch.randn(6), ei)
    with pytest.raises(ValueError):
        conv(x, ei)                                              # a CPU x: no CPU fallback


def test_a_non_symmetric_structure_is_refused_by_the_graph(monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    conv = nn_ops.PNAConv(4, 8, ["mean"], ["identity"], torch.tensor([0, 2, 1]))
    del stub.calls[:]
    with pytest.raises(ValueError):
        conv._core(torch.randn(3, 4), torch.tensor([[0, 1, 2], [1, 0, 0]]))
    assert stub.calls == ["graph_for"]


def test_ops_want_is_checked():
    from dual_dmp_amd import ops
    assert ops._moments_want("std") == ("std",) and ops._moments_want(["sum", "min", "var"]) == ("sum", "min", "var")
    for bad in ((), ("mean", "sum"), ("std", "var"), ("max", "max"), ("add",), ("median",)):
        with pytest.raises(ops.DdmpError):
            ops._moments_want(bad)
    assert ops._stats_want("max") == ("max",)                    # gather_stats keeps refusing the second moment
    for bad in (("std",), ("var",), ("mean", "std")):
        with pytest.raises(ops.DdmpError):
            ops._stats_want(bad)


# ------------------------------------------------------------------------------------------------ the header
def test_header_declares_the_two_entry_points_and_abi_3():
    from dual_dmp_amd import _lib
    src = open(_lib.HEADER).read()
    assert re.search(r"#define\s+DDMP_ABI_VERSION\s+3\b", src)
    protos = _lib.parse_header()
    assert "ddmp_gather_moments_f32" in protos and "ddmp_gather_moments_bwd_f32" in protos
    names = [a for _, a in protos["ddmp_gather_moments_f32"][1]]
    assert names == ["g", "B", "ldb", "C", "mean", "as_std", "R", "ldr", "tw", "tstride", "S", "lds", "Mx", "ldmx", "argmx", "ldamx",
                     "Mn", "ldmn", "argmn", "ldamn", "V", "ldv", "mu", "ldmu", "invdeg", "stream"]
    names = [a for _, a in protos["ddmp_gather_moments_bwd_f32"][1]]
    assert names == ["g", "C", "dS", "ldds", "dQ", "lddq", "B", "ldb", "invdeg", "dMx", "lddmx", "argmx", "ldamx", "dMn",
                     "lddmn", "argmn", "ldamn", "dB", "lddb", "stream"]
    assert os.path.exists(os.path.join(_lib.CSRC, "pna.hip"))

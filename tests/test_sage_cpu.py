"""SAGEConv: everything that can be checked without a GPU -- the two float64 references against each other, the host side of
``nn_ops._SAGEConvFn`` over torch restatements of the kernels (tests/sage_ops_stub.py) in both GEMM orders with their launch
counts, the tie rule, the edgeless node, ``normalize``, ``root_weight=False`` / ``bias=False``, parameter names, the refusals, and
the public header."""
import os
import re

import pytest
import torch

import sage_ops_stub as stub
from sage_ref import SAGEConvRef, aggregate_dense, aggregate_edge_list, canonical, extremum_winners, sage_forward
from test_edgeconv_cpu import _with_extras, relerr

AGGRS = ["mean", "add", "max", "min", ["mean", "max"], ["add", "max", "min"]]
ids = lambda a: a if isinstance(a, str) else "+".join(a)


@pytest.fixture(scope="module")
def meshes():
    """name -> (edge_index, n): test_edgeconv_cpu.py's recipe -- the small icosphere and the open grid with duplicates and two
    loops on node 5 on top; n counts one more node than the mesh has: the last node has no edge at all."""
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    for name, (v, f) in (("ico", synth.icosphere(2)), ("grid", synth.open_grid(9, 7))):
        e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
        out[name] = (_with_extras(torch.cat([e, e[[1, 0]]], 1)), len(v) + 1)
    return out


def _params(cin, cout, k, seed, bias=True, root=True):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=gen, dtype=torch.float64) * 0.5).requires_grad_(True)
    return r(cout, k * cin), (r(cout) if bias else None), (r(cout, cin) if root else None)


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", ["ico", "grid"])
@pytest.mark.parametrize("aggr", AGGRS, ids=ids)
def test_the_two_references_agree_in_float64(meshes, name, aggr):
    ei, n = meshes[name]
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64, requires_grad=True)
    t = torch.randn(n, 4, generator=gen, dtype=torch.float64)
    wl, bl, wr = _params(5, 4, len(canonical(aggr)), 3)
    outs, grads = [], []
    for form in (aggregate_edge_list, aggregate_dense):
        y = sage_forward(x, ei, aggr, wl, bl, wr, form=form)
        outs.append(y)
        grads.append(torch.autograd.grad((y * t).sum(), [x, wl, bl, wr]))
    assert outs[0].shape == (n, 4) and relerr(outs[0], outs[1]) <= 1e-12
    for form in (aggregate_edge_list, aggregate_dense):                                  # the edgeless node aggregates to 0
        assert all(bool((form(x.detach(), ei, k)[n - 1] == 0).all()) for k in canonical(aggr))
    for a, b in zip(*grads):
        assert relerr(a, b) <= 1e-12, relerr(a, b)


def test_duplicates_count_in_mean_and_add_and_not_in_max_and_min(meshes):
    ei, n = meshes["ico"]
    x = torch.randn(n, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    twice = torch.cat([ei, ei[:, :7]], 1)
    for k in ("max", "min"):
        assert torch.equal(aggregate_edge_list(x, ei, k), aggregate_edge_list(x, twice, k))
    for k in ("add", "mean"):
        assert not torch.equal(aggregate_edge_list(x, ei, k), aggregate_edge_list(x, twice, k))
    deg5 = int((ei[1] == 5).sum())                               # two explicit loops on node 5: ordinary edges
    assert int(((ei[0] == 5) & (ei[1] == 5)).sum()) == 2
    assert relerr(aggregate_edge_list(x, ei, "mean")[5], x[ei[0][ei[1] == 5]].sum(0) / deg5) <= 1e-14


# ------------------------------------------------------------------------------------------------ the host side over the stub
CASES = [(3, 3), (16, 4), (5, 6), (8, 8), (12, 5)]              # (16, 4), (12, 5): transform-first for a single mean / add


def _transform_first(aggr, cin, cout):
    return isinstance(aggr, str) and aggr in ("mean", "add") and (cout + 3) // 4 < (cin + 3) // 4


def _guard_index_add(monkeypatch):
    """From here on ``index_add_`` / ``scatter*`` may only run inside the stub's functions (its stand-ins for a kernel's row loop)
    or in the reference: never in the product's host code."""
    inside = [0]
    for name in ("graph_for", "gather_stats", "gather_stats_bwd"):
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


def _fn_run(monkeypatch, ei, n, aggr, cin, cout, seed, bias=True, root=True, normalize=False):
    """(got, reference): [y, dx, dW_l, (db), (dW_r)] of the product's host code over the stub in float32 and of the edge-list
    reference in float64, on the same inputs."""
    from dual_dmp_amd import nn_ops
    gen = torch.Generator().manual_seed(seed)
    x64 = torch.randn(n, cin, generator=gen, dtype=torch.float64)
    t = torch.randn(n, cout, generator=gen, dtype=torch.float64)
    p64 = [p for p in _params(cin, cout, len(canonical(aggr)), seed + 1, bias, root)]
    xr = x64.clone().requires_grad_(True)
    yr = sage_forward(xr, ei, aggr, *p64, normalize=normalize)
    ref = [yr] + list(torch.autograd.grad((yr * t).sum(), [xr] + [p for p in p64 if p is not None]))
    monkeypatch.setattr(nn_ops, "ops", stub)
    _guard_index_add(monkeypatch)
    conv = nn_ops.SAGEConv(cin, cout, aggr=aggr, normalize=normalize, root_weight=root, bias=bias)
    with torch.no_grad():
        conv.lin_l.weight.copy_(p64[0])
        if bias:
            conv.lin_l.bias.copy_(p64[1])
        if root:
            conv.lin_r.weight.copy_(p64[2])
    x = x64.float().requires_grad_(True)
    del stub.calls[:], stub.want_args[:], stub.wants[:]
    y = conv._core(x, ei)
    got = [y] + list(torch.autograd.grad((y * t.float()).sum(), [x] + list(conv.parameters())))
    return got, ref


@pytest.mark.parametrize("cin,cout", CASES)
@pytest.mark.parametrize("aggr", AGGRS, ids=ids)
def test_sage_fn_over_the_stub_equals_the_reference(meshes, monkeypatch, aggr, cin, cout):
    ei, n = meshes["ico"]
    got, ref = _fn_run(monkeypatch, ei, n, aggr, cin, cout, cin * 7 + cout)
    if _transform_first(aggr, cin, cout):                       # ONE packed GEMM, ONE launch; ONE launch, wgrad, dgrad
        assert stub.calls == ["graph_for", "gemm_nt", "gather_stats", "gather_stats_bwd", "gemm_tn", "gemm_nn"]
    else:                                                       # ONE launch, ONE GEMM; wgrad, dgrad, ONE launch
        assert stub.calls == ["graph_for", "gather_stats", "gemm_nt", "gemm_tn", "gemm_nn", "gather_stats_bwd"]
    assert stub.wants == [canonical(aggr)] and len(got) == len(ref) == 5
    for a, b, nm in zip(got, ref, ("y", "dx", "dW_l", "db", "dW_r")):
        assert a.shape == b.shape and a.dtype == torch.float32, nm
        assert relerr(a, b) <= 1e-5, (nm, relerr(a, b))


def test_both_gemm_orders_occur():
    assert _transform_first("mean", 16, 4) and _transform_first("add", 12, 5) and not _transform_first("mean", 8, 8)
    assert not _transform_first("max", 16, 4) and not _transform_first(["mean", "max"], 16, 4) and not _transform_first("mean", 5, 6)


@pytest.mark.parametrize("aggr", ["mean", "max", ["add", "max", "min"]], ids=ids)
@pytest.mark.parametrize("bias,root", [(True, False), (False, True), (False, False)])
@pytest.mark.parametrize("cin,cout", [(5, 6), (16, 4)])
def test_root_weight_false_and_bias_false(meshes, monkeypatch, aggr, bias, root, cin, cout):
    ei, n = meshes["grid"]
    got, ref = _fn_run(monkeypatch, ei, n, aggr, cin, cout, 31, bias=bias, root=root)
    assert len(got) == len(ref) == 3 + bias + root
    assert stub.calls.count("gather_stats") == 1 and stub.calls.count("gather_stats_bwd") == 1
    assert [stub.calls.count(k) for k in ("gemm_nt", "gemm_tn", "gemm_nn")] == [1, 1, 1]
    for a, b in zip(got, ref):
        assert a.shape == b.shape and relerr(a, b) <= 1e-5, relerr(a, b)


@pytest.mark.parametrize("aggr", ["mean", ["mean", "max"]], ids=ids)
def test_normalize(meshes, monkeypatch, aggr):
    ei, n = meshes["grid"]
    got, ref = _fn_run(monkeypatch, ei, n, aggr, 5, 6, 17, normalize=True)
    assert relerr(got[0].norm(dim=1), torch.ones(n)) <= 1e-6
    for a, b in zip(got, ref):
        assert a.shape == b.shape and relerr(a, b) <= 1e-5, relerr(a, b)


def test_no_grad_forward_asks_for_no_arg(meshes, monkeypatch):
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    ei, n = meshes["grid"]
    conv = nn_ops.SAGEConv(5, 6, aggr=["mean", "max"])
    x = torch.randn(n, 5)
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


def test_ties_go_to_the_smallest_source_id(meshes):
    """All rows of x equal: every entry of a row ties in max and in min; the whole of the gradient lands on the row's smallest
    neighbour id."""
    ei, n = meshes["ico"]
    g = stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    gen = torch.Generator().manual_seed(1)
    C = 6
    x = torch.randn(1, C, generator=gen).expand(n, C).contiguous()
    dmx, dmn = torch.randn(n, C, generator=gen), torch.randn(n, C, generator=gen)
    (mx, mn), (amx, amn), invdeg = stub.gather_stats(g, x, want=("max", "min"))
    nonempty = g.rowptr[1:] > g.rowptr[:-1]
    assert int(nonempty.sum()) == n - 1 and invdeg is None
    first = g.col[g.rowptr[:-1].clamp(max=g.nnz - 1)]            # CSR columns ascend: a row's first entry is its smallest id
    for v, a in ((mx, amx), (mn, amn)):
        assert torch.equal(v[nonempty], x[nonempty])
        assert torch.equal(a[nonempty].long(), first[nonempty].view(-1, 1).expand(-1, C))
    ref_arg, gap, empty = extremum_winners(x.double(), ei, n, "min")
    assert torch.equal(ref_arg, amn.long()) and bool((gap[~empty] == 0).all())
    dx, dr = stub.gather_stats_bwd(g, dmx=dmx, argmx=amx, dmn=dmn, argmn=amn)
    want = torch.zeros((n, C), dtype=torch.float64).index_add_(0, first[nonempty], (dmx + dmn)[nonempty].double())
    assert dr is None and relerr(dx, want) <= 1e-6


def test_the_edgeless_node(meshes, monkeypatch):
    """It aggregates to 0 in every statistic, so its output is lin_r(x_i) + bias, and it receives a gradient through the root only."""
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    ei, n = meshes["ico"]
    for aggr, cin, cout in (("mean", 5, 8), ("mean", 16, 4), (["add", "max", "min"], 5, 8)):
        conv = nn_ops.SAGEConv(cin, cout, aggr=aggr)
        x = torch.randn(n, cin, requires_grad=True)
        y = conv._core(x, ei)
        want = x[n - 1].detach().double() @ conv.lin_r.weight.detach().double().t() + conv.lin_l.bias.detach().double()
        assert relerr(y[n - 1], want) <= 1e-6
        dy = torch.zeros(n, cout)
        dy[n - 1] = 1000.0
        dx, = torch.autograd.grad(y, [x], dy)
        assert relerr(dx[n - 1], dy[n - 1].double() @ conv.lin_r.weight.detach().double()) <= 1e-6
        assert bool((dx[:n - 1] == 0).all())                     # nobody gathers from it, it gathers from nobody
    g = stub.graph_for(ei, n, norm="gat", add_self_loops=False)
    (s, mx, mn), (_, amx, amn), invdeg = stub.gather_stats(g, torch.randn(n, 8) + 5.0, want=("mean", "max", "min"))
    assert all(bool((v[n - 1] == 0).all()) for v in (s, mx, mn)) and bool((amx[n - 1] == -1).all()) and bool((amn[n - 1] == -1).all())
    assert float(invdeg[n - 1]) == 0.0 and float(invdeg[:n - 1].min()) > 0


# ------------------------------------------------------------------------------------------------ the module
def test_parameter_names_shapes_and_state_dict():
    from dual_dmp_amd.nn_ops import SAGEConv
    conv = SAGEConv(5, 7)
    assert list(conv.state_dict()) == ["lin_l.weight", "lin_l.bias", "lin_r.weight"]
    assert [tuple(v.shape) for v in conv.state_dict().values()] == [(7, 5), (7,), (7, 5)]
    assert (conv.in_channels, conv.out_channels, conv.aggr, conv.normalize, conv.root_weight, conv.project) == (5, 7, "mean", False, True, False)
    conv = SAGEConv(5, 7, aggr=["mean", "max", "min"], root_weight=False)
    assert list(conv.state_dict()) == ["lin_l.weight", "lin_l.bias"] and conv.lin_l.weight.shape == (7, 15) and not hasattr(conv, "lin_r")
    conv = SAGEConv(5, 7, aggr="sum", bias=False)
    assert list(conv.state_dict()) == ["lin_l.weight", "lin_r.weight"] and conv.lin_l.bias is None
    for aggr in AGGRS:
        ref, conv = SAGEConvRef(5, 7, aggr), SAGEConv(5, 7, aggr=aggr)
        assert list(ref.state_dict()) == list(conv.state_dict())
        assert [tuple(v.shape) for v in ref.state_dict().values()] == [tuple(v.shape) for v in conv.state_dict().values()]
    torch.manual_seed(0)
    conv = SAGEConv(16, 400, aggr=["mean", "max"])              # uniform(+-1/sqrt(fan-in)): 32 for lin_l (bias included), 16 for lin_r
    for p, fan in ((conv.lin_l.weight, 32), (conv.lin_l.bias, 32), (conv.lin_r.weight, 16)):
        top = float(p.detach().abs().max())
        assert 0.9 * fan ** -0.5 < top <= fan ** -0.5


def test_every_refusal_raises_before_any_library_call(monkeypatch):
    from dual_dmp_amd import nn_ops, ops
    from dual_dmp_amd.nn_ops import SAGEConv

    class Trap:
        DdmpError = ops.DdmpError

        def __getattr__(self, name):
            raise AssertionError("ops.%s reached before the refusal" % name)

    monkeypatch.setattr(nn_ops, "ops", Trap())
    with pytest.raises(ValueError):
        SAGEConv(4, 8, project=True)
    for aggr in ("lstm", "std", "var", "median", "mul", "softmax", None, 3, [], ["mean", "lstm"], ["max", "std"],
                 ["mean", "add"], ["sum", "mean"], ["add", "sum"], ["max", "max"], ["mean", "max", "mean"]):
        with pytest.raises(ValueError):
            SAGEConv(4, 8, aggr=aggr)
    with pytest.raises(ValueError):
        SAGEConv((4, 4), 8)
    with pytest.raises(TypeError):
        SAGEConv(4, 8, flow="target_to_source")
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1], [1, 0]])
    conv = SAGEConv(4, 8, aggr=["mean", "max"])
    with pytest.raises(ValueError):
        conv((x, x), ei)
    with pytest.raises(ValueError):
        conv(x, ei, size=(6, 6))
    with pytest.raises(ValueError):
        conv(x.to(torch.bfloat16), ei)
    with pytest.raises(ValueError):
        conv(torch.randn(6, 5), ei)
    with pytest.raises(ValueError):
        conv(torch.randn(6), ei)
    with pytest.raises(ValueError):
        conv(x, ei)                                              # a CPU x: no CPU fallback


def test_a_non_symmetric_structure_is_refused_by_the_graph(monkeypatch):
    """The backward reads row j's own entries as the rows j feeds: the valued graph refuses a one-directional edge."""
    from dual_dmp_amd import nn_ops
    monkeypatch.setattr(nn_ops, "ops", stub)
    conv = nn_ops.SAGEConv(4, 8)
    del stub.calls[:]
    with pytest.raises(ValueError):
        conv._core(torch.randn(3, 4), torch.tensor([[0, 1, 2], [1, 0, 0]]))
    assert stub.calls == ["graph_for"]


def test_ops_want_is_checked():
    from dual_dmp_amd import ops
    assert ops._stats_want("max") == ("max",) and ops._stats_want(["add", "min"]) == ("add", "min")
    for bad in ((), ("mean", "add"), ("max", "max"), ("sum",), ("std",)):
        with pytest.raises(ops.DdmpError):
            ops._stats_want(bad)


# ------------------------------------------------------------------------------------------------ the header
def test_header_declares_the_two_entry_points_and_abi_3():
    from dual_dmp_amd import _lib
    src = open(_lib.HEADER).read()
    assert re.search(r"#define\s+DDMP_ABI_VERSION\s+3\b", src)
    protos = _lib.parse_header()
    assert "ddmp_gather_stats_f32" in protos and "ddmp_gather_stats_bwd_f32" in protos
    names = [a for _, a in protos["ddmp_gather_stats_f32"][1]]
    assert names == ["g", "X", "ldx", "C", "mean", "R", "ldr", "bias", "S", "lds", "Mx", "ldmx", "argmx", "ldamx", "Mn", "ldmn",
                     "argmn", "ldamn", "invdeg", "Xcopy", "ldxc", "stream"]
    names = [a for _, a in protos["ddmp_gather_stats_bwd_f32"][1]]
    assert names == ["g", "C", "dS", "ldds", "invdeg", "dMx", "lddmx", "argmx", "ldamx", "dMn", "lddmn", "argmn", "ldamn", "dX0",
                     "lddx0", "dX", "lddx", "dR", "lddr", "stream"]
    assert os.path.exists(os.path.join(_lib.CSRC, "nstat.hip"))

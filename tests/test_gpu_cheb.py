"""The Chebyshev path on the GPU: the fused step kernel (``ops.spmm_axpby``) on every route, the ``ChebConv`` drop-in
(forward, dX, every dW_k, dbias) and the modular nets built from it, against the dense float64 restatement of
``tests/cheb_ref.py``.

Tolerances: the gather tolerance of ``test_spmm_matches_dense`` (rel-L2 < 1e-6) for the kernel, the operator tolerance of
``test_gcnconv_dropin_matches_oracle`` (rel-L2 < 1e-5) for ChebConv -- or, where the reference formula's OWN float32 run on the
CPU is farther than that from its float64 run, four times that distance (the GEMM is split-precision f32-class, not bit-exact
f32, and the contraction is K times longer than GCNConv's) --, and the bounds of ``test_nets_forward_backward_match_oracle``
for the nets."""
import copy

import pytest
import torch

import oracle_jobs as OJ
from cheb_ref import ChebConvRef, axpby_ref, dense_s

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graphs(dev):
    """The four graphs of tests/test_gpu_kernels.py's fixture, with norm="sym": (device edge_index, n, dense float64 S)."""
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    for name, (v, f) in {"ico3": synth.icosphere(3), "grid": synth.open_grid(9, 7)}.items():
        v, f = synth.permute_vertices(v, f, 1)
        m = Mesh(vs=v, faces=f)
        e = torch.tensor(m.edges.T, dtype=torch.long)
        ei = torch.cat([e, e[[1, 0]]], 1)
        fi = torch.from_numpy(m.f_edges)
        out[name + "_v"] = (ei.to(dev), len(v), dense_s(ei, len(v)))
        out[name + "_f"] = (fi.to(dev), len(f), dense_s(fi, len(f)))
    return out


def _variants(g, S, n, C, dev, seed):
    """-> [(name, result of ops.spmm_axpby, float64 reference)] for the forms the recurrences use."""
    from dual_dmp_amd import ops
    gen = torch.Generator().manual_seed(seed)
    x, z, z2 = (torch.randn(n, C, generator=gen) for _ in range(3))
    xd, zd, z2d = x.to(dev), z.to(dev), z2.to(dev)
    out = []
    out.append(("plain", ops.spmm_axpby(g, xd, a=0.7), axpby_ref(S, x, a=0.7)))
    out.append(("b", ops.spmm_axpby(g, xd, a=-1.0, b=0.3), axpby_ref(S, x, a=-1.0, b=0.3)))
    out.append(("one addend", ops.spmm_axpby(g, xd, z=zd, a=-2.0, b=0.25, c=-1.0), axpby_ref(S, x, z, a=-2.0, b=0.25, c=-1.0)))
    out.append(("two addends", ops.spmm_axpby(g, xd, z=zd, z2=z2d, a=-1.2, b=0.4, c=1.0, d=-1.0),
                axpby_ref(S, x, z, z2, a=-1.2, b=0.4, c=1.0, d=-1.0)))
    # a coefficient without its operand is ignored
    out.append(("ignored", ops.spmm_axpby(g, xd, z2=z2d, a=0.5, c=float("nan"), d=2.0), axpby_ref(S, x, None, z2, a=0.5, d=2.0)))
    y = zd.clone()                                               # Y aliases Z
    r = ops.spmm_axpby(g, xd, out=y, z=y, z2=z2d, a=-1.2, b=0.4, c=1.0, d=-1.0)
    assert r.data_ptr() == y.data_ptr()
    out.append(("in place", y, axpby_ref(S, x, z, z2, a=-1.2, b=0.4, c=1.0, d=-1.0)))
    y2 = z2d.clone()                                             # Y aliases Z2
    ops.spmm_axpby(g, xd, out=y2, z=zd, z2=y2, a=0.3, c=0.5, d=-1.0)
    out.append(("in place 2", y2, axpby_ref(S, x, z, z2, a=0.3, c=0.5, d=-1.0)))
    # column blocks of ONE wider buffer (ldx = ldy = ldz = 3 C): block 2 = step(block 1, block 0), as ChebConv lays T out
    wide = torch.randn(n, 3 * C, generator=gen)
    wd = wide.to(dev)
    ops.spmm_axpby(g, wd[:, C:2 * C], out=wd[:, 2 * C:], z=wd[:, :C], a=-2.0, b=0.5, c=-1.0)
    assert torch.equal(wd[:, :2 * C].cpu(), wide[:, :2 * C])     # the other blocks are untouched
    out.append(("strided", wd[:, 2 * C:], axpby_ref(S, wide[:, C:2 * C], wide[:, :C], a=-2.0, b=0.5, c=-1.0)))
    return out


@pytest.mark.parametrize("C", [8, 16, 32, 64, 128, 256, 512, 3, 20])
@pytest.mark.parametrize("gname", ["ico3_v", "ico3_f", "grid_v", "grid_f"])
def test_spmm_axpby_matches_dense(dev, graphs, C, gname):
    from dual_dmp_amd import ops
    ei, n, S = graphs[gname]
    g = ops.graph_for(ei, n, norm="sym")
    assert (g.n_rows, g.n_cols, g.nnz) == (n, n, ei.shape[1])
    assert ops.graph_for(ei, n, norm="sym") is g and ops.graph_for(ei, n) is not g       # cached per (tensor, norm)
    assert ops.graph_for(ei, n).nnz == ei.shape[1] + n
    for name, got, ref in _variants(g, S, n, C, dev, C):
        err = relerr(got, ref)
        print("spmm_axpby %s C=%d %s: rel-L2 %.2e" % (gname, C, name, err))
        assert err < 1e-6, (name, err)


@pytest.mark.parametrize("C", [3, 8, 32, 96])
def test_spmm_axpby_isolated_nodes_multi_edges_self_loops(dev, graphs, C):
    """Rows without entries (dinv = 0: the row is b X + c Z + d Z2), a doubled edge and explicit self loops (dropped), on
    the scalar, row, and lean kernels; the isolated nodes sit inside a chunk and fill the last one."""
    from dual_dmp_amd import ops
    ei0, n0, _ = graphs["grid_v"]
    ei0 = ei0.cpu()
    iso = torch.tensor([3, 17, 40])                              # cut every edge of three nodes
    keep = ~(torch.isin(ei0[0], iso) | torch.isin(ei0[1], iso))
    n = n0 + 70                                                  # + a whole chunk of isolated nodes behind the mesh
    dup = ei0[:, keep][:, :6]
    dup = torch.cat([dup, dup[[1, 0]]], 1)                       # six edges twice, both directions (stays symmetric)
    loops = torch.tensor([[0, 5, 17], [0, 5, 17]])
    ei = torch.cat([ei0[:, keep], dup, loops], 1)
    S = dense_s(ei, n)
    assert float(S.diagonal().abs().max()) == 0.0 and float(S[17].abs().max()) == 0.0 and float(S[n - 1].abs().max()) == 0.0
    assert float((S - S.T).abs().max()) == 0.0
    eid = ei.to(dev)
    g = ops.graph_for(eid, n, norm="sym")
    assert g.nnz == ei.shape[1] - 3
    for name, got, ref in _variants(g, S, n, C, dev, 100 + C):
        err = relerr(got, ref)
        print("spmm_axpby isolated C=%d %s: rel-L2 %.2e" % (C, name, err))
        assert err < 1e-6, (name, err)
        assert bool(torch.isfinite(got).all())
    x = torch.randn(n, C)
    y = ops.spmm_axpby(g, x.to(dev), a=1.0)
    assert float(y[17].abs().max()) == 0.0 and float(y[n0:].abs().max()) == 0.0          # exactly zero, not NaN
    # the plain gather takes such a graph too
    assert relerr(ops.spmm(g, x.to(dev)), S @ x.double()) < 1e-6


@pytest.mark.parametrize("C", [3, 16, 64, 512])
def test_spmm_axpby_is_bit_reproducible(dev, graphs, C):
    from dual_dmp_amd import ops
    ei, n, _ = graphs["ico3_v"]
    g = ops.graph_for(ei, n, norm="sym")
    torch.manual_seed(C)
    x, z, z2 = (torch.randn(n, C, device=dev) for _ in range(3))
    first = ops.spmm_axpby(g, x, z=z, z2=z2, a=-1.0, b=0.1, c=1.0, d=-1.0)
    for _ in range(3):
        assert torch.equal(ops.spmm_axpby(g, x, z=z, z2=z2, a=-1.0, b=0.1, c=1.0, d=-1.0), first)


def test_spmm_axpby_refuses_bad_arguments(dev, graphs):
    from dual_dmp_amd import ops
    ei, n, _ = graphs["grid_v"]
    g = ops.graph_for(ei, n, norm="sym")
    x = torch.randn(n, 8, device=dev)
    with pytest.raises(ops.DdmpError):
        ops.spmm_axpby(g, x, out=x)                              # Y must not alias X
    with pytest.raises(ops.DdmpError):
        ops.spmm_axpby(g, x, z=torch.randn(n, 4, device=dev), c=1.0)
    with pytest.raises(ops.DdmpError):
        ops.spmm_axpby(g, x.cpu())
    with pytest.raises(ops.DdmpError):
        ops.graph_for(ei, n, norm="rw")


def test_spmm_axpby_slab_route_agrees_bit_for_bit(dev, tmp_path):
    """C % 32 == 0 where the lean gather's 32-bit offsets do not reach runs ``spmm_slab_kernel``'s form of the epilogue: forced
    here with DDMP_SPMM_LEAN=0 in a process of its own (the switch is read once per process) -- the same sums in the same
    order and the same epilogue expression, so the same bits."""
    import os
    import subprocess
    import sys
    import numpy as np
    import cheb_route_worker as W
    out = str(tmp_path / "slab.npy")
    env = dict(os.environ, DDMP_SPMM_LEAN="0")
    r = subprocess.run([sys.executable, W.__file__, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert torch.equal(torch.from_numpy(np.load(out)), W.run(dev))


@pytest.fixture(scope="module")
def big(dev):
    """144,400-face torus in RCB order (as test_spmm_lds_patch_route_on_a_large_face_graph builds it): face and vertex edge lists."""
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    v, f = synth.rcb_relabel(*synth.torus(380, 190))
    m = Mesh(vs=v, faces=f)
    fi = torch.from_numpy(m.f_edges)
    e = torch.tensor(m.edges.T, dtype=torch.long)
    return (fi, len(f)), (torch.cat([e, e[[1, 0]]], 1), len(v))


def test_spmm_axpby_on_a_large_face_graph_matches_the_composition(dev, big):
    """A face graph large enough for the LDS-patch selection of the plain gather (144,400 faces, RCB order), C = 256, one
    addend: the fused step against ``ops.spmm`` + torch arithmetic on the same norm="sym" graph (rel-L2 < 1e-6), and on the
    vertex graph (6 entries per row)."""
    from dual_dmp_amd import ops, _lib
    L = _lib.lib()
    for ei, n in big:
        eid = ei.to(dev)
        g = ops.graph_for(eid, n, norm="sym")
        assert g.nnz == ei.shape[1]
        assert L.ddmp_spmm_patch_selected(g.handle, 256, 0, 0, 0) == 1      # the composition's gather runs the LDS-patch kernel
        torch.manual_seed(n)
        x, z = torch.randn(n, 256, device=dev), torch.randn(n, 256, device=dev)
        a, b, c = -2.0 / 1.7, 2.0 * (2.0 / 1.7 - 1.0), -1.0
        composed = a * ops.spmm(g, x) + b * x + c * z
        fused = ops.spmm_axpby(g, x, z=z, a=a, b=b, c=c)
        err = relerr(fused, composed)
        print("spmm_axpby large n=%d: rel-L2 against the composition %.2e" % (n, err))
        assert err < 1e-6
        y = z.clone()
        ops.spmm_axpby(g, x, out=y, z=y, a=a, b=b, c=c)
        assert torch.equal(y, fused)                             # in place = out of place, bit for bit


def test_empty_rows_on_a_graph_with_patch_tables(dev, big):
    """The patch-table builder and the LDS-patch gather with rows that have no entries -- scattered inside chunks and a whole
    64-row chunk of them (that chunk has no patch: it goes to the lean gather's list) -- on the 144,400-face graph with the edges
    of some faces cut: the plain gather at C = 256 (LDS-patch route) and the fused step against a float64 sparse product."""
    from dual_dmp_amd import ops, _lib
    (fi, n), _ = big
    iso = torch.cat([torch.arange(640, 704), torch.tensor([5, 70001, n - 1])])
    keep = ~(torch.isin(fi[0], iso) | torch.isin(fi[1], iso))
    ei = fi[:, keep].contiguous()
    g = ops.graph_for(ei.to(dev), n, norm="sym")
    assert g.nnz == ei.shape[1]
    L = _lib.lib()
    assert L.ddmp_spmm_patch_selected(g.handle, 256, 0, 0, 0) == 1
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], torch.ones(ei.shape[1], dtype=torch.float64))
    d = torch.where(deg > 0, deg.clamp(min=1.0).pow(-0.5), torch.zeros_like(deg))
    S = torch.sparse_coo_tensor(torch.stack([ei[1], ei[0]]), d[ei[1]] * d[ei[0]], size=(n, n)).coalesce()
    torch.manual_seed(7)
    x, z = torch.randn(n, 256), torch.randn(n, 256)
    sx = torch.sparse.mm(S, x.double())
    y = ops.spmm(g, x.to(dev))
    assert relerr(y, sx) < 1e-6
    assert float(y[640:704].abs().max()) == 0.0 and float(y[5].abs().max()) == 0.0 and float(y[n - 1].abs().max()) == 0.0
    fused = ops.spmm_axpby(g, x.to(dev), z=z.to(dev), a=-2.0, b=0.5, c=-1.0)
    assert relerr(fused, -2.0 * sx + 0.5 * x.double() - z.double()) < 1e-6
    assert torch.equal(fused[640:704].cpu(), (0.5 * x - z)[640:704])


def _run(conv, x, ei, dy, lambda_max):
    xr = x.clone().requires_grad_(True)
    y = conv(xr, ei, lambda_max=lambda_max)
    y.backward(dy)
    out = {"y": y.detach(), "dx": xr.grad, "dbias": conv.bias.grad}
    for k in range(conv.K):
        out["dW%d" % k] = conv.lins[k].weight.grad
    return out


CASES = [(16, 32, 3, None), (7, 32, 2, 1.7), (64, 32, 5, None), (512, 256, 3, 1.7), (512, 256, 5, None), (32, 3, 1, None),
         (32, 3, 4, 1.7), (5, 6, 5, 1.7), (5, 6, 1, 1.7)]


@pytest.mark.parametrize("mesh", ["grid", "flip"])
@pytest.mark.parametrize("cin,cout,K,lambda_max", CASES)
def test_chebconv_dropin_matches_float64_reference(dev, cin, cout, K, lambda_max, mesh):
    """Forward, dX, every dW_k and dbias from a loaded state_dict.  Bound per quantity: max(1e-5, 4 x the rel-L2 distance of
    the reference formula's own float32 CPU run from its float64 run) -- see the module docstring."""
    from dual_dmp_amd.nn_ops import ChebConv
    _, noisy, _, data = OJ.case(mesh)
    n = len(noisy.vs)
    torch.manual_seed(cin * cout + K)
    ref32 = ChebConvRef(cin, cout, K)
    with torch.no_grad():
        ref32.bias.normal_()
    ref64 = copy.deepcopy(ref32).double()
    ours = ChebConv(cin, cout, K).to(dev)
    assert sorted(n_ for n_, _ in ours.named_parameters()) == sorted(n_ for n_, _ in ref32.named_parameters())
    res = ours.load_state_dict(ref32.state_dict())
    assert list(res.missing_keys) == [] and list(res.unexpected_keys) == []
    x, dy = torch.randn(n, cin), torch.randn(n, cout)
    r64 = _run(ref64, x.double(), data.edge_index, dy.double(), lambda_max)
    r32 = _run(ref32, x, data.edge_index, dy, lambda_max)
    got = _run(ours, x.to(dev), data.edge_index.to(dev), dy.to(dev), lambda_max)
    assert got["y"].dtype == torch.float32 and tuple(got["dx"].shape) == (n, cin)
    bad = []
    for key, ref in r64.items():
        e32 = relerr(r32[key], ref)
        bound = max(1e-5, 4.0 * e32)
        err = relerr(got[key], ref)
        print("ChebConv %s (%d, %d) K=%d lambda_max=%s %s: rel-L2 %.2e (float32 reference %.2e, bound %.2e)"
              % (mesh, cin, cout, K, lambda_max, key, err, e32, bound))
        if not err < bound:
            bad.append((key, err, bound))
    assert not bad, bad


def test_chebconv_without_input_gradient_and_without_bias(dev):
    from dual_dmp_amd.nn_ops import ChebConv
    _, noisy, _, data = OJ.case("grid")
    n = len(noisy.vs)
    torch.manual_seed(1)
    ref = ChebConvRef(16, 8, 3, bias=False).double()
    ours = ChebConv(16, 8, 3, bias=False).to(dev)
    ours.load_state_dict(ref.state_dict())
    x, dy = torch.randn(n, 16), torch.randn(n, 8)
    yr = ref(x.double(), data.edge_index)
    yr.backward(dy.double())
    xo = x.to(dev)                                               # no gradient wanted: the Clenshaw chain is skipped
    yo = ours(xo, data.edge_index.to(dev))
    yo.backward(dy.to(dev))
    assert xo.grad is None and relerr(yo, yr) < 1e-5
    for k in range(3):
        assert relerr(ours.lins[k].weight.grad, ref.lins[k].weight.grad) < 1e-5


def _cheb_oracle_net(oracle, Ref, K):
    """oracle.PosNetRef / NormalNetRef with its twelve convs replaced by the test's ChebConv reference."""
    ref = Ref()
    for i in range(1, 13):
        old = getattr(ref, "conv%d" % i)
        setattr(ref, "conv%d" % i, ChebConvRef(old.lin.weight.shape[1], old.lin.weight.shape[0], K))
    return ref


def test_cheb_nets_forward_backward_match_float64_reference(dev, oracle):
    """PosNet / NormalNet(dev, fused=False, conv="cheb", K=3) on "ico3" against a float64 net; the bounds of
    test_nets_forward_backward_match_oracle (modular GCN net): forward rel-L2 < 1e-4, every parameter gradient < 5e-3, the conv
    biases left out (analytically zero behind BatchNorm)."""
    from dual_dmp_amd.networks import PosNet, NormalNet
    gt, noisy, smooth, data = OJ.case("ico3")
    odata = oracle.OracleDataset(noisy, smooth)
    for k in ("z1", "z2", "x_pos"):
        setattr(odata, k, getattr(odata, k).double())
    for Ref, Ours, n_out in ((oracle.PosNetRef, PosNet, len(noisy.vs)), (oracle.NormalNetRef, NormalNet, len(noisy.faces))):
        with pytest.raises(ValueError):
            Ours(dev, fused=True, conv="cheb")
        torch.manual_seed(5)
        ref = _cheb_oracle_net(oracle, Ref, 3)
        with torch.no_grad():
            for i in range(1, 13):
                getattr(ref, "conv%d" % i).bias.normal_(std=0.1)
                getattr(ref, "bn%d" % i).weight.uniform_(0.5, 1.5)
                getattr(ref, "bn%d" % i).bias.normal_(std=0.1)
        net = Ours(dev, fused=False, conv="cheb", K=3)
        res = net.load_state_dict(ref.state_dict())
        assert list(res.missing_keys) == [] and list(res.unexpected_keys) == []
        assert sum(p.numel() for p in net.parameters()) == sum(p.numel() for p in ref.parameters())
        ref.double()
        dout = torch.randn(n_out, 3)
        ref.train()
        o_ref = ref(odata)
        o_ref.backward(dout.double())
        net.train()
        o = net(data)
        o.backward(dout.to(dev))
        print("%s cheb K=3: forward rel-L2 %.2e" % (Ours.__name__, relerr(o, o_ref)))
        assert relerr(o, o_ref) < 1e-4, (Ours.__name__, relerr(o, o_ref))
        got = {n: p.grad for n, p in net.named_parameters()}
        worst = ("", 0.0)
        for n, p in ref.named_parameters():
            if n.startswith("conv") and n.endswith(".bias"):
                continue
            err = relerr(got[n], p.grad)
            worst = max(worst, (n, err), key=lambda t: t[1])
            assert err < 5e-3, (n, err)
        print("%s cheb K=3: worst parameter-gradient rel-L2 %.2e (%s)" % (Ours.__name__, worst[1], worst[0]))

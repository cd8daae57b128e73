"""ChebConv drop-in, the self-loop-free graph flavour and the fused Chebyshev-step entry point: everything that can be
checked without a GPU (parameter contract, exported symbols, argument checks before any device work, the host CSR builder,
and the unchanged default of the modular nets)."""
import ctypes
import math

import numpy as np
import pytest
import torch


def test_chebconv_parameter_contract():
    from dual_dmp_amd.nn_ops import ChebConv
    for K in (1, 3):
        torch.manual_seed(K)
        conv = ChebConv(7, 32, K)
        names = [n for n, _ in conv.named_parameters()]
        # (nn.Module lists a module's own parameters before its children's, in PyG as here: bias first)
        assert names == ["bias"] + ["lins.%d.weight" % k for k in range(K)], names
        assert list(conv.state_dict().keys()) == names
        a = math.sqrt(6.0 / (7 + 32))
        for k in range(K):
            w = conv.lins[k].weight.detach()
            assert tuple(w.shape) == (32, 7) and float(w.abs().max()) <= a and float(w.abs().max()) > 0.5 * a
        assert tuple(conv.bias.shape) == (32,) and float(conv.bias.detach().abs().max()) == 0.0
    assert ChebConv(4, 4, 2, bias=False).bias is None
    with pytest.raises(ValueError):
        ChebConv(7, 32, 0)
    with pytest.raises(ValueError):
        ChebConv(7, 32, 3, normalization="rw")


def test_chebconv_loads_a_pyg_shaped_state_dict_and_refuses_what_is_not_built():
    from dual_dmp_amd.nn_ops import ChebConv
    from dual_dmp_amd.ops import DdmpError
    from cheb_ref import ChebConvRef
    ref = ChebConvRef(5, 6, 3)
    conv = ChebConv(5, 6, 3)
    res = conv.load_state_dict(ref.state_dict())
    assert list(res.missing_keys) == [] and list(res.unexpected_keys) == []
    assert torch.equal(conv.lins[2].weight, ref.lins[2].weight)
    x = torch.randn(4, 5)
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    with pytest.raises(DdmpError):                               # no CPU fallback
        conv(x, ei)
    with pytest.raises(ValueError):
        conv(x, ei, torch.ones(4))                               # edge_weight
    with pytest.raises(ValueError):
        conv(x, ei, batch=torch.zeros(4, dtype=torch.long))
    with pytest.raises(ValueError):
        conv(x, ei, lambda_max=torch.tensor(2.0))


def test_header_declares_and_library_exports_the_new_entry_points():
    from dual_dmp_amd import _lib
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in ("ddmp_spmm_axpby_f32", "ddmp_csr_build_sym_host", "ddmp_graph_create_sym"):
        assert name in protos, name
        assert hasattr(L, name), name
    assert len(protos["ddmp_spmm_axpby_f32"][1]) == 15
    assert L.ddmp_abi_version() == 3
    # argument checks come before any device work: no GPU is needed to be refused
    buf = (ctypes.c_float * 64)()
    other = (ctypes.c_float * 64)()
    fake_graph = (ctypes.c_char * 256)()                         # never dereferenced: the checks below fail first
    p, q, g = ctypes.addressof(buf), ctypes.addressof(other), ctypes.addressof(fake_graph)
    call = lambda g_, x, y, C=8, ldx=8, ldy=8, z=None, ldz=0: L.ddmp_spmm_axpby_f32(g_, x, ldx, y, ldy, z, ldz, None, 0, C, 1.0,
                                                                                 0.0, 0.0, 0.0, None)
    assert call(None, p, q) == -1
    assert call(g, None, q) == -1
    assert call(g, p, None) == -1
    assert call(g, p, p) == -1                                   # X == Y
    assert call(g, p, q, C=0) == -1
    assert call(g, p, q, C=8, ldx=4) == -1
    assert call(g, p, q, z=p, ldz=4) == -1                       # an addend narrower than C
    out = ctypes.c_void_p()
    assert L.ddmp_graph_create_sym(0, 0, None, 0, ctypes.byref(out)) == -1
    assert L.ddmp_graph_create_sym(4, 2, None, 0, ctypes.byref(out)) == -1


def test_sym_csr_builder_multiplicity_self_loop_isolated_node():
    from dual_dmp_amd import ops
    # 5 nodes: edge 0-1 twice (both directions each), 1-2, 2-3, an explicit self loop on 2, node 4 isolated
    src = [0, 1, 0, 1, 1, 2, 2, 2, 3]
    dst = [1, 0, 1, 0, 2, 1, 2, 3, 2]
    ei = np.array([src, dst], dtype=np.int64)
    rowptr, col, dinv = ops.csr_build_host(ei, 5, norm="sym")
    assert rowptr.tolist() == [0, 2, 5, 7, 8, 8]                 # row lengths 2, 3, 2, 1, 0
    assert col.tolist() == [1, 1, 0, 0, 2, 1, 3, 2]              # multiplicity kept, sorted, no diagonal entry
    for i in range(5):
        assert i not in col[rowptr[i]:rowptr[i + 1]].tolist()
    deg = np.array([2.0, 3.0, 2.0, 1.0])
    np.testing.assert_allclose(dinv[:4], deg ** -0.5, rtol=1e-7)
    assert dinv[4] == 0.0 and dinv.dtype == np.float32
    # the GCN flavour of the same list is what it was: one self loop per node, (1 + indeg)^-1/2
    rp2, col2, dinv2 = ops.csr_build_host(ei, 5)
    assert rp2.tolist() == [0, 3, 7, 10, 12, 13] and col2.tolist() == [0, 1, 1, 0, 0, 1, 2, 1, 2, 3, 2, 3, 4]
    np.testing.assert_allclose(dinv2, np.array([3.0, 4.0, 3.0, 2.0, 1.0]) ** -0.5, rtol=1e-7)
    with pytest.raises(ops.DdmpError):
        ops.csr_build_host(ei, 5, norm="rw")
    # capacity: nnz entries suffice for the self-loop-free flavour, one less does not
    L = __import__("dual_dmp_amd._lib", fromlist=["lib"]).lib()
    rp, cc, dv = np.zeros(6, np.int32), np.zeros(8, np.int32), np.zeros(5, np.float32)
    cap = ctypes.c_int64(8)
    assert L.ddmp_csr_build_sym_host(5, 9, ei.ctypes.data, rp.ctypes.data, cc.ctypes.data, dv.ctypes.data, ctypes.byref(cap)) == 0
    assert cap.value == 8
    cap = ctypes.c_int64(7)
    assert L.ddmp_csr_build_sym_host(5, 9, ei.ctypes.data, rp.ctypes.data, cc.ctypes.data, dv.ctypes.data, ctypes.byref(cap)) == -4
    bad = np.array([[0, 7], [1, 0]], dtype=np.int64)
    cap = ctypes.c_int64(8)
    assert L.ddmp_csr_build_sym_host(5, 2, bad.ctypes.data, rp.ctypes.data, cc.ctypes.data, dv.ctypes.data, ctypes.byref(cap)) == -2


def _gcn_names():
    names = []
    for i in range(1, 13):
        names += ["conv%d.bias" % i, "conv%d.lin.weight" % i]
    names += ["linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"]
    for i in range(1, 13):
        names += ["bn%d.weight" % i, "bn%d.bias" % i]
    return names


def test_modular_nets_keep_their_default_and_take_cheb():
    from dual_dmp_amd.networks import PosNet, NormalNet
    torch.manual_seed(2)
    net = PosNet(device="cpu", fused=False)
    assert [n for n, _ in net.named_parameters()] == _gcn_names()
    torch.manual_seed(2)
    again = PosNet("cpu", fused=False, conv="gcn")               # same object, same RNG draws
    for (n1, p1), (n2, p2) in zip(net.named_parameters(), again.named_parameters()):
        assert n1 == n2 and torch.equal(p1, p2)
    assert sum(p.numel() for p in net.parameters()) == 749955
    for make in (PosNet, NormalNet):
        cheb = make("cpu", fused=False, conv="cheb", K=3)
        names = [n for n, _ in cheb.named_parameters()]
        assert "conv1.lins.0.weight" in names and "conv12.lins.2.weight" in names and "conv5.bias" in names
        assert not any(".lin.weight" in n for n in names)
        assert len([n for n in names if n.startswith("conv")]) == 12 * 4
        with pytest.raises(ValueError):
            make("cpu", fused=True, conv="cheb")
        with pytest.raises(ValueError):
            make("cpu", fused=False, conv="sage")


@pytest.mark.parametrize("cin,cout,K,lambda_max", [(5, 6, 1, None), (7, 32, 2, 1.7), (16, 8, 4, 1.7), (6, 3, 5, None)])
def test_chebconv_host_logic_against_autograd(monkeypatch, cin, cout, K, lambda_max):
    """The autograd function's packing, block layout, launch count and Clenshaw backward, with the kernels replaced by a
    float64 CPU stand-in: forward and every gradient against autograd on the dense float64 reference (float32 interfaces:
    1e-6).  The graph has an isolated node and a doubled edge."""
    from dual_dmp_amd import nn_ops
    from cheb_ref import ChebConvRef, CpuChebOps, dense_s
    n = 9
    e = torch.tensor([[0, 1, 2, 3, 4, 5, 6, 0, 0], [1, 2, 3, 4, 5, 6, 0, 3, 1]])    # node 7 and 8: isolated; 0-1 twice
    ei = torch.cat([e, e[[1, 0]]], 1)
    stub = CpuChebOps(dense_s(ei, n))
    monkeypatch.setattr(nn_ops, "ops", stub)
    torch.manual_seed(K)
    ref = ChebConvRef(cin, cout, K).double()
    with torch.no_grad():
        ref.bias.normal_()
    ours = nn_ops.ChebConv(cin, cout, K)
    ours.load_state_dict(ref.state_dict())
    x, dy = torch.randn(n, cin), torch.randn(n, cout)
    xr = x.double().requires_grad_(True)
    yr = ref(xr, ei, lambda_max)
    yr.backward(dy.double())
    lam = 2.0 if lambda_max is None else lambda_max
    xo = x.clone().requires_grad_(True)
    yo = nn_ops._ChebConvFn.apply(xo, ours.bias, None, -2.0 / lam, 2.0 / lam - 1.0, *[l.weight for l in ours.lins])
    assert stub.calls == ["spmm_axpby"] * (K - 1) + ["gemm_nt"]            # K - 1 gathers, ONE GEMM
    stub.calls.clear()
    yo.backward(dy)
    assert sorted(stub.calls) == sorted(["gemm_tn", "gemm_nn"] + ["spmm_axpby"] * (K - 1))
    rel = lambda a, b: float((a.detach().double() - b).norm() / (b.norm() + 1e-30))
    assert rel(yo, yr) < 1e-6 and rel(xo.grad, xr.grad) < 1e-6 and rel(ours.bias.grad, ref.bias.grad) < 1e-6
    for k in range(K):
        assert rel(ours.lins[k].weight.grad, ref.lins[k].weight.grad) < 1e-6, k

"""edge_weight for GCNConv / ChebConv: everything that can be checked without a GPU -- exported entry points and their argument
refusals, the host structure builder of a valued graph and the host restatement of its values against the dense reference
(tests/gcnw_ref.py), the drop-ins' constructor / signature / state_dict, and the refusals that depend on shape, dtype and device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

NEW = ("ddmp_csr_build_valued_host", "ddmp_graph_create_valued", "ddmp_graph_set_values", "ddmp_graph_values_status",
       "ddmp_graph_export_values", "ddmp_spmm_t_f32", "ddmp_sddmm_f32", "ddmp_graph_weight_grad", "ddmp_spmm_lean_selected")


def test_header_declares_and_library_exports_the_valued_graph_entry_points():
    from dual_dmp_amd import _lib
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in NEW:
        assert name in protos, name
        assert hasattr(L, name), name
    assert L.ddmp_abi_version() == 3
    assert len(protos["ddmp_sddmm_f32"][1]) == 8 and len(protos["ddmp_graph_create_valued"][1]) == 6


def test_argument_refusals_come_before_any_device_work():
    from dual_dmp_amd import _lib
    L = _lib.lib()
    buf, other = (ctypes.c_float * 64)(), (ctypes.c_float * 64)()
    fake = (ctypes.c_char * 1024)()                              # a zeroed handle: an UNVALUED graph, never dereferenced further
    p, q, g = ctypes.addressof(buf), ctypes.addressof(other), ctypes.addressof(fake)
    sd = lambda g_, dy, h, G, C=8, lddy=8, ldh=8: L.ddmp_sddmm_f32(g_, dy, lddy, h, ldh, C, G, None)
    assert sd(None, p, q, p) == -1 and sd(g, None, q, p) == -1 and sd(g, p, None, p) == -1 and sd(g, p, q, None) == -1
    assert sd(g, p, q, p, C=0) == -1 and sd(g, p, q, p, lddy=4) == -1 and sd(g, p, q, p, ldh=4) == -1
    assert L.ddmp_graph_set_values(None, p, None) == -1
    assert L.ddmp_graph_set_values(g, p, None) == -1             # an unvalued graph
    assert L.ddmp_graph_weight_grad(g, p, q, None) == -1 and L.ddmp_graph_weight_grad(None, p, q, None) == -1
    st = ctypes.c_int()
    assert L.ddmp_graph_values_status(g, ctypes.byref(st), None) == -1
    assert L.ddmp_graph_export_values(g, p, None, None, None, None) == -1
    tr = lambda g_, x, y, C=8, ldx=8, ldy=8: L.ddmp_spmm_t_f32(g_, x, ldx, y, ldy, C, None, None)
    assert tr(None, p, q) == -1 and tr(g, p, p) == -1 and tr(g, p, q, C=0) == -1 and tr(g, p, q, ldx=4) == -1
    assert tr(g, p, q) == -1                                     # an unvalued graph has no transposed values
    out = ctypes.c_void_p()
    assert L.ddmp_graph_create_valued(0, 0, None, 0, 0, ctypes.byref(out)) == -1
    assert L.ddmp_graph_create_valued(4, 2, None, 0, 0, ctypes.byref(out)) == -1
    assert L.ddmp_graph_create_valued(4, 0, None, 0, 0, None) == -1


def _dense_from_tables(t, vals, n):
    A = np.zeros((n, n), np.float64)
    for i in range(n):
        for e in range(t["rowptr"][i], t["rowptr"][i + 1]):
            assert A[i, t["col"][e]] == 0.0                      # coalesced: one entry per (target, source)
            A[i, t["col"][e]] = vals[e]
    return A


# 7 nodes: 0-1 twice, 1-2, 2-3, 3-0, 4-5, explicit loops on 2 (two of them: the last wins) and on 5, node 6 isolated
_SRC = [0, 1, 0, 1, 1, 2, 2, 3, 3, 0, 2, 4, 5, 2, 5]
_DST = [1, 0, 1, 0, 2, 1, 3, 2, 0, 3, 2, 5, 4, 2, 5]
_N = 7


def _weights(kind, nnz):
    gen = torch.Generator().manual_seed(11)
    w = torch.rand(nnz, generator=gen, dtype=torch.float64) + 0.25
    if kind == "zero":
        w[4] = 0.0                                               # a zero-weight edge (1 -> 2)
    return w.float()


@pytest.mark.parametrize("opts", [dict(), dict(improved=True), dict(add_self_loops=False), dict(normalize=False),
                                  dict(normalize=False, add_self_loops=False)])
@pytest.mark.parametrize("kind", ["nonsym", "zero", "none"])
def test_host_structure_and_values_match_the_dense_reference(opts, kind):
    """Duplicates, an explicit loop, two explicit loops on one node (last wins), improved, add_self_loops=False, normalize=False,
    an isolated node, a zero-weight edge, non-symmetric weights: the coalesced CSR with the host restatement of set_values is
    the dense gcn_norm matrix (float32 values against float64: 1e-6), its mirrored values are the transpose."""
    from dual_dmp_amd import ops
    from gcnw_ref import dense_gcn_norm
    ei = np.array([_SRC, _DST], dtype=np.int64)
    w = None if kind == "none" else _weights(kind, ei.shape[1])
    flags = ops.valued_flags("gcn", **opts)
    t = ops.csr_build_valued_host(ei, _N, flags)
    for i in range(_N):
        row = t["col"][t["rowptr"][i]:t["rowptr"][i + 1]].tolist()
        assert row == sorted(set(row))                           # sorted, no duplicate
    for e in range(len(t["col"])):                               # mirror: (i, j) -> (j, i)
        m = t["mirror"][e]
        i = int(np.searchsorted(t["rowptr"], e, side="right") - 1)
        j = int(np.searchsorted(t["rowptr"], m, side="right") - 1)
        assert t["col"][e] == j and t["col"][m] == i
    a, s, ew, ew_t = ops.valued_values_host(t, None if w is None else w.numpy(), flags)
    ref = dense_gcn_norm(torch.from_numpy(ei), w, _N, **opts).numpy()
    si = np.repeat(s, np.diff(t["rowptr"]))
    A = _dense_from_tables(t, si.astype(np.float64) * ew, _N)
    At = _dense_from_tables(t, si.astype(np.float64) * ew_t, _N)
    assert np.abs(A - ref).max() <= 1e-6 * max(1.0, np.abs(ref).max())
    assert np.abs(At - ref.T).max() <= 1e-6 * max(1.0, np.abs(ref).max())
    normalize, loops = opts.get("normalize", True), opts.get("add_self_loops", True)
    if normalize and loops:
        assert len(t["col"]) == 10 + _N and t["eid"][10] == -1 and t["eid"][13] >= 0      # the first loop on 2 is overridden
        e2 = t["eid"][13]
        assert a[e2] == (1.0 if w is None else w[13].item())
        assert s[6] == (np.float32(2.0) ** -0.5 if opts.get("improved") else 1.0)          # the isolated node: its loop alone
    else:
        assert ref[6].sum() == 0 and (s[6] == 0.0 if normalize else s[6] == 1.0)           # isolated: empty row, inf -> 0
    if w is None and normalize and loops and not opts.get("improved"):
        # all-ones weights, default options: the values of the unvalued builder, bit for bit, wherever the edge list has no
        # duplicate (same structure then) -- here per node: s == dinv
        _, _, dinv = ops.csr_build_host(ei, _N)
        assert np.array_equal(s, dinv)


def test_cheb_flavour_drops_loops_and_nonsymmetric_structure_is_refused():
    from dual_dmp_amd import ops, _lib
    from gcnw_ref import dense_s_weighted
    ei = np.array([_SRC, _DST], dtype=np.int64)
    und = {}
    gen = torch.Generator().manual_seed(5)
    w = torch.zeros(ei.shape[1])
    for k in range(ei.shape[1]):                                 # symmetric weights per undirected pair AND per occurrence
        key = (min(_SRC[k], _DST[k]), max(_SRC[k], _DST[k]))
        und.setdefault(key, float(torch.rand((), generator=gen)) + 0.5)
        w[k] = und[key]
    flags = ops.valued_flags("sym")
    assert flags == ops.GV_DROP_LOOPS | ops.GV_NORMALIZE | ops.GV_REQUIRE_SYM
    t = ops.csr_build_valued_host(ei, _N, flags)
    assert len(t["col"]) == 10 and (t["eid"][[10, 13, 14]] == -1).all()
    a, s, ew, ew_t = ops.valued_values_host(t, w.numpy(), flags)
    assert np.array_equal(a, a[t["mirror"]]) and np.array_equal(ew, ew_t)
    ref = dense_s_weighted(torch.from_numpy(ei), w, _N).numpy()
    A = _dense_from_tables(t, np.repeat(s, np.diff(t["rowptr"])).astype(np.float64) * ew, _N)
    assert np.abs(A - ref).max() <= 1e-6
    # a structure that is not symmetric: DDMP_EINVAL from the builder, ValueError from the wrapper
    bad = np.array([[0, 1, 2], [1, 0, 0]], dtype=np.int64)
    with pytest.raises(ValueError):
        ops.csr_build_valued_host(bad, 3, ops.valued_flags("gcn"))
    L = _lib.lib()
    z = lambda k: np.zeros(k, np.int32)
    rp, col, eep, eei, eid, mir = z(4), z(6), z(7), z(3), z(3), z(6)
    cap = ctypes.c_int64(6)
    call = lambda e, flags, c: L.ddmp_csr_build_valued_host(3, e.shape[1], e.ctypes.data, flags, rp.ctypes.data, col.ctypes.data,
                                                            eep.ctypes.data, eei.ctypes.data, eid.ctypes.data, mir.ctypes.data,
                                                            ctypes.byref(c))
    assert call(bad, 5, cap) == -1
    good = np.array([[0, 1, 2, 0], [1, 0, 0, 2]], dtype=np.int64)
    rp, col, eep, eei, eid, mir = z(4), z(7), z(8), z(4), z(4), z(7)
    cap = ctypes.c_int64(7)
    assert call(good, 5, cap) == 0 and cap.value == 7
    cap = ctypes.c_int64(6)
    assert call(good, 5, cap) == -4                              # capacity
    assert call(good, 1 | 8, ctypes.c_int64(7)) == -1            # LOOPS and DROP_LOOPS together
    assert call(good, 1024, ctypes.c_int64(7)) == -1             # an unknown flag
    oob = np.array([[0, 5], [1, 0]], dtype=np.int64)
    assert call(oob, 5, ctypes.c_int64(7)) == -2


def test_gcnconv_constructor_state_dict_and_signature():
    from dual_dmp_amd.nn_ops import GCNConv, ChebConv
    from gcnw_ref import GCNConvRef
    sig = inspect.signature(GCNConv.__init__)
    assert list(sig.parameters)[1:] == ["in_channels", "out_channels", "improved", "cached", "add_self_loops", "normalize", "bias"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["improved"], d["cached"], d["add_self_loops"], d["normalize"], d["bias"]) == (False, False, True, True, True)
    assert list(inspect.signature(GCNConv.forward).parameters)[1:] == ["x", "edge_index", "edge_weight"]
    assert inspect.signature(GCNConv.forward).parameters["edge_weight"].default is None
    assert "edge_weight" in inspect.signature(ChebConv.forward).parameters
    conv = GCNConv(5, 6, improved=True, cached=True, add_self_loops=False, normalize=True)
    assert list(conv.state_dict().keys()) == ["bias", "lin.weight"]
    res = conv.load_state_dict(GCNConvRef(5, 6).state_dict())
    assert list(res.missing_keys) == [] and list(res.unexpected_keys) == []
    nb = GCNConv(5, 6, bias=False)
    assert nb.bias is None and list(nb.state_dict().keys()) == ["lin.weight"]
    assert [n for n, _ in nb.named_parameters()] == ["lin.weight"]


def test_refusals_that_depend_on_shape_dtype_and_device_only():
    from dual_dmp_amd import ops
    from dual_dmp_amd.nn_ops import GCNConv, ChebConv
    x = torch.randn(4, 5)
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    for conv in (GCNConv(5, 6), ChebConv(5, 6, 2)):
        with pytest.raises(ValueError):
            conv(x, ei, torch.ones(3))                           # wrong length
        with pytest.raises(ValueError):
            conv(x, ei, torch.ones(4, 1))                        # wrong shape
        with pytest.raises(ValueError):
            conv(x, ei, torch.ones(4, dtype=torch.long))         # integer dtype
        with pytest.raises(ValueError):
            conv(x, ei, torch.ones(4, dtype=torch.float16))
        with pytest.raises(ValueError):
            conv(x, ei, torch.ones(4))                           # not on a GPU
        with pytest.raises(ValueError):
            conv(x, ei, [1.0, 1.0, 1.0, 1.0])                    # not a tensor
    with pytest.raises(ops.DdmpError):                           # without weights: the old refusal, no CPU fallback
        GCNConv(5, 6)(x, ei)
    with pytest.raises(ValueError):
        ops.graph_for(ei, 4, edge_weight=torch.ones(5))
    with pytest.raises(ops.DdmpError):
        ops.graph_for(ei, 4, norm="rw", edge_weight=torch.ones(4))


def test_gradient_form_matches_float64_autograd_on_the_host():
    """The chain rule ddmp_graph_weight_grad implements, restated in float64 numpy on the host tables, against autograd through
    the dense reference (non-symmetric weights, duplicates, loop entries): the formula itself, before any kernel."""
    from dual_dmp_amd import ops
    from gcnw_ref import dense_gcn_norm
    ei = np.array([_SRC, _DST], dtype=np.int64)
    gen = torch.Generator().manual_seed(3)
    w = (torch.rand(ei.shape[1], generator=gen, dtype=torch.float64) + 0.25).requires_grad_(True)
    Gd = torch.randn(_N, _N, generator=gen, dtype=torch.float64)
    (dense_gcn_norm(torch.from_numpy(ei), w, _N) * Gd).sum().backward()
    flags = ops.valued_flags("gcn")
    t = ops.csr_build_valued_host(ei, _N, flags)
    rp, col, mir = t["rowptr"], t["col"], t["mirror"]
    wd = w.detach().numpy()
    a = np.array([wd[t["ee_idx"][t["ee_ptr"][e]:t["ee_ptr"][e + 1]]].sum() if t["ee_ptr"][e + 1] > t["ee_ptr"][e] else 1.0
                  for e in range(len(col))])
    row = np.repeat(np.arange(_N), np.diff(rp))
    deg = np.bincount(row, a, _N)
    s = np.where(deg > 0, deg ** -0.5, 0.0)
    G = Gd.numpy()[row, col]
    rc = np.bincount(row, a * s[col] * G + a[mir] * s[col] * G[mir], _N)
    ge = s[row] * s[col] * G - 0.5 * s[row] ** 3 * rc[row]
    dw = np.where(t["eid"] >= 0, ge[np.maximum(t["eid"], 0)], 0.0)
    assert np.linalg.norm(dw - w.grad.numpy()) <= 1e-12 * np.linalg.norm(w.grad.numpy())
    assert dw[10] == 0.0 and w.grad[10] == 0.0                   # the overridden loop gets no gradient


def test_modular_net_weight_lookup():
    """``_ModularNet._weight``: absent attribute -> None (the unweighted operator); a tensor on the net's device is passed as it is
    (a learnable one keeps its gradient path)."""
    from dual_dmp_amd.networks import PosNet

    class Data:
        pass

    net = PosNet("cpu", fused=False)
    d = Data()
    assert net._weight(d, "edge_weight") is None
    d.edge_weight = None
    assert net._weight(d, "edge_weight") is None
    w = torch.ones(4, requires_grad=True)
    d.edge_weight = w
    assert net._weight(d, "edge_weight") is w
    L = __import__("dual_dmp_amd._lib", fromlist=["lib"]).lib()
    assert L.ddmp_spmm_lean_selected(None, 32, 32, 32) == 0

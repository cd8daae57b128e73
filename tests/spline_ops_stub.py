"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the B-spline entry points of ``dual_dmp_amd.ops`` (``spline_fwd``,
``spline_bwd_node``) and of the few other calls ``nn_ops._SplineConvFn`` makes, with the same signatures.  Tests inject it with
``monkeypatch.setattr(nn_ops, "ops", spline_ops_stub)`` to pin the host side (the packed ``[weight blocks ; lin.weight]`` GEMM, the
``[Hf | R]`` / ``[dHf | dR]`` row buffers, the block layout of ``weight``, the ``mirror`` use) without a GPU; the product never
imports it and has no CPU fallback.  The graph is gmm_ops_stub's -- the HOST structure of the valued graph plus ``eid``, the entry
of every input edge.  Arithmetic is float64 internally, float32 at the interfaces.  Every formula is written out per input edge as
the kernels compute it (the reduced block index first, then the wrap of ``+ 1``) -- no autograd."""
import math

import torch

import gmm_ops_stub as _m

DdmpError = _m.DdmpError
SPLINE_MAX_DIM = 5
Graph = _m.Graph
on_device, gemm_nt, gemm_nn, gemm_tn, colsum = _m.on_device, _m.gemm_nt, _m.gemm_nn, _m.gemm_tn, _m.colsum
calls = []                      # names of the entry points reached, in order


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    assert norm == "gat" and edge_weight is None and not improved and normalize and not add_self_loops
    calls.append("graph_for")
    return Graph(edge_index, num_nodes, 0)


def _basis(attr, kernel_size, is_open):
    """-> (b [E_in, S] float64, k [E_in, S] int64), the kernels' way: i0 = floor(v) reduced into [0, kernel_size) once, then
    i0 + 1 == kernel_size wraps to 0."""
    E, dim = attr.shape
    assert len(kernel_size) == dim and len(is_open) == dim and 1 <= dim <= SPLINE_MAX_DIM
    S = 1 << dim
    b = torch.ones((E, S), dtype=torch.float64)
    k = torch.zeros((E, S), dtype=torch.int64)
    stride = 1
    for d in range(dim):
        v = (attr[:, d] * float(kernel_size[d] - int(bool(is_open[d])))).double()       # (the product is rounded in float32)
        fl = torch.floor(v)
        fr = v - fl
        i0 = torch.remainder(fl.long(), kernel_size[d])
        for s in range(S):
            up = (s >> d) & 1
            b[:, s] *= fr if up else 1.0 - fr
            i = i0 + up
            k[:, s] += torch.where(i >= kernel_size[d], torch.zeros_like(i), i) * stride
        stride *= kernel_size[d]
    return b, k


def _counts(g, mean):
    """-> [n] float64: the number of input edges into every row (at least 1), or ones."""
    cnt = torch.zeros(g.n_rows, dtype=torch.float64).index_add_(0, g.row[g.eid], torch.ones(g.nnz_in, dtype=torch.float64))
    return cnt.clamp(min=1.0) if mean else torch.ones_like(cnt)


def spline_fwd(g, hf, attr, kernel_size, is_open, root=None, bias=None, mean=True, out=None):
    calls.append("spline_fwd")
    assert g.values_key == ("ones",) and attr.dtype == torch.float32 and attr.shape[0] == g.nnz_in
    K = math.prod(kernel_size)
    n, C = g.n_rows, hf.shape[1] // K
    assert hf.shape[1] == K * C
    b, k = _basis(attr, kernel_size, is_open)
    src, dst = g.col[g.eid], g.row[g.eid]
    blocks = hf.double().view(-1, K, C)[src.unsqueeze(1), k]                            # [E_in, S, C]
    y = torch.zeros((n, C), dtype=torch.float64).index_add_(0, dst, (b.unsqueeze(-1) * blocks).sum(1))
    y = y / _counts(g, mean).unsqueeze(1)
    if root is not None:
        assert root.shape == (n, C)
        y = y + root.double()
    if bias is not None:
        y = y + bias.double()
    return y.float()


def spline_bwd_node(g, dout, attr, kernel_size, is_open, C, mean=True, out=None, root=False):
    calls.append("spline_bwd_node")
    K = math.prod(kernel_size)
    n = g.n_rows
    assert dout.shape == (n, C)
    hc = K * C
    wt = hc + (C if root else 0)
    b, k = _basis(attr, kernel_size, is_open)
    own = g.mirror[g.eid]                                        # row j's own entry (j, i) of every input edge j -> i
    j, i = g.row[own], g.col[own]
    assert torch.equal(j, g.col[g.eid]) and torch.equal(i, g.row[g.eid])
    gi = dout.double()[i] / _counts(g, mean)[i].unsqueeze(1)                            # [E_in, C]
    dhf = torch.zeros((n * K, C), dtype=torch.float64)
    for s in range(b.shape[1]):
        dhf.index_add_(0, j * K + k[:, s], b[:, s].unsqueeze(1) * gi)
    if out is None:
        out = torch.empty((n, wt), dtype=torch.float32)
    assert out.shape[0] == n and out.shape[1] >= wt
    out[:, :hc] = dhf.view(n, hc).float()
    if root:
        out[:, hc:wt] = dout
    return out[:, :hc], out[:, hc:wt] if root else None

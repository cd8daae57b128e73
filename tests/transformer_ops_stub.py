"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the graph-transformer entry points of ``dual_dmp_amd.ops`` (``tconv_fwd``,
``tconv_bwd_edge``, ``tconv_bwd_node``) and of the few other calls ``nn_ops._TransformerConvFn`` makes, with the same signatures.
Tests inject it with ``monkeypatch.setattr(nn_ops, "ops", transformer_ops_stub)`` to pin the host side (packing, the ``mirror``
use, the head layout, where the skip term and its gradient go) without a GPU; the product never imports it and has no CPU
fallback.  The graph is the HOST structure of the valued graph, as in tests/gat_ops_stub.py.  Arithmetic is float64 internally,
float32 at the interfaces.  Every formula is written out per CSR entry as the kernels compute it -- no autograd."""
import math

import torch

from gat_ops_stub import DdmpError, Graph, _rowsum, colsum, gemm_nn, gemm_nt, gemm_tn, on_device  # noqa: F401
from dual_dmp_amd import ops as _ops

calls = []                      # names of the entry points reached, in order


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    assert norm == "gat" and edge_weight is None and not improved and normalize and not add_self_loops
    calls.append("graph_for")
    return Graph(edge_index, num_nodes, 0)


def _put(out, v):
    if out is None:
        return v.float()
    out.copy_(v)
    return out


def _h(t, heads):
    return t.double().view(t.shape[0], heads, -1)


def tconv_fwd(g, q, k, v, heads, scale=None, skip=None, out=None):
    calls.append("tconv_fwd" if skip is None else "tconv_fwd+skip")
    assert g.values_key == ("ones",) and not (g.valued & _ops.GV_LOOPS)
    n, C = g.n_rows, q.shape[1] // heads
    scale = 1.0 / math.sqrt(C) if scale is None else scale
    z = scale * (_h(q, heads)[g.row] * _h(k, heads)[g.col]).sum(-1)
    m = torch.full((n, heads), -float("inf"), dtype=torch.float64).scatter_reduce(0, g.row.view(-1, 1).expand(-1, heads), z, "amax")
    ex = g.a.view(-1, 1) * torch.exp(z - m[g.row])
    alpha = ex / _rowsum(g, ex)[g.row]
    y = _rowsum(g, alpha.unsqueeze(-1) * _h(v, heads)[g.col]).reshape(n, heads * C)
    if skip is not None:
        y = y + skip.double()
    return _put(out, y), alpha.float()


def tconv_bwd_edge(g, dout, k, v, alpha, heads, scale=None, out=None):
    calls.append("tconv_bwd_edge")
    n, C = g.n_rows, k.shape[1] // heads
    scale = 1.0 / math.sqrt(C) if scale is None else scale
    dal = (_h(dout, heads)[g.row] * _h(v, heads)[g.col]).sum(-1)
    al = alpha.double()
    delta = _rowsum(g, al * dal)
    dz = al * (dal - delta[g.row])
    dq = scale * _rowsum(g, dz.unsqueeze(-1) * _h(k, heads)[g.col])
    return dz.float(), _put(out, dq.reshape(n, heads * C))


def tconv_bwd_node(g, dout, q, alpha, dz, heads, scale=None, out_k=None, out_v=None, out_s=None):
    calls.append("tconv_bwd_node" if out_s is None else "tconv_bwd_node+skip")
    n, C = g.n_rows, q.shape[1] // heads
    scale = 1.0 / math.sqrt(C) if scale is None else scale
    # row j's entries e' enumerate the targets i' = col e' that j feeds; m = mirror e' is the entry (i', j)
    dk = scale * _rowsum(g, dz.double()[g.mirror].unsqueeze(-1) * _h(q, heads)[g.col])
    dv = _rowsum(g, alpha.double()[g.mirror].unsqueeze(-1) * _h(dout, heads)[g.col])
    if out_s is not None:
        out_s.copy_(dout)
    return _put(out_k, dk.reshape(n, heads * C)), _put(out_v, dv.reshape(n, heads * C))

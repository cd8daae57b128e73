"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the residual-gated entry points of ``dual_dmp_amd.ops`` (``rgate_fwd``,
``rgate_bwd_row``, ``rgate_bwd_node``) and of the few other calls ``nn_ops._ResGatedFn`` makes, with the same signatures.  Tests
inject it with ``monkeypatch.setattr(nn_ops, "ops", resgated_ops_stub)`` to pin the host side (packing, the block order, the
``mult[mirror]`` use, where the skip term, the bias and their gradients go) without a GPU; the product never imports it and has
no CPU fallback.  The graph is the HOST structure of the valued graph, as in tests/gat_ops_stub.py.  Arithmetic is float64
internally, float32 at the interfaces.  Every formula is written out per CSR entry as the kernels compute it -- no autograd."""
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


def _gate(g, k, q):
    """g_e = sigmoid(K[row e] + Q[col e]) per entry of the CSR, [entries, C]."""
    return torch.sigmoid(k.double()[g.row] + q.double()[g.col])


def rgate_fwd(g, k, q, v, skip=None, bias=None, out=None):
    calls.append("rgate_fwd" + ("+skip" if skip is not None else "") + ("+bias" if bias is not None else ""))
    assert g.values_key == ("ones",) and not (g.valued & _ops.GV_LOOPS)
    y = _rowsum(g, g.a.view(-1, 1) * _gate(g, k, q) * v.double()[g.col])
    if skip is not None:
        y = y + skip.double()
    if bias is not None:
        y = y + bias.double()
    return _put(out, y)


def rgate_bwd_row(g, dout, k, q, v, out=None):
    calls.append("rgate_bwd_row")
    gt = _gate(g, k, q)
    return _put(out, _rowsum(g, g.a.view(-1, 1) * dout.double()[g.row] * v.double()[g.col] * gt * (1 - gt)))


def rgate_bwd_node(g, dout, k, q, v, out_q=None, out_v=None, out_s=None):
    calls.append("rgate_bwd_node" if out_s is None else "rgate_bwd_node+skip")
    # row j's entries e' enumerate the targets i = col e' that j feeds; the edge j -> i is the entry mirror e' = (i, j), whose
    # multiplicity need not be that of e' = (j, i)
    a = g.a[g.mirror].view(-1, 1)
    gt = torch.sigmoid(k.double()[g.col] + q.double()[g.row])
    d = dout.double()[g.col]
    dq = _rowsum(g, a * d * v.double()[g.row] * gt * (1 - gt))
    dv = _rowsum(g, a * d * gt)
    if out_s is not None:
        out_s.copy_(dout)
    return _put(out_q, dq), _put(out_v, dv)

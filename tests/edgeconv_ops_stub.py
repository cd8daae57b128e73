"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the max-aggregation entry points of ``dual_dmp_amd.ops`` (``gather_max``,
``gather_max_bwd``) and of the few other calls ``nn_ops._EdgeConvFn`` makes, with the same signatures and the same tie rule (the
smallest source id wins).  Tests inject it with ``monkeypatch.setattr(nn_ops, "ops", edgeconv_ops_stub)`` to pin the host side
(the packed ``[Wa - Wb ; Wb]`` GEMM, the ``[A | B]`` / ``[dA | dB]`` row buffers, the weight-gradient recombination) without a
GPU; the product never imports it and has no CPU fallback.  The graph is gat_ops_stub's: the HOST structure of the valued graph.
Every formula is written out per CSR entry as the kernels compute it -- no autograd."""
import torch

import gat_ops_stub as _g

DdmpError = _g.DdmpError
on_device, Graph, gemm_nt, gemm_nn, gemm_tn, colsum, _rowsum = _g.on_device, _g.Graph, _g.gemm_nt, _g.gemm_nn, _g.gemm_tn, _g.colsum, _g._rowsum
calls = []                      # names of the entry points reached, in order
want_args = []                  # the want_arg of every gather_max call


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    calls.append("graph_for")
    return _g.graph_for(edge_index, num_nodes, norm, edge_weight, improved, add_self_loops, normalize)


def gather_max(g, b, a=None, out=None, want_arg=True):
    calls.append("gather_max")
    want_args.append(bool(want_arg))
    assert g.values_key == ("ones",) and b.dtype == torch.float32 and (a is None or a.shape == b.shape)
    n, C = g.n_rows, b.shape[1]
    idx = g.row.view(-1, 1).expand(-1, C)
    vals = b[g.col]
    mx = torch.full((n, C), -float("inf")).scatter_reduce(0, idx, vals, "amax")
    big = torch.iinfo(torch.int64).max
    cand = torch.where(vals == mx[g.row], g.col.view(-1, 1).expand(-1, C), torch.full((), big, dtype=torch.int64))
    arg = torch.full((n, C), big, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin")
    empty = (g.rowptr[1:] == g.rowptr[:-1]).view(-1, 1)
    y = mx if a is None else a + mx                              # one float32 add, as the kernel
    y = torch.where(empty, torch.zeros(()), y)
    arg = torch.where(empty, torch.full((), -1, dtype=torch.int64), arg).to(torch.int32)
    return y, (arg if want_arg else None)


def gather_max_bwd(g, dg, arg, out=None):
    calls.append("gather_max_bwd")
    assert arg is not None and arg.dtype == torch.int32 and arg.shape == dg.shape
    n, C = g.n_rows, dg.shape[1]
    cp = (C + 3) // 4 * 4
    hit = arg.long()[g.col] == g.row.view(-1, 1)
    db = _rowsum(g, torch.where(hit, dg.double()[g.col], torch.zeros((), dtype=torch.float64))).float()
    empty = (g.rowptr[1:] == g.rowptr[:-1]).view(-1, 1)
    da = torch.where(empty, torch.zeros(()), dg[:n])
    if out is None:
        out = torch.empty((n, 2 * cp))
    assert out.shape == (n, 2 * cp)
    out[:, :C], out[:, cp:cp + C] = da, db
    return out[:, :C], out[:, cp:cp + C]

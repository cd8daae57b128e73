"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the graph-attention entry points of ``dual_dmp_amd.ops`` (``gat_scores``,
``gat_fwd``, ``gat_bwd_edge``, ``gat_bwd_node``, ``gat_datt``) and of the few other calls ``nn_ops._GATConvFn`` makes, with the
same signatures.  Tests inject it with ``monkeypatch.setattr(nn_ops, "ops", gat_ops_stub)`` to pin the host side (packing, the
``mirror`` use, the head layout) without a GPU; the product never imports it and has no CPU fallback.  The graph is the HOST
structure of the valued graph (``ops.csr_build_valued_host`` + ``ops.valued_values_host``: library host code, no GPU).  Arithmetic
is float64 internally, float32 at the interfaces.  Every formula is written out per CSR entry as the kernels compute it -- no
autograd."""
import contextlib

import numpy as np
import torch

from dual_dmp_amd import ops as _ops

DdmpError = _ops.DdmpError
calls = []                      # names of the entry points reached, in order


def on_device(dev):
    return contextlib.nullcontext()


class Graph:
    def __init__(self, edge_index, n, flags):
        t = _ops.csr_build_valued_host(edge_index.cpu().numpy(), n, flags)
        a = _ops.valued_values_host(t, None, flags)[0]
        self.n_rows = self.n_cols = int(n)
        self.nnz = len(t["col"])
        self.rowptr = torch.from_numpy(t["rowptr"].astype(np.int64))
        self.col = torch.from_numpy(t["col"].astype(np.int64))
        self.mirror = torch.from_numpy(t["mirror"].astype(np.int64))
        self.row = torch.repeat_interleave(torch.arange(n), self.rowptr[1:] - self.rowptr[:-1])
        self.a = torch.from_numpy(a.astype(np.float64))
        self.valued, self.values_key = flags | _ops.GV_VALUED, ("ones",)


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    assert norm == "gat" and edge_weight is None and not improved and normalize
    calls.append("graph_for")
    return Graph(edge_index, num_nodes, _ops.GV_LOOPS if add_self_loops else 0)


def gemm_nt(a, w, out=None, bias=None):
    y = a.double() @ w.double().t()
    return (y if bias is None else y + bias.double()).float()


def gemm_nn(a, w, out=None):
    return (a.double() @ w.double()).float()


def gemm_tn(g, z, out=None):
    return (g.double().t() @ z.double()).float()


def colsum(x, sums=None, n_rows=None):
    return x.double().sum(0)


def _rowsum(g, v):
    return torch.zeros((g.n_rows,) + tuple(v.shape[1:]), dtype=v.dtype).index_add_(0, g.row, v)


def _z(g, s_src, s_dst):
    return s_src.double()[g.col] + s_dst.double()[g.row]                                # [entries, heads], before the leaky relu


def gat_scores(hf, att_src, att_dst, heads):
    calls.append("gat_scores")
    n, C = hf.shape[0], hf.shape[1] // heads
    h3 = hf.double().view(n, heads, C)
    return (h3 * att_src.double().view(1, heads, C)).sum(-1).float(), (h3 * att_dst.double().view(1, heads, C)).sum(-1).float()


def gat_fwd(g, hf, s_src, s_dst, heads, slope, bias=None, out=None):
    calls.append("gat_fwd")
    assert g.values_key == ("ones",)
    n, C = g.n_rows, hf.shape[1] // heads
    z0 = _z(g, s_src, s_dst)
    z = torch.where(z0 > 0, z0, slope * z0)
    m = torch.full((n, heads), -float("inf"), dtype=torch.float64).scatter_reduce(0, g.row.view(-1, 1).expand(-1, heads), z, "amax")
    ex = g.a.view(-1, 1) * torch.exp(z - m[g.row])
    alpha = ex / _rowsum(g, ex)[g.row]
    y = _rowsum(g, alpha.unsqueeze(-1) * hf.double().view(-1, heads, C)[g.col]).reshape(n, heads * C)
    if bias is not None:
        y = y + bias.double()
    return y.float(), alpha.float()


def gat_bwd_edge(g, dout, hf, s_src, s_dst, alpha, heads, slope):
    calls.append("gat_bwd_edge")
    C = hf.shape[1] // heads
    dal = (dout.double().view(-1, heads, C)[g.row] * hf.double().view(-1, heads, C)[g.col]).sum(-1)
    al = alpha.double()
    delta = _rowsum(g, al * dal)
    z0 = _z(g, s_src, s_dst)
    ds = al * (dal - delta[g.row]) * torch.where(z0 > 0, torch.ones_like(z0), torch.full_like(z0, slope))
    return ds.float(), _rowsum(g, ds).float()


def gat_bwd_node(g, dout, alpha, ds, ds_dst, att_src, att_dst, heads):
    calls.append("gat_bwd_node")
    n, C = g.n_rows, dout.shape[1] // heads
    ds_src = _rowsum(g, ds.double()[g.mirror])
    dhf = _rowsum(g, alpha.double()[g.mirror].unsqueeze(-1) * dout.double().view(-1, heads, C)[g.col])
    dhf = dhf + ds_src.unsqueeze(-1) * att_src.double().view(1, heads, C) + ds_dst.double().unsqueeze(-1) * att_dst.double().view(1, heads, C)
    return dhf.reshape(n, heads * C).float(), ds_src.float()


def gat_datt(hf, ds_src, ds_dst, heads):
    calls.append("gat_datt")
    n, C = hf.shape[0], hf.shape[1] // heads
    h3 = hf.double().view(n, heads, C)
    return (ds_src.double().unsqueeze(-1) * h3).sum(0).float(), (ds_dst.double().unsqueeze(-1) * h3).sum(0).float()

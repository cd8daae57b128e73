"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the dynamic-attention entry points of ``dual_dmp_amd.ops`` (``gatv2_fwd``,
``gatv2_bwd_edge``, ``gatv2_bwd_node``, ``gatv2_datt``) and of the few other calls ``nn_ops._GATv2ConvFn`` makes, with the same
signatures.  Tests inject it with ``monkeypatch.setattr(nn_ops, "ops", gatv2_ops_stub)`` to pin the host side (packing, the
``mirror`` use, the head layout, the shared-weights sum) without a GPU; the product never imports it and has no CPU fallback.
The graph is the HOST structure of the valued graph, as in tests/gat_ops_stub.py.  Arithmetic is float64 internally, float32 at
the interfaces.  Every formula is written out per CSR entry as the kernels compute it -- no autograd."""
import torch

from gat_ops_stub import DdmpError, Graph, _rowsum, colsum, gemm_nn, gemm_nt, gemm_tn, on_device  # noqa: F401
from dual_dmp_amd import ops as _ops

calls = []                      # names of the entry points reached, in order


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    assert norm == "gat" and edge_weight is None and not improved and normalize
    calls.append("graph_for")
    return Graph(edge_index, num_nodes, _ops.GV_LOOPS if add_self_loops else 0)


def _u(g, xl, xr, heads):
    C = xl.shape[1] // heads
    # the float32 sum the kernels form, then float64
    return (xl.view(-1, heads, C)[g.col] + xr.view(-1, heads, C)[g.row]).double(), C


def _put(out, v):
    if out is None:
        return v.float()
    out.copy_(v)
    return out


def gatv2_fwd(g, xl, xr, att, heads, slope, bias=None, out=None):
    calls.append("gatv2_fwd")
    assert g.values_key == ("ones",) and att.shape[0] == heads
    n = g.n_rows
    u, C = _u(g, xl, xr, heads)
    z = (torch.where(u > 0, u, slope * u) * att.double().view(1, heads, C)).sum(-1)
    m = torch.full((n, heads), -float("inf"), dtype=torch.float64).scatter_reduce(0, g.row.view(-1, 1).expand(-1, heads), z, "amax")
    ex = g.a.view(-1, 1) * torch.exp(z - m[g.row])
    alpha = ex / _rowsum(g, ex)[g.row]
    y = _rowsum(g, alpha.unsqueeze(-1) * xl.double().view(-1, heads, C)[g.col]).reshape(n, heads * C)
    if bias is not None:
        y = y + bias.double()
    return _put(out, y), alpha.float()


def gatv2_bwd_edge(g, dout, xl, xr, att, alpha, heads, slope, out=None, want_datt=True):
    calls.append("gatv2_bwd_edge")
    n = g.n_rows
    u, C = _u(g, xl, xr, heads)
    dal = (dout.double().view(-1, heads, C)[g.row] * xl.double().view(-1, heads, C)[g.col]).sum(-1)
    al = alpha.double()
    delta = _rowsum(g, al * dal)
    dz = al * (dal - delta[g.row])
    dl = torch.where(u > 0, torch.ones_like(u), torch.full_like(u, slope))
    dxr = _rowsum(g, dz.unsqueeze(-1) * dl) * att.double().view(1, heads, C)
    part = _rowsum(g, dz.unsqueeze(-1) * torch.where(u > 0, u, slope * u)).reshape(n, heads * C).float() if want_datt else None
    return dz.float(), _put(out, dxr.reshape(n, heads * C)), part


def gatv2_bwd_node(g, dout, xl, xr, att, alpha, dz, heads, slope, out=None):
    calls.append("gatv2_bwd_node")
    n = g.n_rows
    C = xl.shape[1] // heads
    # row j's entries e' enumerate the targets i' = col e' that j feeds; m = mirror e' is the entry (i', j)
    u = (xl.view(-1, heads, C)[g.row] + xr.view(-1, heads, C)[g.col]).double()
    dl = torch.where(u > 0, torch.ones_like(u), torch.full_like(u, slope))
    t = alpha.double()[g.mirror].unsqueeze(-1) * dout.double().view(-1, heads, C)[g.col]
    t = t + dz.double()[g.mirror].unsqueeze(-1) * att.double().view(1, heads, C) * dl
    return _put(out, _rowsum(g, t).reshape(n, heads * C))


def gatv2_datt(part, heads):
    calls.append("gatv2_datt")
    return part.double().sum(0).view(heads, -1).float()

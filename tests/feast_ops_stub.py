"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the feature-steered entry points of ``dual_dmp_amd.ops`` (``feast_fwd``,
``feast_bwd_edge``, ``feast_bwd_node``, ``feast_dc``) and of the few other calls ``nn_ops._FeaStConvFn`` makes, with the same
signatures.  Tests inject it with ``monkeypatch.setattr(nn_ops, "ops", feast_ops_stub)`` to pin the host side (the packed
``[lin.weight; u.weight]`` GEMM, the ``[Hf | P]`` / ``[dHf | dP]`` row buffers, the ``mirror`` use, the head layout) without a GPU;
the product never imports it and has no CPU fallback.  The graph is gat_ops_stub's: the HOST structure of the valued graph.
Arithmetic is float64 internally, float32 at the interfaces.  Every formula is written out per CSR entry as the kernels compute
it -- no autograd."""
import torch

import gat_ops_stub as _g

DdmpError = _g.DdmpError
on_device, Graph, gemm_nt, gemm_nn, gemm_tn, colsum, _rowsum = _g.on_device, _g.Graph, _g.gemm_nt, _g.gemm_nn, _g.gemm_tn, _g.colsum, _g._rowsum
calls = []                      # names of the entry points reached, in order


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    calls.append("graph_for")
    return _g.graph_for(edge_index, num_nodes, norm, edge_weight, improved, add_self_loops, normalize)


def feast_fwd(g, hf, p, c, heads, bias=None, out=None):
    calls.append("feast_fwd")
    assert g.values_key == ("ones",) and p.shape[1] == heads and c.shape == (heads,)
    n, C = g.n_rows, hf.shape[1] // heads
    z = p.double()[g.col] - p.double()[g.row] + c.double()
    ex = torch.exp(z - z.amax(1, keepdim=True))
    q = ex / ex.sum(1, keepdim=True)
    deg = _rowsum(g, g.a)
    beta = (g.a / deg[g.row]).view(-1, 1) * q
    y = _rowsum(g, (beta.unsqueeze(-1) * hf.double().view(-1, heads, C)[g.col]).sum(1))
    if bias is not None:
        y = y + bias.double()
    return y.float(), beta.float()


def feast_bwd_edge(g, dout, hf, beta, heads):
    calls.append("feast_bwd_edge")
    C = hf.shape[1] // heads
    assert dout.shape[1] == C
    ge = torch.einsum("ec,ehc->eh", dout.double()[g.row], hf.double().view(-1, heads, C)[g.col])
    b = beta.double()
    delta = (b * ge).sum(1, keepdim=True) / b.sum(1, keepdim=True)
    dz = b * (ge - delta)
    return dz.float(), _rowsum(g, dz).float()


def feast_bwd_node(g, dout, beta, dz, rs, heads, out=None):
    calls.append("feast_bwd_node")
    n, C = g.n_rows, dout.shape[1]
    dhf = _rowsum(g, beta.double()[g.mirror].unsqueeze(-1) * dout.double()[g.col].unsqueeze(1)).reshape(n, heads * C).float()
    dp = (_rowsum(g, dz.double()[g.mirror]) - rs.double()).float()
    if out is None:
        return dhf, dp
    hc = heads * C
    assert out.shape[0] == n and out.shape[1] >= hc + heads
    out[:, :hc], out[:, hc:hc + heads] = dhf, dp
    return out[:, :hc], out[:, hc:hc + heads]


def feast_dc(rs, heads):
    calls.append("feast_dc")
    assert rs.shape[1] == heads
    return rs.double().sum(0).float()

"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the Gaussian-mixture entry points of ``dual_dmp_amd.ops`` (``gmm_fwd``,
``gmm_bwd_edge``, ``gmm_bwd_node``) and of the few other calls ``nn_ops._GMMConvFn`` makes, with the same signatures.  Tests
inject it with ``monkeypatch.setattr(nn_ops, "ops", gmm_ops_stub)`` to pin the host side (the packed ``[g^T ; root.weight]`` GEMM,
the ``[Hf | R]`` / ``[dHf | dR]`` row buffers, the ``mirror`` use, the component layout, the ``[dmu | dsigma]`` column layout)
without a GPU; the product never imports it and has no CPU fallback.  The graph is gat_ops_stub's -- the HOST structure of the
valued graph -- plus ``eid``, the entry of every input edge.  Arithmetic is float64 internally, float32 at the interfaces.  Every
formula is written out per CSR entry / input edge as the kernels compute it -- no autograd."""
import numpy as np
import torch

import gat_ops_stub as _g
from dual_dmp_amd import ops as _ops

DdmpError = _g.DdmpError
on_device, gemm_nt, gemm_nn, gemm_tn, colsum, _rowsum = _g.on_device, _g.gemm_nt, _g.gemm_nn, _g.gemm_tn, _g.colsum, _g._rowsum
calls = []                      # names of the entry points reached, in order
EPS = 1e-15


class Graph(_g.Graph):
    def __init__(self, edge_index, n, flags):
        super().__init__(edge_index, n, flags)
        t = _ops.csr_build_valued_host(edge_index.cpu().numpy(), n, flags)
        self.eid = torch.from_numpy(t["eid"].astype(np.int64))
        self.nnz_in = int(edge_index.shape[1])
        assert flags == 0 and bool((self.eid >= 0).all())


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    assert norm == "gat" and edge_weight is None and not improved and normalize and not add_self_loops
    calls.append("graph_for")
    return Graph(edge_index, num_nodes, 0)


def _gamma(g, attr, mu, sigma):
    """-> (gamma [E_in, K], diff [E_in, K, dim], inv [K, dim], deg [n]) in float64."""
    assert attr.shape[0] == g.nnz_in and mu.shape == sigma.shape and attr.shape[1] == mu.shape[1]
    inv = 1.0 / (EPS + sigma.double() ** 2)
    diff = attr.double().unsqueeze(1) - mu.double().unsqueeze(0)
    return torch.exp(-0.5 * (diff ** 2 * inv).sum(-1)), diff, inv, _rowsum(g, g.a)


def gmm_fwd(g, hf, attr, mu, sigma, K, root=None, bias=None, out=None):
    calls.append("gmm_fwd")
    assert g.values_key == ("ones",) and mu.shape[0] == K
    n, C = g.n_rows, hf.shape[1] // K
    gamma, _, _, deg = _gamma(g, attr, mu, sigma)
    w = torch.zeros((g.nnz, K), dtype=torch.float64).index_add_(0, g.eid, gamma) / deg[g.row].unsqueeze(1)
    y = _rowsum(g, (w.unsqueeze(-1) * hf.double().view(-1, K, C)[g.col]).sum(1))
    if root is not None:
        assert root.shape == (n, C)
        y = y + root.double()
    if bias is not None:
        y = y + bias.double()
    return y.float(), w.float()


def gmm_bwd_edge(g, dout, hf, attr, mu, sigma, K, want_dattr=False):
    calls.append("gmm_bwd_edge")
    n, C = g.n_rows, hf.shape[1] // K
    assert dout.shape[1] == C
    gamma, diff, inv, deg = _gamma(g, attr, mu, sigma)
    ge = torch.einsum("ec,ekc->ek", dout.double()[g.row], hf.double().view(-1, K, C)[g.col])
    c = gamma * ge[g.eid] / deg[g.row[g.eid]].unsqueeze(1)                              # [E_in, K]
    u = c.unsqueeze(-1) * diff * inv                                                    # the dmu terms [E_in, K, dim]
    v = u * diff * (sigma.double() * inv)                                               # the dsigma terms
    tgt = g.row[g.eid]
    parts = torch.zeros((n, 2 * mu.numel()), dtype=torch.float64).index_add_(0, tgt, torch.cat([u.flatten(1), v.flatten(1)], 1))
    return parts.float(), (-u.sum(1)).float() if want_dattr else None


def gmm_bwd_node(g, dout, w, K, out=None, root=False):
    calls.append("gmm_bwd_node")
    n, C = g.n_rows, dout.shape[1]
    hc = K * C
    wt = hc + (C if root else 0)
    dhf = _rowsum(g, w.double()[g.mirror].unsqueeze(-1) * dout.double()[g.col].unsqueeze(1)).reshape(n, hc).float()
    if out is None:
        out = torch.empty((n, wt), dtype=torch.float32)
    assert out.shape[0] == n and out.shape[1] >= wt
    out[:, :hc] = dhf
    if root:
        out[:, hc:wt] = dout
    return out[:, :hc], out[:, hc:wt] if root else None


def feast_dc(rs, heads):
    calls.append("feast_dc")
    assert rs.shape[1] == heads
    return rs.double().sum(0).float()

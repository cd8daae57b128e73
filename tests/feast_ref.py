"""TEST-SIDE REFERENCE for FeaStConv: two independent restatements of torch_geometric 2.2.0's FeaStConv (int ``in_channels``,
mean aggregation) in plain torch, float64 by default, differentiable.

* ``feast_edge_list`` / ``FeaStConvRef`` -- the edge-list form PyG itself uses: remove self loops, add one per node, a per-edge
  softmax over the heads of ``u (x_j - x_i) + c``, the head-mixed source rows, a scatter mean over the edges of each target
  (``index_add_`` and a count).  Duplicate edges are separate edges.
* ``dense_feast`` -- a dense [N, N, heads] form whose multiplicities come from an accumulated adjacency matrix.

``edge_index`` row 0 = source j, row 1 = target i."""
import math

import torch
import torch.nn as nn


def feast_edges(edge_index, n, add_self_loops=True):
    """-> (src, dst) the operator aggregates over: with ``add_self_loops`` explicit loops leave and every node gets exactly one."""
    src, dst = edge_index[0], edge_index[1]
    if add_self_loops:
        keep = src != dst
        loop = torch.arange(n, dtype=src.dtype, device=src.device)
        src, dst = torch.cat([src[keep], loop]), torch.cat([dst[keep], loop])
    return src, dst


def feast_edge_list(x, edge_index, weight, u, c, bias, heads, add_self_loops=True, full=False):
    """The edge-list form.  ``weight``: [heads * out, in], ``u``: [heads, in], ``c``: [heads], ``bias``: [out] or None.
    ``full``: -> (out, dict(src, dst, hf, p, z, q, deg)); ``z`` (the per-edge logits P[j] - P[i] + c, [E, heads]) keeps its gradient:
    that is dz per edge."""
    n = x.shape[0]
    C = weight.shape[0] // heads
    hf = (x @ weight.t()).view(n, heads, C)
    p = x @ u.t()
    src, dst = feast_edges(edge_index, n, add_self_loops)
    z = p[src] - p[dst] + c
    if full:
        z.retain_grad()
    q = torch.softmax(z, dim=1)
    msg = (q.unsqueeze(-1) * hf[src]).sum(1)
    deg = torch.zeros(n, dtype=x.dtype).index_add_(0, dst, torch.ones(len(dst), dtype=x.dtype))
    out = torch.zeros((n, C), dtype=x.dtype).index_add_(0, dst, msg) / deg.clamp(min=1.0).unsqueeze(-1)
    if bias is not None:
        out = out + bias
    if full:
        return out, dict(src=src, dst=dst, hf=hf, p=p, z=z, q=q, deg=deg)
    return out


def dense_feast(x, edge_index, weight, u, c, bias, heads, add_self_loops=True):
    """The dense form: cnt[i, j] = number of edges j -> i (diagonal forced to 1 with ``add_self_loops``); out[i] = sum_j cnt[i, j]
    sum_h softmax_h(P[j] - P[i] + c)[h] Hf[j, h] / sum_j cnt[i, j]."""
    n = x.shape[0]
    C = weight.shape[0] // heads
    hf = torch.einsum("ni,hci->nhc", x, weight.view(heads, C, -1))
    p = torch.einsum("ni,hi->nh", x, u)
    cnt = torch.zeros((n, n), dtype=x.dtype)
    cnt.index_put_((edge_index[1], edge_index[0]), torch.ones(edge_index.shape[1], dtype=x.dtype), accumulate=True)
    if add_self_loops:
        cnt.fill_diagonal_(1.0)
    z = p.unsqueeze(0) - p.unsqueeze(1) + c                       # [i, j, h]
    z = z - z.amax(2, keepdim=True).detach()
    e = torch.exp(z)
    q = e / e.sum(2, keepdim=True)
    deg = cnt.sum(1)
    wgt = cnt / torch.where(deg > 0, deg, torch.ones_like(deg)).unsqueeze(1)
    out = torch.einsum("ij,ijh,jhc->ic", wgt, q, hf)
    if bias is not None:
        out = out + bias
    return out


class FeaStConvRef(nn.Module):
    """Edge-list reference with PyG's parameter names and shapes."""

    def __init__(self, in_channels, out_channels, heads=1, add_self_loops=True, bias=True, dtype=torch.float64):
        super().__init__()
        self.in_channels, self.out_channels, self.heads, self.add_self_loops = in_channels, out_channels, heads, add_self_loops
        self.lin = nn.Linear(in_channels, heads * out_channels, bias=False, dtype=dtype)
        self.u = nn.Linear(in_channels, heads, bias=False, dtype=dtype)
        self.c = nn.Parameter(torch.empty(heads, dtype=dtype))
        self.bias = nn.Parameter(torch.empty(out_channels, dtype=dtype)) if bias else None
        a = 1.0 / math.sqrt(in_channels)
        with torch.no_grad():
            self.lin.weight.uniform_(-a, a)
            self.u.weight.uniform_(-a, a)
            self.c.normal_(0.0, 0.1)
            if self.bias is not None:
                self.bias.normal_(0.0, 0.1)

    def load_from(self, conv):
        """Copy the parameters of a ``FeaStConv`` (or another reference) into this one, in this one's dtype."""
        with torch.no_grad():
            self.lin.weight.copy_(conv.lin.weight.detach().cpu())
            self.u.weight.copy_(conv.u.weight.detach().cpu())
            self.c.copy_(conv.c.detach().cpu())
            if self.bias is not None:
                self.bias.copy_(conv.bias.detach().cpu())
        return self

    def forward(self, x, edge_index, full=False):
        return feast_edge_list(x, edge_index, self.lin.weight, self.u.weight, self.c, self.bias, self.heads, self.add_self_loops,
                               full=full)

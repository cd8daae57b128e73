"""TEST-SIDE REFERENCE for GATConv: two independent restatements of torch_geometric 2.2.0's GATConv (int ``in_channels``, no
edge features, no dropout) in plain torch, float64 by default, differentiable.

* ``GATConvRef`` -- the edge-list form PyG itself uses: remove self loops, add one per node, per-edge scores, a scatter softmax
  over the edges of each target (``index_add_``), a scatter sum of the weighted source rows.  Duplicate edges are separate edges.
* ``dense_gat`` -- a dense [N, N, heads] masked softmax whose multiplicities come from an accumulated adjacency matrix.

``edge_index`` row 0 = source j, row 1 = target i."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


def gat_edges(edge_index, n, add_self_loops=True):
    """-> (src, dst) the operator attends over: with ``add_self_loops`` explicit loops leave and every node gets exactly one."""
    src, dst = edge_index[0], edge_index[1]
    if add_self_loops:
        keep = src != dst
        loop = torch.arange(n, dtype=src.dtype, device=src.device)
        src, dst = torch.cat([src[keep], loop]), torch.cat([dst[keep], loop])
    return src, dst


def gat_edge_list(x, edge_index, weight, att_src, att_dst, bias, heads, concat=True, negative_slope=0.2, add_self_loops=True,
                  full=False):
    """The edge-list form.  ``full``: -> (out, dict(src, dst, hf, s_src, s_dst, pre, alpha)); ``pre`` (the per-edge
    s_src[j] + s_dst[i], [E, heads]) keeps its gradient."""
    n = x.shape[0]
    C = weight.shape[0] // heads
    hf = (x @ weight.t()).view(n, heads, C)
    s_src = (hf * att_src.view(1, heads, C)).sum(-1)
    s_dst = (hf * att_dst.view(1, heads, C)).sum(-1)
    src, dst = gat_edges(edge_index, n, add_self_loops)
    pre = s_src[src] + s_dst[dst]
    if full:
        pre.retain_grad()
    z = F.leaky_relu(pre, negative_slope)
    m = torch.full((n, heads), -math.inf, dtype=z.dtype).scatter_reduce(0, dst.view(-1, 1).expand(-1, heads), z.detach(), "amax")
    ex = torch.exp(z - m[dst])
    den = torch.zeros((n, heads), dtype=z.dtype).index_add_(0, dst, ex)
    alpha = ex / den[dst]
    out = torch.zeros((n, heads, C), dtype=z.dtype).index_add_(0, dst, alpha.unsqueeze(-1) * hf[src])
    out = out.reshape(n, heads * C) if concat else out.mean(1)
    if bias is not None:
        out = out + bias
    if full:
        return out, dict(src=src, dst=dst, hf=hf, s_src=s_src, s_dst=s_dst, pre=pre, alpha=alpha)
    return out


def dense_gat(x, edge_index, weight, att_src, att_dst, bias, heads, concat=True, negative_slope=0.2, add_self_loops=True):
    """The dense form: cnt[i, j] = number of edges j -> i (diagonal forced to 1 with ``add_self_loops``), softmax over j of
    cnt * exp(z) per head."""
    n = x.shape[0]
    C = weight.shape[0] // heads
    hf = (x @ weight.t()).view(n, heads, C)
    s_src = torch.einsum("nhc,hc->nh", hf, att_src.view(heads, C))
    s_dst = torch.einsum("nhc,hc->nh", hf, att_dst.view(heads, C))
    cnt = torch.zeros((n, n), dtype=x.dtype)
    cnt.index_put_((edge_index[1], edge_index[0]), torch.ones(edge_index.shape[1], dtype=x.dtype), accumulate=True)
    if add_self_loops:
        cnt.fill_diagonal_(1.0)
    z = F.leaky_relu(s_src.unsqueeze(0) + s_dst.unsqueeze(1), negative_slope)          # [i, j, h]
    mask = (cnt > 0).unsqueeze(-1)
    m = torch.where(mask, z, torch.full_like(z, -math.inf)).amax(1, keepdim=True).detach()
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))                         # (a row without entries)
    e = torch.where(mask, cnt.unsqueeze(-1) * torch.exp(torch.where(mask, z - m, torch.zeros_like(z))), torch.zeros_like(z))
    den = e.sum(1, keepdim=True)
    alpha = e / torch.where(den > 0, den, torch.ones_like(den))
    out = torch.einsum("ijh,jhc->ihc", alpha, hf)
    out = out.reshape(n, heads * C) if concat else out.mean(1)
    if bias is not None:
        out = out + bias
    return out


class GATConvRef(nn.Module):
    """Edge-list reference with PyG's parameter names and shapes (``lin_src`` / ``lin_dst`` are one module)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, add_self_loops=True, bias=True,
                 dtype=torch.float64):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.add_self_loops = concat, negative_slope, add_self_loops
        self.lin_src = nn.Linear(in_channels, heads * out_channels, bias=False, dtype=dtype)
        self.lin_dst = self.lin_src
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels, dtype=dtype))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels, dtype=dtype))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels, dtype=dtype)) if bias else None
        a, b = math.sqrt(6.0 / (in_channels + heads * out_channels)), math.sqrt(6.0 / (heads + out_channels))
        with torch.no_grad():
            self.lin_src.weight.uniform_(-a, a)
            self.att_src.uniform_(-b, b)
            self.att_dst.uniform_(-b, b)

    def load_from(self, conv):
        """Copy the parameters of a ``GATConv`` (or another reference) into this one, in this one's dtype."""
        with torch.no_grad():
            self.lin_src.weight.copy_(conv.lin_src.weight.detach().cpu())
            self.att_src.copy_(conv.att_src.detach().cpu())
            self.att_dst.copy_(conv.att_dst.detach().cpu())
            if self.bias is not None:
                self.bias.copy_(conv.bias.detach().cpu())
        return self

    def forward(self, x, edge_index, full=False):
        return gat_edge_list(x, edge_index, self.lin_src.weight, self.att_src, self.att_dst, self.bias, self.heads, self.concat,
                             self.negative_slope, self.add_self_loops, full=full)

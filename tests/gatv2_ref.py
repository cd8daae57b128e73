"""TEST-SIDE REFERENCE for GATv2Conv: two independent restatements of torch_geometric 2.2.0's GATv2Conv (int ``in_channels``, no
edge features, no dropout) in plain torch, float64 by default, differentiable.

* ``gatv2_core`` / ``gatv2_edge_list`` / ``GATv2ConvRef`` -- the edge-list form PyG itself uses: remove self loops, add one per
  node, per-edge ``u = Xl[j] + Xr[i]``, ``z = sum_c att leaky_relu(u)``, a scatter softmax over the edges of each target
  (``index_add_``), a scatter sum of the weighted source rows.  Duplicate edges are separate edges.
* ``dense_gatv2`` -- a dense [N, N, heads] masked softmax whose multiplicities come from an accumulated adjacency matrix.

``pos`` (edge-list form only): a bool [E, heads, C] tensor that REPLACES the reference's own ``u > 0`` decisions, in the leaky
relu and with it in its derivative (teacher forcing across the kink; E counts the edges of ``gatv2_edges``, in its order).

``edge_index`` row 0 = source j, row 1 = target i."""
import math

import torch
import torch.nn as nn


def gatv2_edges(edge_index, n, add_self_loops=True):
    """-> (src, dst) the operator attends over: with ``add_self_loops`` explicit loops leave and every node gets exactly one."""
    src, dst = edge_index[0], edge_index[1]
    if add_self_loops:
        keep = src != dst
        loop = torch.arange(n, dtype=src.dtype, device=src.device)
        src, dst = torch.cat([src[keep], loop]), torch.cat([dst[keep], loop])
    return src, dst


def gatv2_core(xl, xr, edge_index, att, bias, heads, concat=True, negative_slope=0.2, add_self_loops=True, full=False, pos=None):
    """The edge-list form from ``xl`` / ``xr`` [N, heads * C].  ``full``: -> (out, dict(src, dst, u, z, alpha)); ``z`` ([E, heads])
    keeps its gradient."""
    n = xl.shape[0]
    C = xl.shape[1] // heads
    xl3, xr3 = xl.view(n, heads, C), xr.view(n, heads, C)
    src, dst = gatv2_edges(edge_index, n, add_self_loops)
    u = xl3[src] + xr3[dst]
    own = u > 0
    lu = torch.where(own if pos is None else pos, u, negative_slope * u)
    z = (lu * att.view(1, heads, C)).sum(-1)
    if full and z.requires_grad:
        z.retain_grad()
    m = torch.full((n, heads), -math.inf, dtype=z.dtype).scatter_reduce(0, dst.view(-1, 1).expand(-1, heads), z.detach(), "amax")
    ex = torch.exp(z - m[dst])
    den = torch.zeros((n, heads), dtype=z.dtype).index_add_(0, dst, ex)
    alpha = ex / den[dst]
    out = torch.zeros((n, heads, C), dtype=z.dtype).index_add_(0, dst, alpha.unsqueeze(-1) * xl3[src])
    out = out.reshape(n, heads * C) if concat else out.mean(1)
    if bias is not None:
        out = out + bias
    if full:
        return out, dict(src=src, dst=dst, u=u, own=own, z=z, alpha=alpha)
    return out


def _lin(x, w, b):
    y = x @ w.t()
    return y if b is None else y + b


def gatv2_edge_list(x, edge_index, wl, bl, wr, br, att, bias, heads, concat=True, negative_slope=0.2, add_self_loops=True,
                    full=False, pos=None):
    """``wr`` None: shared weights (Xr = Xl)."""
    xl = _lin(x, wl, bl)
    xr = xl if wr is None else _lin(x, wr, br)
    return gatv2_core(xl, xr, edge_index, att, bias, heads, concat, negative_slope, add_self_loops, full, pos)


def dense_gatv2(x, edge_index, wl, bl, wr, br, att, bias, heads, concat=True, negative_slope=0.2, add_self_loops=True):
    """The dense form: cnt[i, j] = number of edges j -> i (diagonal forced to 1 with ``add_self_loops``), softmax over j of
    cnt * exp(z) per head."""
    n = x.shape[0]
    C = wl.shape[0] // heads
    xl = _lin(x, wl, bl).view(n, heads, C)
    xr = xl if wr is None else _lin(x, wr, br).view(n, heads, C)
    cnt = torch.zeros((n, n), dtype=x.dtype)
    cnt.index_put_((edge_index[1], edge_index[0]), torch.ones(edge_index.shape[1], dtype=x.dtype), accumulate=True)
    if add_self_loops:
        cnt.fill_diagonal_(1.0)
    u = xl.unsqueeze(0) + xr.unsqueeze(1)                                              # [i, j, h, c]
    z = torch.einsum("ijhc,hc->ijh", torch.maximum(u, torch.zeros_like(u)) + negative_slope * torch.minimum(u, torch.zeros_like(u)),
                     att.view(heads, C))
    mask = (cnt > 0).unsqueeze(-1)
    m = torch.where(mask, z, torch.full_like(z, -math.inf)).amax(1, keepdim=True).detach()
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))                         # (a row without entries)
    e = torch.where(mask, cnt.unsqueeze(-1) * torch.exp(torch.where(mask, z - m, torch.zeros_like(z))), torch.zeros_like(z))
    den = e.sum(1, keepdim=True)
    alpha = e / torch.where(den > 0, den, torch.ones_like(den))
    out = torch.einsum("ijh,jhc->ihc", alpha, xl)
    out = out.reshape(n, heads * C) if concat else out.mean(1)
    if bias is not None:
        out = out + bias
    return out


class GATv2ConvRef(nn.Module):
    """Edge-list reference with PyG's parameter names and shapes (``share_weights``: ``lin_r`` IS ``lin_l``)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, add_self_loops=True, bias=True,
                 share_weights=False, dtype=torch.float64):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.add_self_loops = concat, negative_slope, add_self_loops
        self.share_weights = share_weights
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=bias, dtype=dtype)
        self.lin_r = self.lin_l if share_weights else nn.Linear(in_channels, heads * out_channels, bias=bias, dtype=dtype)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels, dtype=dtype))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels, dtype=dtype)) if bias else None
        a, b = math.sqrt(6.0 / (in_channels + heads * out_channels)), math.sqrt(6.0 / (heads + out_channels))
        with torch.no_grad():
            self.lin_l.weight.uniform_(-a, a)
            self.lin_r.weight.uniform_(-a, a)
            self.att.uniform_(-b, b)

    def load_from(self, conv):
        """Copy the parameters of a ``GATv2Conv`` (or another reference) into this one, in this one's dtype."""
        with torch.no_grad():
            for mine, theirs in ((self.lin_l, conv.lin_l),) if self.share_weights else ((self.lin_l, conv.lin_l), (self.lin_r, conv.lin_r)):
                mine.weight.copy_(theirs.weight.detach().cpu())
                if mine.bias is not None:
                    mine.bias.copy_(theirs.bias.detach().cpu())
            self.att.copy_(conv.att.detach().cpu())
            if self.bias is not None:
                self.bias.copy_(conv.bias.detach().cpu())
        return self

    def forward(self, x, edge_index, full=False, pos=None):
        share = self.share_weights
        return gatv2_edge_list(x, edge_index, self.lin_l.weight, self.lin_l.bias, None if share else self.lin_r.weight,
                               None if share else self.lin_r.bias, self.att, self.bias, self.heads, self.concat,
                               self.negative_slope, self.add_self_loops, full=full, pos=pos)

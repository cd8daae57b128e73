"""TEST-SIDE REFERENCE for TransformerConv: two independent restatements of torch_geometric 2.2.0's TransformerConv (int
``in_channels``, no edge features, no dropout) in plain torch, float64 by default, differentiable.  Written from the published
source from memory -- PyG cannot be installed here, so this could not be checked against it.

* ``transformer_core`` / ``transformer_edge_list`` / ``TransformerConvRef`` -- the edge-list form PyG itself uses: per-edge
  ``z = Q[i] . K[j] / sqrt(C)``, a scatter softmax over the edges of each target (``index_add_``), a scatter sum of the weighted
  value rows.  No self loops are added; duplicate edges are separate edges; an explicit loop is an ordinary edge.
* ``dense_transformer`` -- a dense [N, N, heads] masked softmax whose multiplicities come from an accumulated adjacency matrix.

Parameters are passed as ``p = (wq, bq, wk, bk, wv, bv, ws, bs, wb)``: ``ws`` None = ``root_weight=False``; ``bs`` None =
``bias=False``; ``wb`` ([1, 3 * width]) None = no ``beta`` gate.  ``edge_index`` row 0 = source j, row 1 = target i."""
import math

import torch
import torch.nn as nn


def _lin(x, w, b):
    y = x @ w.t()
    return y if b is None else y + b


def _finish(m, x, ws, bs, wb):
    """The skip term and the gate on the aggregate ``m`` [N, width]."""
    if ws is None:
        return m
    x_r = _lin(x, ws, bs)
    if wb is None:
        return m + x_r
    b = torch.sigmoid(torch.cat([m, x_r, m - x_r], dim=-1) @ wb.t())
    return b * x_r + (1 - b) * m


def transformer_core(q, k, v, edge_index, heads, concat=True, full=False):
    """The attention part of the edge-list form from ``q`` / ``k`` / ``v`` [N, heads * C] -> m.  ``full``: -> (m, dict(src, dst, z,
    alpha)); ``z`` ([E, heads]) keeps its gradient."""
    n = q.shape[0]
    C = q.shape[1] // heads
    q3, k3, v3 = q.view(n, heads, C), k.view(n, heads, C), v.view(n, heads, C)
    src, dst = edge_index[0], edge_index[1]
    z = (q3[dst] * k3[src]).sum(-1) / math.sqrt(C)
    if full and z.requires_grad:
        z.retain_grad()
    mx = torch.full((n, heads), -math.inf, dtype=z.dtype).scatter_reduce(0, dst.view(-1, 1).expand(-1, heads), z.detach(), "amax")
    ex = torch.exp(z - mx[dst])
    den = torch.zeros((n, heads), dtype=z.dtype).index_add_(0, dst, ex)
    alpha = ex / den[dst]
    m = torch.zeros((n, heads, C), dtype=z.dtype).index_add_(0, dst, alpha.unsqueeze(-1) * v3[src])
    m = m.reshape(n, heads * C) if concat else m.mean(1)
    if full:
        return m, dict(src=src, dst=dst, z=z, alpha=alpha)
    return m


def transformer_edge_list(x, edge_index, wq, bq, wk, bk, wv, bv, ws, bs, wb, heads, concat=True, full=False):
    out = transformer_core(_lin(x, wq, bq), _lin(x, wk, bk), _lin(x, wv, bv), edge_index, heads, concat, full)
    if full:
        return _finish(out[0], x, ws, bs, wb), out[1]
    return _finish(out, x, ws, bs, wb)


def dense_transformer(x, edge_index, wq, bq, wk, bk, wv, bv, ws, bs, wb, heads, concat=True):
    """The dense form: cnt[i, j] = number of edges j -> i, softmax over j of cnt * exp(z) per head; a row without entries is 0."""
    n = x.shape[0]
    C = wq.shape[0] // heads
    q, k, v = (_lin(x, w, b).view(n, heads, C) for w, b in ((wq, bq), (wk, bk), (wv, bv)))
    cnt = torch.zeros((n, n), dtype=x.dtype)
    cnt.index_put_((edge_index[1], edge_index[0]), torch.ones(edge_index.shape[1], dtype=x.dtype), accumulate=True)
    z = torch.einsum("ihc,jhc->ijh", q, k) / math.sqrt(C)
    mask = (cnt > 0).unsqueeze(-1)
    mx = torch.where(mask, z, torch.full_like(z, -math.inf)).amax(1, keepdim=True).detach()
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))                     # (a row without entries)
    e = torch.where(mask, cnt.unsqueeze(-1) * torch.exp(torch.where(mask, z - mx, torch.zeros_like(z))), torch.zeros_like(z))
    den = e.sum(1, keepdim=True)
    alpha = e / torch.where(den > 0, den, torch.ones_like(den))
    m = torch.einsum("ijh,jhc->ihc", alpha, v)
    m = m.reshape(n, heads * C) if concat else m.mean(1)
    return _finish(m, x, ws, bs, wb)


class TransformerConvRef(nn.Module):
    """Edge-list reference with PyG's parameter names and shapes."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, bias=True, root_weight=True,
                 dtype=torch.float64):
        super().__init__()
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.root_weight, self.beta = concat, root_weight, beta and root_weight
        hc = heads * out_channels
        sw = hc if concat else out_channels
        self.lin_key = nn.Linear(in_channels, hc, dtype=dtype)
        self.lin_query = nn.Linear(in_channels, hc, dtype=dtype)
        self.lin_value = nn.Linear(in_channels, hc, dtype=dtype)
        self.lin_skip = nn.Linear(in_channels, sw, bias=bias, dtype=dtype)
        self.lin_beta = nn.Linear(3 * sw, 1, bias=False, dtype=dtype) if self.beta else None
        self.lin_edge = None

    def load_from(self, conv):
        """Copy the parameters of a ``TransformerConv`` (or another reference) into this one, in this one's dtype."""
        with torch.no_grad():
            for name in ("lin_key", "lin_query", "lin_value", "lin_skip", "lin_beta"):
                mine, theirs = getattr(self, name), getattr(conv, name)
                if mine is None:
                    continue
                mine.weight.copy_(theirs.weight.detach().cpu())
                if mine.bias is not None:
                    mine.bias.copy_(theirs.bias.detach().cpu())
        return self

    def params(self):
        root = self.root_weight
        return (self.lin_query.weight, self.lin_query.bias, self.lin_key.weight, self.lin_key.bias, self.lin_value.weight,
                self.lin_value.bias, self.lin_skip.weight if root else None, self.lin_skip.bias if root else None,
                self.lin_beta.weight if self.beta else None)

    def forward(self, x, edge_index, full=False):
        return transformer_edge_list(x, edge_index, *self.params(), self.heads, self.concat, full=full)

"""TEST-SIDE REFERENCE for EdgeConv: two independent restatements of torch_geometric 2.2.0's EdgeConv (max aggregation) in plain
torch, float64 by default, differentiable.

* ``edgeconv_edge_list`` / ``EdgeConvRef`` -- the edge-list form PyG itself uses: the FULL edge function ``nn`` (activations
  included) on ``cat[x_i, x_j - x_i]`` per edge, then a segment maximum over the edges of each target, 0 for a target without
  edges.  No self loops are added; duplicate edges and explicit loops are ordinary edges.
* ``dense_edgeconv`` -- an [N, N] mask and a maximum over it.

``winners_and_gaps`` gives, for a matrix B [N, C] and the edge structure, the smallest source id that attains each (i, c)'s
maximum and the gap to the runner-up among the row's OTHER sources: the conditioning of the arg-max.

``edge_index`` row 0 = source j, row 1 = target i."""
import copy

import torch
import torch.nn as nn


def edgeconv_edge_list(x, edge_index, fn):
    """The edge-list form.  ``fn``: the edge function, a module in x's dtype."""
    n = x.shape[0]
    src, dst = edge_index[0], edge_index[1]
    msg = fn(torch.cat([x[dst], x[src] - x[dst]], 1))
    idx = dst.view(-1, 1).expand(-1, msg.shape[1])
    return torch.zeros((n, msg.shape[1]), dtype=x.dtype).scatter_reduce(0, idx, msg, "amax", include_self=False)


def dense_edgeconv(x, edge_index, fn):
    """The dense form: z[i, j, :] = fn(cat[x_i, x_j - x_i]) for every pair, a maximum over the j with an edge j -> i."""
    n = x.shape[0]
    mask = torch.zeros((n, n), dtype=torch.bool)
    mask[edge_index[1], edge_index[0]] = True
    xi = x.unsqueeze(1).expand(n, n, -1)
    z = fn(torch.cat([xi, x.unsqueeze(0) - xi], 2).reshape(n * n, -1)).reshape(n, n, -1)
    z = torch.where(mask.unsqueeze(-1), z, torch.full_like(z, -float("inf")))
    has = mask.any(1, keepdim=True)
    return torch.where(has, z.amax(1), torch.zeros((), dtype=x.dtype))


def as_dtype(fn, dtype):
    """A deep copy of the edge function in ``dtype`` (its parameters are new leaves)."""
    return copy.deepcopy(fn).to("cpu").to(dtype)


class EdgeConvRef(nn.Module):
    """Edge-list reference with PyG's attribute name: the edge function sits under ``nn``."""

    def __init__(self, fn, dtype=torch.float64):
        super().__init__()
        self.nn = as_dtype(fn, dtype)

    def forward(self, x, edge_index):
        return edgeconv_edge_list(x, edge_index, self.nn)


def winners_and_gaps(b, edge_index, n):
    """-> (arg int64 [n, C], gap [n, C], empty bool [n]).  arg[i, c]: the smallest source j among the edges j -> i with
    b[j, c] = max; -1 for a target without edges.  gap[i, c]: that maximum minus the largest b[j', c] over the OTHER distinct
    sources of i (inf when there is none): 0 when two different sources tie."""
    C = b.shape[1]
    key = torch.unique(edge_index[1] * n + edge_index[0])       # coalesced, sorted by (target, source)
    dst, src = key // n, key % n
    idx = dst.view(-1, 1).expand(-1, C)
    vals = b[src]
    neg = torch.full((n, C), -float("inf"), dtype=b.dtype)
    mx = neg.scatter_reduce(0, idx, vals, "amax")
    big = torch.iinfo(torch.int64).max
    cand = torch.where(vals == mx[dst], src.view(-1, 1).expand(-1, C), torch.full((), big, dtype=torch.int64))
    arg = torch.full((n, C), big, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin")
    others = torch.where(src.view(-1, 1) == arg[dst], torch.full((), -float("inf"), dtype=b.dtype), vals)
    second = neg.scatter_reduce(0, idx, others, "amax")
    empty = torch.ones(n, dtype=torch.bool)
    empty[dst] = False
    arg[empty] = -1
    gap = mx - second
    gap[empty] = float("inf")
    return arg, gap, empty

"""TEST-SIDE REFERENCE for SAGEConv: two independent restatements of torch_geometric 2.2.0's SAGEConv (mean / add / max / min
aggregation, or a list of them concatenated in list order) in plain torch, float64 by default, differentiable.

* ``aggregate_edge_list`` / ``SAGEConvRef`` -- the edge-list form PyG itself uses: ``x[src]`` per edge, then ``index_add_`` (add,
  mean: divided by the number of edges into the target) or ``scatter_reduce`` (amax / amin) over the edges of each target, 0 for a
  target without edges.  No self loops are added; duplicate edges and explicit loops are ordinary edges.
* ``aggregate_dense`` -- an [N, N] matrix of edge counts and a masked [N, N, C] tensor, for small N.

``out = lin_l(cat_k aggr_k) + lin_r(x)``, then (``normalize``) ``F.normalize(out, p=2, dim=-1)``.

``extremum_winners`` gives, for every max / min output (i, c), the smallest source id that attains it and the gap to the
runner-up among the row's OTHER sources: the conditioning of the arg-max / arg-min.

``edge_index`` row 0 = source j, row 1 = target i."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from edgeconv_ref import winners_and_gaps

AGGRS = ("mean", "add", "max", "min")


def canonical(aggr):
    """The aggregators as a tuple of names out of ``AGGRS`` (``"sum"`` is ``"add"``)."""
    return tuple("add" if a == "sum" else a for a in ([aggr] if isinstance(aggr, str) else aggr))


def aggregate_edge_list(x, edge_index, aggr):
    """One aggregator, the edge-list form -> [N, C]."""
    n, C = x.shape
    src, dst = edge_index[0], edge_index[1]
    msg = x[src]
    if aggr in ("add", "mean"):
        out = torch.zeros((n, C), dtype=x.dtype).index_add_(0, dst, msg)
        if aggr == "mean":
            cnt = torch.zeros(n, dtype=x.dtype).index_add_(0, dst, torch.ones(len(dst), dtype=x.dtype))
            out = out / cnt.clamp(min=1).view(-1, 1)
        return out
    idx = dst.view(-1, 1).expand(-1, C)
    return torch.zeros((n, C), dtype=x.dtype).scatter_reduce(0, idx, msg, "amax" if aggr == "max" else "amin", include_self=False)


def aggregate_dense(x, edge_index, aggr):
    """One aggregator, the dense form: cnt[i, j] = the number of edges j -> i."""
    n = x.shape[0]
    cnt = torch.zeros((n, n), dtype=x.dtype)
    cnt.index_put_((edge_index[1], edge_index[0]), torch.ones(edge_index.shape[1], dtype=x.dtype), accumulate=True)
    if aggr in ("add", "mean"):
        out = cnt @ x
        return out / cnt.sum(1).clamp(min=1).view(-1, 1) if aggr == "mean" else out
    mask = (cnt > 0).unsqueeze(-1)
    fill = -float("inf") if aggr == "max" else float("inf")
    z = torch.where(mask, x.unsqueeze(0).expand(n, n, -1), torch.full((), fill, dtype=x.dtype))
    z = z.amax(1) if aggr == "max" else z.amin(1)
    return torch.where(mask.any(1), z, torch.zeros((), dtype=x.dtype))


def sage_forward(x, edge_index, aggr, wl, bl, wr, normalize=False, form=aggregate_edge_list, on_block=None):
    """SAGEConv's arithmetic from explicit parameters (``bl`` / ``wr`` may be None).  ``on_block(name, block)``: called with every
    aggregated [N, in] block before the concatenation (a test registers gradient hooks there)."""
    blocks = [form(x, edge_index, k) for k in canonical(aggr)]
    if on_block is not None:
        for k, b in zip(canonical(aggr), blocks):
            on_block(k, b)
    a = torch.cat(blocks, 1)
    out = a @ wl.t()
    if bl is not None:
        out = out + bl
    if wr is not None:
        out = out + x @ wr.t()
    return F.normalize(out, p=2.0, dim=-1) if normalize else out


class _Lin(nn.Module):
    def __init__(self, cin, cout, bias, dtype):
        super().__init__()
        a = 1.0 / math.sqrt(cin)
        self.weight = nn.Parameter((torch.rand(cout, cin, dtype=dtype) * 2 - 1) * a)
        if bias:
            self.bias = nn.Parameter((torch.rand(cout, dtype=dtype) * 2 - 1) * a)
        else:
            self.register_parameter("bias", None)


class SAGEConvRef(nn.Module):
    """Edge-list reference with PyG's parameter names: ``lin_l.weight`` [out, k * in], ``lin_l.bias`` [out] (only with
    ``bias``), ``lin_r.weight`` [out, in] (the attribute is absent with ``root_weight=False``)."""

    def __init__(self, in_channels, out_channels, aggr="mean", normalize=False, root_weight=True, bias=True, dtype=torch.float64):
        super().__init__()
        self.aggr, self.normalize, self.root_weight, self.on_block = aggr, normalize, root_weight, None
        self.lin_l = _Lin(len(canonical(aggr)) * in_channels, out_channels, bias, dtype)
        if root_weight:
            self.lin_r = _Lin(in_channels, out_channels, False, dtype)

    def forward(self, x, edge_index):
        return sage_forward(x, edge_index, self.aggr, self.lin_l.weight, self.lin_l.bias,
                            self.lin_r.weight if self.root_weight else None, self.normalize, on_block=self.on_block)


def extremum_winners(x, edge_index, n, aggr):
    """-> (arg int64 [n, C], gap [n, C] >= 0, empty bool [n]) of the max (min) of x's rows over each target's sources: the smallest
    source id attaining it (-1 for a target without edges) and the distance to the runner-up among the OTHER distinct sources."""
    return winners_and_gaps(x if aggr == "max" else -x, edge_index, n)

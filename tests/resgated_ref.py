"""TEST-SIDE REFERENCE for ResGatedGraphConv: a restatement of torch_geometric 2.2.0's ResGatedGraphConv (int ``in_channels``,
``act=Sigmoid()``, ``aggr="add"``) in plain torch, float64 by default, differentiable.  Written from the published source from
memory -- PyG cannot be installed here, so this could not be checked against it.

* ``resgated_core(k, q, v, edge_index)`` -- the edge-list form PyG itself uses: per edge j -> i the per-channel gate
  ``sigmoid(k[i] + q[j])``, the product with ``v[j]`` and a scatter sum over the targets (``index_add_``) over the RAW edge list.
  No self loops are added; duplicate edges are separate edges; an explicit loop is an ordinary edge.
* ``resgated_edge_list`` / ``ResGatedGraphConvRef`` -- the operator around it.

Parameters are passed as ``p = (wk, bk, wq, bq, wv, bv, ws, bias)``: ``ws`` None = ``root_weight=False``; ``bias`` None =
``bias=False``.  ``edge_index`` row 0 = source j, row 1 = target i."""
import torch
import torch.nn as nn


def resgated_core(k, q, v, edge_index):
    """sum_{j -> i} sigmoid(k[i] + q[j]) * v[j] from ``k`` / ``q`` / ``v`` [N, C] -> [N, C]."""
    src, dst = edge_index[0], edge_index[1]
    gate = torch.sigmoid(k.index_select(0, dst) + q.index_select(0, src))
    return torch.zeros_like(v).index_add_(0, dst, gate * v.index_select(0, src))


def resgated_edge_list(x, edge_index, wk, bk, wq, bq, wv, bv, ws, bias):
    out = resgated_core(x @ wk.t() + bk, x @ wq.t() + bq, x @ wv.t() + bv, edge_index)
    if ws is not None:
        out = out + x @ ws.t()
    if bias is not None:
        out = out + bias
    return out


class ResGatedGraphConvRef(nn.Module):
    """Edge-list reference with PyG's parameter names and shapes."""

    def __init__(self, in_channels, out_channels, root_weight=True, bias=True, dtype=torch.float64):
        super().__init__()
        self.in_channels, self.out_channels, self.root_weight = in_channels, out_channels, root_weight
        self.lin_key = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.lin_query = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.lin_value = nn.Linear(in_channels, out_channels, dtype=dtype)
        self.lin_skip = nn.Linear(in_channels, out_channels, bias=False, dtype=dtype) if root_weight else None
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels, dtype=dtype))
        else:
            self.register_parameter("bias", None)

    def load_from(self, conv):
        """Copy the parameters of a ``ResGatedGraphConv`` (or another reference) into this one, in this one's dtype."""
        with torch.no_grad():
            for name in ("lin_key", "lin_query", "lin_value", "lin_skip"):
                mine, theirs = getattr(self, name), getattr(conv, name)
                if mine is None:
                    continue
                mine.weight.copy_(theirs.weight.detach().cpu())
                if mine.bias is not None:
                    mine.bias.copy_(theirs.bias.detach().cpu())
            if self.bias is not None:
                self.bias.copy_(conv.bias.detach().cpu())
        return self

    def params(self):
        return (self.lin_key.weight, self.lin_key.bias, self.lin_query.weight, self.lin_query.bias, self.lin_value.weight,
                self.lin_value.bias, self.lin_skip.weight if self.root_weight else None, self.bias)

    def forward(self, x, edge_index):
        return resgated_edge_list(x, edge_index, *self.params())

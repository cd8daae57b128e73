"""TEST-SIDE REFERENCE for CGConv: two independent restatements of torch_geometric 2.2.0's CGConv (int ``channels``) in plain torch,
float64 by default, differentiable.  Written from the published source from memory -- PyG is not installed here and cannot be, so
this could not be checked against it.

    z_ij = cat[x_i, x_j, e_ij],   out_i = x_i + sum_{j -> i} sigmoid(lin_f(z_ij)) * softplus(lin_s(z_ij))

(``aggr="mean"``: the sum divided by the number of edges into i; with ``batch_norm`` the sum goes through BatchNorm1d before x_i is
added).  No self loops are added; duplicate edges are separate edges with their own attributes; an explicit loop is an ordinary edge.

* ``cg_messages_edge_list`` -- the edge-list form PyG itself uses: the concatenation per edge, two ``F.linear``, ``F.softplus`` and a
  scatter sum over the targets (``index_add_``) over the RAW edge list.
* ``cg_messages_dense`` -- a dense [N, N] form for graphs WITHOUT duplicate edges: every pair (i, j) gets its message, an adjacency
  mask selects the edges.  It shares nothing with the edge-list form but the formula.
* ``cg_core`` -- the graph part alone from the blocks the kernels take (Af, As, Bf, Bs, the attributes and Ef, Es), edge-list form.
* ``CGConvRef`` -- the operator with PyG's parameter names and shapes.

``edge_index`` row 0 = source j, row 1 = target i.  ``lin_f.weight`` / ``lin_s.weight``: [C, 2 C + dim], columns x_i | x_j | e_ij."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def _mean_scale(dst, n, dtype):
    cnt = torch.zeros(n, dtype=dtype).index_add_(0, dst, torch.ones(dst.shape[0], dtype=dtype))
    return cnt.clamp(min=1.0).unsqueeze(1)


def cg_messages_edge_list(x, edge_index, edge_attr, wf, bf, ws, bs, aggr="add"):
    """The aggregated messages [N, C] (without the residual).  ``edge_attr``: [E, dim] or None; ``bf`` / ``bs``: [C] or None."""
    src, dst = edge_index[0], edge_index[1]
    parts = [x.index_select(0, dst), x.index_select(0, src)] + ([] if edge_attr is None else [edge_attr])
    z = torch.cat(parts, 1)
    msg = torch.sigmoid(F.linear(z, wf, bf)) * F.softplus(F.linear(z, ws, bs))
    out = torch.zeros_like(x).index_add_(0, dst, msg)
    return out / _mean_scale(dst, x.shape[0], x.dtype) if aggr == "mean" else out


def cg_messages_dense(x, edge_index, edge_attr, wf, bf, ws, bs, aggr="add"):
    """The same from dense [N, N] arrays; the graph must not have duplicate edges."""
    n, C = x.shape
    src, dst = edge_index[0], edge_index[1]
    mask = torch.zeros((n, n), dtype=x.dtype)
    mask[dst, src] += 1.0
    assert float(mask.max()) <= 1.0, "the dense form takes graphs without duplicate edges"
    lin = lambda w, b: ((x @ w[:, :C].t()).unsqueeze(1) + (x @ w[:, C:2 * C].t()).unsqueeze(0) + (0.0 if b is None else b))
    pf, ps = lin(wf, bf), lin(ws, bs)                              # [N (target), N (source), C]
    if edge_attr is not None:
        dense = torch.zeros((n, n, edge_attr.shape[1]), dtype=x.dtype)
        dense[dst, src] = edge_attr
        pf, ps = pf + dense @ wf[:, 2 * C:].t(), ps + dense @ ws[:, 2 * C:].t()
    gate = 1.0 / (1.0 + torch.exp(-pf))
    soft = torch.log1p(torch.exp(-ps.abs())) + ps.clamp(min=0.0)
    out = (mask.unsqueeze(-1) * gate * soft).sum(1)
    return out / mask.sum(1).clamp(min=1.0).unsqueeze(1) if aggr == "mean" else out


def cg_core(af, as_, bf, bs, edge_index, edge_attr=None, ef=None, es=None, aggr="add"):
    """sum_{t: j -> i} sigmoid(af[i] + bf[j] + a_t ef) * softplus(as_[i] + bs[j] + a_t es) (``ef`` / ``es``: [dim, C], the edge
    weights transposed, as the kernels take them) -> [N, C]."""
    src, dst = edge_index[0], edge_index[1]
    pf = af.index_select(0, dst) + bf.index_select(0, src)
    ps = as_.index_select(0, dst) + bs.index_select(0, src)
    if edge_attr is not None:
        pf, ps = pf + edge_attr @ ef, ps + edge_attr @ es
    out = torch.zeros_like(af).index_add_(0, dst, torch.sigmoid(pf) * F.softplus(ps))
    return out / _mean_scale(dst, af.shape[0], af.dtype) if aggr == "mean" else out


class CGConvRef(nn.Module):
    """Edge-list reference with PyG's parameter names and shapes."""

    def __init__(self, channels, dim=0, aggr="add", batch_norm=False, bias=True, dtype=torch.float64):
        super().__init__()
        self.channels, self.dim, self.aggr = channels, dim, aggr
        self.lin_f = nn.Linear(2 * channels + dim, channels, bias=bias, dtype=dtype)
        self.lin_s = nn.Linear(2 * channels + dim, channels, bias=bias, dtype=dtype)
        self.bn = nn.BatchNorm1d(channels, dtype=dtype) if batch_norm else None

    def load_from(self, conv):
        """Copy the parameters (and the BatchNorm buffers) of a ``CGConv`` (or another reference) into this one, in this one's dtype."""
        with torch.no_grad():
            for name in ("lin_f", "lin_s"):
                mine, theirs = getattr(self, name), getattr(conv, name)
                mine.weight.copy_(theirs.weight.detach().cpu())
                if mine.bias is not None:
                    mine.bias.copy_(theirs.bias.detach().cpu())
            if self.bn is not None:
                for k, v in conv.bn.state_dict().items():
                    self.bn.state_dict()[k].copy_(v.detach().cpu())
        return self

    def forward(self, x, edge_index, edge_attr=None):
        a = None if edge_attr is None else edge_attr.to(x.dtype)
        out = cg_messages_edge_list(x, edge_index, a, self.lin_f.weight, self.lin_f.bias, self.lin_s.weight, self.lin_s.bias, self.aggr)
        if self.bn is not None:
            out = self.bn(out)
        return out + x

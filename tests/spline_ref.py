"""TEST-SIDE REFERENCE for SplineConv: two independent restatements of torch_geometric 2.2.0's SplineConv (SplineCNN; int
``in_channels``, ``degree=1``, mean or add aggregation) in plain torch, float64 by default, differentiable w.r.t. the features and
the parameters (not the pseudo-coordinates).  Written from the published sources (PyG and its ``torch_spline_conv`` extension)
from memory -- neither can be installed here.

* ``spline_basis`` / ``spline_edge_list`` / ``SplineConvRef`` -- the edge-list form PyG itself uses: per edge the S = 2^dim basis
  products and weight-block indices of its pseudo-coordinates, the S selected blocks of the projected source row mixed by them, a
  scatter sum (or mean) over the edges of each target, then the root term and the bias.  No self loops are added; duplicate edges
  are separate edges with their own pseudo-coordinates.
* ``dense_spline`` -- a dense [N, N, K] form filled by plain Python loops, one edge and one corner at a time: the basis weights of
  all edges j -> i accumulated into one table, one contraction.

``edge_index`` row 0 = source j, row 1 = target i; ``weight``: [K, in, out] with K = prod(kernel_size), the first pseudo-coordinate
varying fastest in the block index; ``root``: [out, in] or None; ``bias``: [out] or None."""
import math

import torch
import torch.nn as nn


def sizes(dim, kernel_size, is_open_spline):
    ks = [kernel_size] * dim if isinstance(kernel_size, int) else list(kernel_size)
    op = [is_open_spline] * dim if isinstance(is_open_spline, bool) else list(is_open_spline)
    assert len(ks) == dim and len(op) == dim
    return ks, [bool(o) for o in op]


def spline_basis(attr, kernel_size, is_open_spline):
    """-> (b [E, S] in attr's dtype, k [E, S] int64): for s in [0, 2^dim) with bits s_d,
    v_d = attr[:, d] (kernel_size[d] - open[d]), b = prod_d (s_d ? frac(v_d) : 1 - frac(v_d)),
    k = sum_d ((floor(v_d) + s_d) mod kernel_size[d]) prod_{d' < d} kernel_size[d']."""
    E, dim = attr.shape
    ks, op = sizes(dim, kernel_size, is_open_spline)
    S = 1 << dim
    b = torch.ones((E, S), dtype=attr.dtype)
    k = torch.zeros((E, S), dtype=torch.int64)
    bits = torch.arange(S)
    stride = 1
    for d in range(dim):
        v = attr[:, d] * (ks[d] - int(op[d]))
        fl = torch.floor(v)
        fr = (v - fl).unsqueeze(1)
        up = ((bits >> d) & 1).unsqueeze(0)                      # [1, S]
        b = b * torch.where(up.bool(), fr, 1 - fr)
        k = k + torch.remainder(fl.long().unsqueeze(1) + up, ks[d]) * stride
        stride *= ks[d]
    return b, k


def spline_edge_list(x, edge_index, attr, weight, root, bias, kernel_size, is_open_spline, aggr="mean"):
    n = x.shape[0]
    K, _, C = weight.shape
    hf = torch.einsum("ni,kio->nko", x, weight)
    src, dst = edge_index[0], edge_index[1]
    b, k = spline_basis(attr.to(x.dtype), kernel_size, is_open_spline)
    assert int(k.max()) < K
    blocks = hf[src.unsqueeze(1), k]                             # [E, S, C]: only the selected blocks
    msg = (b.unsqueeze(-1) * blocks).sum(1)
    out = torch.zeros((n, C), dtype=x.dtype).index_add_(0, dst, msg)
    if aggr == "mean":
        cnt = torch.zeros(n, dtype=x.dtype).index_add_(0, dst, torch.ones(len(dst), dtype=x.dtype))
        out = out / cnt.clamp(min=1.0).unsqueeze(-1)
    else:
        assert aggr == "add"
    if root is not None:
        out = out + x @ root.t()
    if bias is not None:
        out = out + bias
    return out


def dense_spline(x, edge_index, attr, weight, root, bias, kernel_size, is_open_spline, aggr="mean"):
    """The dense form: T[i, j, k] = sum over the edges j -> i and their corners s with block k of b_{t,s}, filled one edge and one
    corner at a time in Python floats (float64); out[i] = sum_j sum_k T[i, j, k] Hf[j, k] / n_i + x_i root^T + bias."""
    n = x.shape[0]
    K, _, C = weight.shape
    E, dim = attr.shape
    ks, op = sizes(dim, kernel_size, is_open_spline)
    assert math.prod(ks) == K
    T = torch.zeros((n, n, K), dtype=torch.float64)
    cnt = torch.zeros(n, dtype=torch.float64)
    a = attr.double().tolist()
    for t in range(E):
        j, i = int(edge_index[0, t]), int(edge_index[1, t])
        cnt[i] += 1
        for s in range(1 << dim):
            w, blk, stride = 1.0, 0, 1
            for d in range(dim):
                v = a[t][d] * (ks[d] - (1 if op[d] else 0))
                lo = math.floor(v)
                f = v - lo
                up = (s >> d) & 1
                w *= f if up else 1.0 - f
                blk += ((lo + up) % ks[d]) * stride              # (Python's % is the non-negative modulo)
                stride *= ks[d]
            T[i, j, blk] += w
    hf = torch.stack([x @ weight[k] for k in range(K)], 1)       # [n, K, C]
    out = torch.einsum("ijk,jkc->ic", T.to(x.dtype), hf)
    if aggr == "mean":
        out = out / torch.where(cnt > 0, cnt, torch.ones_like(cnt)).to(x.dtype).unsqueeze(1)
    if root is not None:
        out = out + torch.einsum("ni,ci->nc", x, root)
    if bias is not None:
        out = out + bias
    return out


class SplineConvRef(nn.Module):
    """Edge-list reference with PyG's parameter names and shapes."""

    def __init__(self, in_channels, out_channels, dim, kernel_size, is_open_spline=True, aggr="mean", root_weight=True, bias=True,
                 dtype=torch.float64):
        super().__init__()
        ks, op = sizes(dim, kernel_size, is_open_spline)
        self.in_channels, self.out_channels, self.dim, self.kernel_size, self.is_open_spline, self.aggr = \
            in_channels, out_channels, dim, ks, op, aggr
        K = math.prod(ks)
        self.weight = nn.Parameter(torch.empty(K, in_channels, out_channels, dtype=dtype))
        self.lin = nn.Linear(in_channels, out_channels, bias=False, dtype=dtype) if root_weight else None
        self.bias = nn.Parameter(torch.zeros(out_channels, dtype=dtype)) if bias else None
        with torch.no_grad():
            a = 1.0 / math.sqrt(in_channels * K)
            self.weight.uniform_(-a, a)
            if root_weight:
                a = 1.0 / math.sqrt(in_channels)
                self.lin.weight.uniform_(-a, a)

    def load_from(self, conv):
        """Copy the parameters of a ``SplineConv`` (or another reference) into this one, in this one's dtype."""
        with torch.no_grad():
            self.weight.copy_(conv.weight.detach().cpu())
            if self.lin is not None:
                self.lin.weight.copy_(conv.lin.weight.detach().cpu())
            if self.bias is not None:
                self.bias.copy_(conv.bias.detach().cpu())
        return self

    def forward(self, x, edge_index, edge_attr):
        return spline_edge_list(x, edge_index, edge_attr, self.weight, None if self.lin is None else self.lin.weight, self.bias,
                                self.kernel_size, self.is_open_spline, self.aggr)

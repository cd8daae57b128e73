"""Test-side reference for ``edge_weight``: dense restatement of ``torch_geometric.nn.conv.gcn_conv.gcn_norm`` and ``GCNConv``
2.2.0 (and of ChebConv's weighted ``S``) in plain torch on the CPU, differentiable w.r.t. everything including ``edge_weight``
(autograd through the dense matrix gives every gradient).  Test infrastructure only.

Written from the published PyG source from memory: PyG is not installed here and cannot be, so this restatement could not be
checked against it.  The formulas:

``gcn_norm(edge_index, edge_weight, N, improved, add_self_loops)``: ``w_e = 1`` without ``edge_weight``;
``fill = 2 if improved else 1``.  With ``add_self_loops`` (``add_remaining_self_loops``): explicit self loops are removed from
the edge list; every node gets ONE loop of weight ``fill``, except that a node with explicit loops keeps the weight of its LAST
explicit loop in input order.  ``deg_i = sum of w_e over the entries with target i`` (loop included), ``s_i = deg_i^-1/2`` with
``inf -> 0``, entry value ``s_i w_e s_j`` at ``A[i = target, j = source]``.  Duplicate edges each contribute (they add up in the
dense matrix).  ``normalize=False``: no self loops are added and the entry value is ``w_e``, whatever ``add_self_loops`` says.
``GCNConv``: ``Y = A (X W^T) + b``.

ChebConv with weights: self loops removed, ``S = D^-1/2 A_w D^-1/2`` (symmetric weights only, so that the degree over sources
that PyG takes there equals the degree over targets), ``L^ = -(2 / lambda_max) S + (2 / lambda_max - 1) I``."""
import math

import torch
import torch.nn as nn


def dense_gcn_norm(ei, w, n, improved=False, add_self_loops=True, normalize=True, dtype=torch.float64):
    """-> dense [n, n] operator (rows = targets), differentiable w.r.t. ``w`` (None = ones)."""
    src, dst = ei[0].cpu(), ei[1].cpu()
    nnz = src.shape[0]
    w = torch.ones(nnz, dtype=dtype) if w is None else w.to(dtype)
    A = torch.zeros(n, n, dtype=dtype)
    if not normalize:
        return A.index_put((dst, src), w, accumulate=True)
    if add_self_loops:
        fill = 2.0 if improved else 1.0
        loop = src == dst
        keep = ~loop
        A = A.index_put((dst[keep], src[keep]), w[keep], accumulate=True)
        diag = torch.full((n,), fill, dtype=dtype)
        last = {}
        for k in torch.nonzero(loop).flatten().tolist():      # the LAST explicit loop of a node wins
            last[int(src[k])] = k
        if last:
            nodes = torch.tensor(list(last.keys()), dtype=torch.long)
            ks = torch.tensor(list(last.values()), dtype=torch.long)
            diag = diag.index_put((nodes,), w[ks])
        A = A + torch.diag(diag)
    else:
        A = A.index_put((dst, src), w, accumulate=True)
    deg = A.sum(1)
    s = torch.where(deg > 0, deg.clamp(min=1e-300 if dtype == torch.float64 else 1e-30).pow(-0.5), torch.zeros_like(deg))
    return s[:, None] * A * s[None, :]


def dense_s_weighted(ei, w, n, dtype=torch.float64):
    """ChebConv's S for symmetric weights: loops dropped, none added."""
    src, dst = ei[0].cpu(), ei[1].cpu()
    keep = src != dst
    A = torch.zeros(n, n, dtype=dtype).index_put((dst[keep], src[keep]), w.to(dtype)[keep], accumulate=True)
    deg = A.sum(1)
    s = torch.where(deg > 0, deg.clamp(min=1e-300).pow(-0.5), torch.zeros_like(deg))
    return s[:, None] * A * s[None, :]


class GCNConvRef(nn.Module):
    """Parameters ``lin.weight`` [out, in] (Glorot-uniform) and ``bias`` [out] (zeros), as PyG names them."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True):
        super().__init__()
        self.opts = dict(improved=improved, add_self_loops=add_self_loops, normalize=normalize)
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        a = math.sqrt(6.0 / (in_channels + out_channels))
        with torch.no_grad():
            self.lin.weight.uniform_(-a, a)

    def forward(self, x, edge_index, edge_weight=None):
        A = dense_gcn_norm(edge_index, edge_weight, x.shape[0], dtype=x.dtype, **self.opts)
        y = A @ self.lin(x)
        return y if self.bias is None else y + self.bias

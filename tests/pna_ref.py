"""TEST-SIDE REFERENCE for PNAConv: two independent restatements of torch_geometric 2.2.0's PNAConv (towers, single-layer pre / post
MLPs, the aggregators mean / sum / max / min / std / var and the degree scalers) in plain torch, float64 by default, differentiable.

* ``aggregate_edge_list`` / ``PNAConvRef`` -- the edge-list form PyG itself uses: the explicit [E, T, F] messages
  ``pre_nns[t](cat[x_i, x_j])``, then ``index_add_`` / ``scatter_reduce`` over the edges of each target; var = mean(h^2) - mean(h)^2
  (``VarAggregation``), std = ``sqrt(var.clamp(min=1e-5))``, then 0 where that is <= sqrt(1e-5) (``StdAggregation``).  A target
  without edges aggregates to 0.  No self loops are added; duplicate edges and explicit loops are ordinary edges.
* ``aggregate_dense`` -- an [N, N] matrix of edge counts and masked [N, N, T, F] messages, for small N, with a TWO-PASS variance
  (the mean first, then the mean of the squared deviations).

The scalers: with ``d_i = max(in-degree_i, 1)``, ``delta_lin = sum k deg[k] / sum deg`` and ``delta_log = sum log(k + 1) deg[k] /
sum deg``: identity 1, amplification ``log(d + 1) / delta_log``, attenuation ``delta_log / log(d + 1)``, linear ``d / delta_lin``,
inverse_linear ``delta_lin / d``; the concatenation is scaler-major, then aggregator, then F.
``out_t = post_nns[t](cat[x_i, that])``, ``y = lin(cat_t out_t)``.

``extremum_winners`` is sage_ref.py's.  ``edge_index`` row 0 = source j, row 1 = target i."""
import math

import torch
import torch.nn as nn

from sage_ref import extremum_winners  # noqa: F401  (re-exported: the tests take it from here)

AGGRS = ("mean", "sum", "max", "min", "std", "var")
SCALERS = ("identity", "amplification", "attenuation", "linear", "inverse_linear")
STD_FLOOR = 1e-5


def degree_histogram(edge_index, n):
    d = torch.zeros(n, dtype=torch.long).index_add_(0, edge_index[1], torch.ones(edge_index.shape[1], dtype=torch.long))
    return torch.zeros(int(d.max()) + 1, dtype=torch.long).index_add_(0, d, torch.ones(n, dtype=torch.long))


def deltas(deg):
    """(delta_lin, delta_log) of the histogram ``deg``."""
    h = deg.to(torch.float64)
    k = torch.arange(h.numel(), dtype=torch.float64)
    return float((k * h).sum() / h.sum()), float((torch.log(k + 1) * h).sum() / h.sum())


def _std_of(var):
    s = var.clamp(min=STD_FLOOR).sqrt()
    return s.masked_fill(s <= math.sqrt(STD_FLOOR), 0.0)


def aggregate_edge_list(msg, edge_index, n, aggr):
    """One aggregator over the per-edge messages ``msg`` [E, ...] -> [n, ...]."""
    dst = edge_index[1]
    zeros = lambda: torch.zeros((n,) + tuple(msg.shape[1:]), dtype=msg.dtype)
    cnt = torch.zeros(n, dtype=msg.dtype).index_add_(0, dst, torch.ones(len(dst), dtype=msg.dtype)).clamp(min=1)
    cnt = cnt.view((-1,) + (1,) * (msg.dim() - 1))
    if aggr == "sum":
        return zeros().index_add_(0, dst, msg)
    if aggr == "mean":
        return zeros().index_add_(0, dst, msg) / cnt
    if aggr in ("std", "var"):
        mean = zeros().index_add_(0, dst, msg) / cnt
        var = zeros().index_add_(0, dst, msg * msg) / cnt - mean * mean
        return var if aggr == "var" else _std_of(var)
    idx = dst.view((-1,) + (1,) * (msg.dim() - 1)).expand_as(msg)
    return zeros().scatter_reduce(0, idx, msg, "amax" if aggr == "max" else "amin", include_self=False)


def aggregate_dense(msg_of, x_shape, edge_index, n, aggr):
    """One aggregator, the dense form.  ``msg_of(i, j)`` -> the messages [n, n, ...] of every (target, source) pair."""
    cnt = torch.zeros((n, n), dtype=torch.float64)
    cnt.index_put_((edge_index[1], edge_index[0]), torch.ones(edge_index.shape[1], dtype=torch.float64), accumulate=True)
    m = msg_of()                                                 # [n(target), n(source), ...]
    c = cnt.view((n, n) + (1,) * (m.dim() - 2)).to(m.dtype)
    deg = c.sum(1).clamp(min=1)
    if aggr == "sum":
        return (c * m).sum(1)
    if aggr == "mean":
        return (c * m).sum(1) / deg
    if aggr in ("std", "var"):
        mean = (c * m).sum(1) / deg
        var = (c * (m - mean.unsqueeze(1)) ** 2).sum(1) / deg    # two passes
        return var if aggr == "var" else _std_of(var)
    mask = c > 0
    fill = -float("inf") if aggr == "max" else float("inf")
    z = torch.where(mask, m, torch.full((), fill, dtype=m.dtype))
    z = z.amax(1) if aggr == "max" else z.amin(1)
    return torch.where(mask.any(1), z, torch.zeros((), dtype=m.dtype))


def scaler_table(edge_index, n, scalers, delta, dtype=torch.float64):
    d = torch.zeros(n, dtype=dtype).index_add_(0, edge_index[1], torch.ones(edge_index.shape[1], dtype=dtype)).clamp(min=1)
    col = {"identity": torch.ones_like(d), "amplification": torch.log(d + 1) / delta[1], "attenuation": delta[1] / torch.log(d + 1),
           "linear": d / delta[0], "inverse_linear": delta[0] / d}
    return torch.stack([col[s] for s in scalers], 1)


def pna_forward(x, edge_index, aggregators, scalers, delta, pre, post, lin, form="edge", on_block=None):
    """PNAConv's arithmetic from explicit parameters: ``pre`` / ``post`` lists of (weight, bias) per tower, ``lin`` = (weight,
    bias).  ``on_block(name, block)``: called with every aggregated [N, T, F] block before the scalers (a test registers
    gradient hooks there)."""
    n, F = x.shape
    T = len(pre)
    src, dst = edge_index[0], edge_index[1]
    if form == "edge":
        h = torch.cat([x[dst], x[src]], 1)                                                  # [E, 2F]
        msg = torch.stack([h @ w.t() + b for w, b in pre], 1)                               # [E, T, F]
        blocks = [aggregate_edge_list(msg, edge_index, n, a) for a in aggregators]
    else:
        def msg_of():
            h = torch.cat([x.unsqueeze(1).expand(n, n, F), x.unsqueeze(0).expand(n, n, F)], 2)   # [target, source, 2F]
            return torch.stack([h @ w.t() + b for w, b in pre], 2)                          # [n, n, T, F]
        blocks = [aggregate_dense(msg_of, x.shape, edge_index, n, a) for a in aggregators]
    if on_block is not None:
        for a, b in zip(aggregators, blocks):
            on_block(a, b)
    agg = torch.cat(blocks, -1)                                                             # [N, T, A F]
    sc = scaler_table(edge_index, n, scalers, delta, x.dtype)
    scaled = torch.cat([agg * sc[:, s].view(-1, 1, 1) for s in range(len(scalers))], -1)    # [N, T, S A F]
    full = torch.cat([x.unsqueeze(1).expand(n, T, F), scaled], -1)
    outs = [full[:, t] @ w.t() + b for t, (w, b) in enumerate(post)]
    return torch.cat(outs, 1) @ lin[0].t() + lin[1]


class _Lin(nn.Module):
    def __init__(self, cin, cout, dtype):
        super().__init__()
        a = 1.0 / math.sqrt(cin)
        self.weight = nn.Parameter((torch.rand(cout, cin, dtype=dtype) * 2 - 1) * a)
        self.bias = nn.Parameter((torch.rand(cout, dtype=dtype) * 2 - 1) * a)


class PNAConvRef(nn.Module):
    """Edge-list reference with PyG's parameter names: ``pre_nns.{t}.0.weight`` [F, 2F] / ``.bias``, ``post_nns.{t}.0.weight``
    [F_out, (A S + 1) F] / ``.bias``, ``lin.weight`` [out, out] / ``.bias``."""

    def __init__(self, in_channels, out_channels, aggregators, scalers, deg, towers=1, dtype=torch.float64):
        super().__init__()
        self.aggregators, self.scalers, self.delta, self.on_block, self.form = list(aggregators), list(scalers), deltas(deg), None, "edge"
        F, fo = in_channels, out_channels // towers
        self.pre_nns = nn.ModuleList([nn.Sequential(_Lin(2 * F, F, dtype)) for _ in range(towers)])
        self.post_nns = nn.ModuleList([nn.Sequential(_Lin((len(aggregators) * len(scalers) + 1) * F, fo, dtype)) for _ in range(towers)])
        self.lin = _Lin(out_channels, out_channels, dtype)

    def forward(self, x, edge_index):
        return pna_forward(x, edge_index, self.aggregators, self.scalers, self.delta,
                           [(s[0].weight, s[0].bias) for s in self.pre_nns], [(s[0].weight, s[0].bias) for s in self.post_nns],
                           (self.lin.weight, self.lin.bias), form=self.form, on_block=self.on_block)


def moments64(x, h):
    """float64 two-pass (sum, deg, mean, var) of x[col] over each row of the host graph ``h`` (rows, col, a = multiplicity), from the
    given (float32) inputs; 0 for a row without entries."""
    x = x.double()
    rs = lambda v: torch.zeros((h.n_rows,) + tuple(v.shape[1:]), dtype=torch.float64).index_add_(0, h.row, v)
    deg = rs(h.a)
    s = rs(h.a.view(-1, 1) * x[h.col])
    mean = s / deg.clamp(min=1).view(-1, 1)
    var = rs(h.a.view(-1, 1) * (x[h.col] - mean[h.row]) ** 2) / deg.clamp(min=1).view(-1, 1)
    return s, deg, mean, var

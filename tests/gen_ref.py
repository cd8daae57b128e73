"""TEST INFRASTRUCTURE: float64 restatement of ``torch_geometric.nn.GENConv`` 2.2.0 with ``aggr="softmax"`` (Li et al., DeeperGCN,
2020) and of ``SoftmaxAggregation``, from the published source from memory -- PyG cannot be installed here, so this file is the pin.

    h   = lin_src(x) if in != out else x
    m_j = relu(h_j) + eps
    agg_i[c] = sum_{j -> i} softmax_{j -> i}(t m_j[c]) m_j[c]            (per channel; a duplicate edge counts twice; no edge: 0)
    agg = normalize(agg, p=2, dim=-1) * ||x_i||_2 * msg_norm.scale      (only with msg_norm; the RAW x)
    out = agg + (lin_dst(x) if in != out else x)
    y   = mlp(out)            mlp: Linear(out, out * expansion), norm, ReLU, Dropout(0), ..., Linear(out * expansion, out)

Two independent forms of the aggregation, both differentiable: ``softmax_aggr_edge_list`` (``index_add_`` over the edges, as PyG's
scatter softmax runs) and ``softmax_aggr_dense`` (an [N, N] multiplicity matrix and a masked softmax over its columns).  The tests
hold them to each other in float64 and the kernels to the edge-list form."""
import torch
import torch.nn as nn


def message(h, eps):
    """GENConv's message of a source row; ``eps=None``: the row itself (a plain SoftmaxAggregation)."""
    return h if eps is None else torch.relu(h) + eps


def softmax_aggr_edge_list(m, edge_index, n, t, full=False):
    """agg [n, C] of the node messages ``m`` [n, C] over the edges (row 0: sources, row 1: targets); ``t``: float or [1] tensor.
    ``full``: also lse [n, C] = log sum_{j -> i} exp(t m_j) (0 on a node without edges)."""
    src, dst = edge_index[0], edge_index[1]
    C = m.shape[1]
    z = m[src] * t
    idx = dst.view(-1, 1).expand(-1, C)
    mx = torch.full((n, C), -float("inf"), dtype=m.dtype).scatter_reduce(0, idx, z.detach(), "amax")
    has = torch.zeros(n, dtype=torch.bool).index_fill_(0, dst, True).view(-1, 1)
    mx = torch.where(has, mx, torch.zeros((), dtype=m.dtype))
    ex = torch.exp(z - mx[dst])
    den = torch.zeros((n, C), dtype=m.dtype).index_add_(0, dst, ex)
    num = torch.zeros((n, C), dtype=m.dtype).index_add_(0, dst, ex * m[src])
    one = torch.ones((), dtype=m.dtype)
    agg = torch.where(has, num / torch.where(has, den, one), torch.zeros((), dtype=m.dtype))
    if not full:
        return agg
    return agg, torch.where(has, mx + torch.log(torch.where(has, den, one)), torch.zeros((), dtype=m.dtype))


def softmax_aggr_dense(m, edge_index, n, t):
    """The same through the dense [n, n] multiplicity matrix A[i, j] = number of edges j -> i."""
    A = torch.zeros((n, n), dtype=m.dtype).index_put_((edge_index[1], edge_index[0]), torch.ones((), dtype=m.dtype), accumulate=True)
    z = (m * t).unsqueeze(0).expand(n, -1, -1)                                   # [i, j, c]
    mask = (A > 0).unsqueeze(-1)
    zm = torch.where(mask, z, torch.full((), -float("inf"), dtype=m.dtype))
    mx = zm.detach().amax(1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros((), dtype=m.dtype))
    w = A.unsqueeze(-1) * torch.exp(torch.where(mask, z - mx, torch.zeros((), dtype=m.dtype)))
    den = w.sum(1)
    num = (w * m.unsqueeze(0)).sum(1)
    has = (A.sum(1) > 0).view(-1, 1)
    return torch.where(has, num / torch.where(has, den, torch.ones((), dtype=m.dtype)), torch.zeros((), dtype=m.dtype))


def dt_rows_edge_list(m, edge_index, n, t, agg, lse, dagg):
    """The per-SOURCE-row partials of the temperature's gradient: dt_rows[j] = sum_c m_j[c] sum_{j -> i} p dagg[i, c] (m_j[c] -
    agg[i, c]) with p = exp(t m_j[c] - lse[i, c]); their sum is d/dt of sum(agg * dagg)."""
    src, dst = edge_index[0], edge_index[1]
    p = torch.exp(m[src] * t - lse[dst])
    r = torch.zeros((n, m.shape[1]), dtype=m.dtype).index_add_(0, src, p * dagg[dst] * (m[src] - agg[dst]))
    return (m * r).sum(1)


def kernel_reference(h, root, dout, edge_index, n, t, eps, dtype):
    """Everything the two launches produce, in ``dtype``: y (with the root), lse, dh, dt_rows."""
    h = h.detach().to(dtype).clone().requires_grad_(True)
    tt = torch.tensor([float(t)], dtype=dtype, requires_grad=True)
    m = message(h, eps)
    agg, lse = softmax_aggr_edge_list(m, edge_index, n, tt, full=True)
    y = agg if root is None else agg + root.to(dtype)
    (y * dout.to(dtype)).sum().backward()
    dt = dt_rows_edge_list(m.detach(), edge_index, n, float(t), agg.detach(), lse.detach(), dout.to(dtype))
    return dict(y=y.detach(), lse=lse.detach(), dh=h.grad, dt_rows=dt, dt=tt.grad)


class _T(nn.Module):
    def __init__(self, t, learn):
        super().__init__()
        self.learn = bool(learn)
        self.t = nn.Parameter(torch.full((1,), float(t), dtype=torch.float64)) if learn else float(t)


class _Scale(nn.Module):
    def __init__(self, learn):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(1, dtype=torch.float64), requires_grad=bool(learn))


class GENConvRef(nn.Module):
    """The restatement as a module with PyG's parameter names; ``form``: "edge" or "dense".  ``dtype``: float64 (the reference) or
    float32 (the yardstick of what any float32 evaluation can reach)."""

    def __init__(self, in_channels, out_channels, t=1.0, learn_t=False, msg_norm=False, learn_msg_scale=False, norm="batch",
                 num_layers=2, expansion=2, eps=1e-7, bias=False, dtype=torch.float64):
        super().__init__()
        self.in_channels, self.out_channels, self.eps, self.form = in_channels, out_channels, eps, "edge"
        self.aggr_module = _T(t, learn_t)
        if in_channels != out_channels:
            self.lin_src = nn.Linear(in_channels, out_channels, bias=bias)
            self.lin_dst = nn.Linear(in_channels, out_channels, bias=bias)
        widths = [out_channels] + [out_channels * expansion] * (num_layers - 1) + [out_channels]
        layers = []
        for i in range(1, len(widths)):
            layers.append(nn.Linear(widths[i - 1], widths[i], bias=bias))
            if i < len(widths) - 1:
                if norm == "batch":
                    layers.append(nn.BatchNorm1d(widths[i]))
                elif norm == "layer":
                    layers.append(nn.LayerNorm(widths[i]))
                layers += [nn.ReLU(), nn.Dropout(0.0)]
        self.mlp = nn.Sequential(*layers)
        if msg_norm:
            self.msg_norm = _Scale(learn_msg_scale)
        self.to(dtype)
        self._pre_relu = []
        for mod in self.mlp:
            if isinstance(mod, nn.ReLU):
                mod.register_forward_hook(lambda _m, inp, _out: self._pre_relu.append(inp[0].detach()))

    def relu_margin(self):
        """The smallest |argument| of any ReLU of the last forward (the message's and the MLP's).  The ReLU's gradient is a step: an
        argument that close to 0 may get the other sign in a float32 evaluation, and then ONE element of the gradient differs by its
        whole size -- a test compares gradients only where this margin is clear of float32 rounding."""
        return min(float(v[v != 0].abs().min()) for v in self._pre_relu)     # (an exact 0 comes out of an earlier ReLU: no ambiguity)

    def load_from(self, conv):
        """Take every parameter and buffer (and the unlearnt temperature and eps) of a ``nn_ops.GENConv``."""
        dt = next(self.mlp.parameters()).dtype
        self.load_state_dict({k: v.detach().cpu().to(dt) if v.is_floating_point() else v.detach().cpu() for k, v in conv.state_dict().items()})
        if not self.aggr_module.learn:
            self.aggr_module.t = float(conv.aggr_module.t)
        self.eps = conv.eps
        self.train(conv.training)
        return self

    def aggregate(self, h, edge_index):
        aggr = softmax_aggr_edge_list if self.form == "edge" else softmax_aggr_dense
        m = message(h, self.eps)
        if self.eps is not None:
            self._pre_relu.append(h.detach())
        agg = aggr(m, edge_index, h.shape[0], self.aggr_module.t)
        if agg.requires_grad:
            agg.retain_grad()
        self.last_m, self.last_agg = m, agg                       # (for dt_rows_of_last_backward)
        return agg

    def dt_rows_of_last_backward(self, edge_index):
        """dt_rows of the last forward + backward (``dt_rows_edge_list`` on what ``aggregate`` kept)."""
        m, agg, n = self.last_m.detach(), self.last_agg.detach(), self.last_m.shape[0]
        t = float(torch.as_tensor(self.aggr_module.t).detach())
        _, lse = softmax_aggr_edge_list(m, edge_index, n, t, full=True)
        return dt_rows_edge_list(m, edge_index, n, t, agg, lse, self.last_agg.grad)

    def pre_mlp(self, x, edge_index):
        lin = self.in_channels != self.out_channels
        agg = self.aggregate(self.lin_src(x) if lin else x, edge_index)
        if hasattr(self, "msg_norm"):
            agg = torch.nn.functional.normalize(agg, p=2.0, dim=-1) * x.norm(p=2, dim=-1, keepdim=True) * self.msg_norm.scale
        return agg + (self.lin_dst(x) if lin else x)

    def forward(self, x, edge_index):
        del self._pre_relu[:]
        return self.mlp(self.pre_mlp(x, edge_index))

"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the point-pair entry points of ``dual_dmp_amd.ops`` (``ppf_entries``,
``gather_max_attr``, ``gather_max_attr_bwd``) and of the few other calls ``nn_ops._PPFConvFn`` makes, with the same signatures and
the same tie rule (the smallest source id wins).  Tests inject it with ``monkeypatch.setattr(nn_ops, "ops", ppf_ops_stub)`` to pin
the host side (the ``[Wx | Wp]`` split, the transposed edge block, the ``[ceil(n / 8), 4, C]`` layout of the partials, where the
bias goes) without a GPU; the product never imports it and has no CPU fallback.  The graph is gat_ops_stub's: the HOST structure of
the valued graph.  Arithmetic is float64 internally, float32 at the interfaces.  Every formula is written out per CSR entry as the
kernels compute it -- no autograd."""
import torch

import gat_ops_stub as _g

DdmpError = _g.DdmpError
on_device, Graph, _rowsum = _g.on_device, _g.Graph, _g._rowsum
calls = []                      # names of the entry points reached, in order
want_args = []                  # the want_arg of every gather_max_attr call


def _logged(name, fn):
    def wrapped(*a, **k):
        calls.append(name)
        return fn(*a, **k)
    return wrapped


gemm_nt, gemm_nn, gemm_tn, colsum = (_logged(k, getattr(_g, k)) for k in ("gemm_nt", "gemm_nn", "gemm_tn", "colsum"))


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    calls.append("graph_for")
    assert norm == "gat" and edge_weight is None and not improved and normalize
    return Graph(edge_index, num_nodes, _g._ops.GV_LOOPS if add_self_loops else 0)


def gatv2_datt(part, heads):
    calls.append("gatv2_datt")
    assert part.shape[1] % heads == 0
    return part.double().sum(0).view(heads, -1).float()


def ppf_entries(g, pos, normal):
    calls.append("ppf_entries")
    assert pos.dtype == normal.dtype == torch.float32 and pos.shape == normal.shape == (g.n_rows, 3)
    assert not pos.requires_grad and not normal.requires_grad
    p, nr = pos.double(), normal.double()
    i, j = g.row, g.col
    d = p[j] - p[i]
    ang = lambda a, b: torch.atan2(torch.cross(a, b, dim=1).norm(dim=1), (a * b).sum(1))
    f = torch.stack([d.norm(dim=1), ang(nr[i], d), ang(nr[j], d), ang(nr[i], nr[j])], 1)
    f[i == j] = 0.0                                              # a loop: exactly 0
    return f.float()


def _messages(g, b, f, e):
    assert g.values_key == ("ones",) and f.dtype == e.dtype == torch.float32
    assert f.shape == (g.nnz, 4) and f.is_contiguous() and e.dim() == 2 and e.shape[0] == 4 and e.is_contiguous()
    msg = f.double() @ e.double()
    if b is not None:
        assert b.dtype == torch.float32 and b.shape == (g.n_rows, e.shape[1])
        msg = msg + b.double()[g.col]
    return msg


def gather_max_attr(g, b, f, e, out=None, want_arg=True):
    calls.append("gather_max_attr")
    want_args.append(bool(want_arg))
    n, C = g.n_rows, e.shape[1]
    msg = _messages(g, b, f, e)
    idx = g.row.view(-1, 1).expand(-1, C)
    mx = torch.full((n, C), -float("inf"), dtype=torch.float64).scatter_reduce(0, idx, msg, "amax")
    big = torch.iinfo(torch.int64).max
    cand = torch.where(msg == mx[g.row], g.col.view(-1, 1).expand(-1, C), torch.full((), big, dtype=torch.int64))
    arg = torch.full((n, C), big, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin")
    empty = (g.rowptr[1:] == g.rowptr[:-1]).view(-1, 1)
    y = torch.where(empty, torch.zeros((), dtype=torch.float64), mx).float()
    arg = torch.where(empty, torch.full((), -1, dtype=torch.int64), arg).to(torch.int32)
    return y, (arg if want_arg else None)


def gather_max_attr_bwd(g, dg, arg, f, out=None, want_parts=True):
    calls.append("gather_max_attr_bwd")
    assert arg is not None and arg.dtype == torch.int32 and arg.shape == dg.shape and f.shape == (g.nnz, 4)
    n, C = g.n_rows, dg.shape[1]
    hit = arg.long()[g.col] == g.row.view(-1, 1)                 # node side: entry (j, i) of row j, arg[i, c] == j
    db = _rowsum(g, torch.where(hit, dg.double()[g.col], torch.zeros((), dtype=torch.float64))).float()
    if out is None:
        out = torch.empty((n, C))
    assert out.shape == (n, C)
    out.copy_(db)
    parts = None
    if want_parts:                                               # row side: entry (i, j) of row i, arg[i, c] == j
        won = (arg.long()[g.row] == g.col.view(-1, 1)).double() * dg.double()[g.row]          # [entries, C]
        per_entry = f.double().unsqueeze(-1) * won.unsqueeze(1)                              # [entries, 4, C]
        groups = (n + 7) // 8
        parts = torch.zeros((groups, 4, C), dtype=torch.float64).index_add_(0, g.row // 8, per_entry).reshape(groups, 4 * C).float()
    return out, parts

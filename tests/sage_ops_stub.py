"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the neighbour-statistics entry points of ``dual_dmp_amd.ops``
(``gather_stats``, ``gather_stats_bwd``) and of the few other calls ``nn_ops._SAGEConvFn`` makes, with the same signatures and the
same tie rule (the smallest source id wins).  Tests inject it with ``monkeypatch.setattr(nn_ops, "ops", sage_ops_stub)`` to pin
the host side (the ``[A_1 | ... | A_k | X]`` row buffer and the column-packed weight, the ``[L | R]`` / ``[dL | dR]`` buffers of
the transform-first form, the routing of every gradient block) without a GPU; the product never imports it and has no CPU
fallback.  The graph is gat_ops_stub's: the HOST structure of the valued graph.  Every formula is written out per CSR entry as
the kernels compute it -- no autograd, and no ``index_add_`` outside ``_rowsum``, the stand-in for a kernel's row loop."""
import torch

import gat_ops_stub as _g

DdmpError = _g.DdmpError
on_device, Graph, colsum, _rowsum = _g.on_device, _g.Graph, _g.colsum, _g._rowsum
calls = []                      # names of the entry points reached, in order
want_args = []                  # the want_arg of every gather_stats call
wants = []                      # the want of every gather_stats call


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    calls.append("graph_for")
    return _g.graph_for(edge_index, num_nodes, norm, edge_weight, improved, add_self_loops, normalize)


def gemm_nt(a, w, out=None, bias=None):
    calls.append("gemm_nt")
    assert a.shape[1] % 4 == 0 and a.shape[1] == w.shape[1]
    return _g.gemm_nt(a, w, out, bias)


def gemm_nn(a, w, out=None):
    calls.append("gemm_nn")
    assert a.shape[1] == w.shape[0]
    return _g.gemm_nn(a, w, out)


def gemm_tn(g, z, out=None):
    calls.append("gemm_tn")
    assert g.shape[0] == z.shape[0]
    return _g.gemm_tn(g, z, out)


def _extremum(g, x, sign):
    """(value, arg) of max (sign = 1) or min (sign = -1) of x[col e] over each row's entries; 0 / -1 for a row without entries."""
    n, C = g.n_rows, x.shape[1]
    idx = g.row.view(-1, 1).expand(-1, C)
    vals = sign * x[g.col]
    mx = torch.full((n, C), -float("inf")).scatter_reduce(0, idx, vals, "amax")
    big = torch.iinfo(torch.int64).max
    cand = torch.where(vals == mx[g.row], g.col.view(-1, 1).expand(-1, C), torch.full((), big, dtype=torch.int64))
    arg = torch.full((n, C), big, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin")
    empty = (g.rowptr[1:] == g.rowptr[:-1]).view(-1, 1)
    return torch.where(empty, torch.zeros(()), sign * mx), torch.where(empty, torch.full((), -1, dtype=torch.int64), arg).to(torch.int32)


def gather_stats(g, x, want=("mean",), root=None, bias=None, copy_x=False, want_arg=True, out=None):
    calls.append("gather_stats")
    want = (want,) if isinstance(want, str) else tuple(want)
    want_args.append(bool(want_arg))
    wants.append(want)
    assert g.values_key == ("ones",) and g.valued == _g._ops.GV_VALUED and x.dtype == torch.float32
    assert len(set(want)) == len(want) and set(want) <= {"mean", "add", "max", "min"} and not {"mean", "add"} <= set(want)
    assert (root is None and bias is None) or "mean" in want or "add" in want
    n, C = g.n_rows, x.shape[1]
    nb = len(want) + bool(copy_x)
    if out is None:
        out = torch.empty((n, nb * C))
    assert out.shape[0] == n and out.shape[1] >= nb * C
    deg = _rowsum(g, g.a)
    invdeg = torch.where(deg > 0, 1.0 / deg, torch.zeros((), dtype=torch.float64)).float()
    args = []
    for k, w in enumerate(want):
        blk = out[:, k * C:(k + 1) * C]
        if w in ("mean", "add"):
            s = _rowsum(g, g.a.view(-1, 1) * x.double()[g.col])
            if w == "mean":
                s = s * invdeg.double().view(-1, 1)
            if root is not None:
                s = s + root.double()[:n]
            if bias is not None:
                s = s + bias.double()
            blk.copy_(s.float())
            args.append(None)
        else:
            v, arg = _extremum(g, x, 1.0 if w == "max" else -1.0)
            blk.copy_(v)
            args.append(arg if want_arg else None)
    if copy_x:
        out[:, (nb - 1) * C:nb * C] = x[:n]
    return tuple(out[:, k * C:(k + 1) * C] for k in range(nb)), tuple(args), (invdeg if "mean" in want else None)


def gather_stats_bwd(g, ds=None, invdeg=None, dmx=None, argmx=None, dmn=None, argmn=None, dx0=None, root=False, out=None):
    calls.append("gather_stats_bwd")
    first = next(t for t in (ds, dmx, dmn) if t is not None)
    assert (dmx is None) == (argmx is None) and (dmn is None) == (argmn is None) and (ds is not None or (not root and invdeg is None))
    n, C = g.n_rows, first.shape[1]
    acc = torch.zeros((n, C), dtype=torch.float64)
    if ds is not None:
        f = g.a[g.mirror]
        if invdeg is not None:
            f = f * invdeg.double()[g.col]
        acc = acc + _rowsum(g, f.view(-1, 1) * ds.double()[g.col])
    for dm, arg in ((dmx, argmx), (dmn, argmn)):
        if dm is not None:
            assert arg.dtype == torch.int32 and arg.shape == dm.shape
            hit = arg.long()[g.col] == g.row.view(-1, 1)
            acc = acc + _rowsum(g, torch.where(hit, dm.double()[g.col], torch.zeros((), dtype=torch.float64)))
    if dx0 is not None:
        acc = acc + dx0.double()
    wt = C + (C if root else 0)
    if out is None:
        out = torch.empty((n, wt))
    assert out.shape[0] == n and out.shape[1] >= wt
    out[:, :C] = acc.float()
    if root:
        out[:, C:wt] = ds[:n]
    return out[:, :C], (out[:, C:wt] if root else None)

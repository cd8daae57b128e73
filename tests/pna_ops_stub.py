"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the neighbour-moments entry points of ``dual_dmp_amd.ops``
(``gather_moments``, ``gather_moments_bwd``) and of the few other calls ``nn_ops._PNAConvFn`` makes, with the same signatures, the
same tie rule (the smallest source id wins) and the same tower-major layout.  Tests inject it with
``monkeypatch.setattr(nn_ops, "ops", pna_ops_stub)`` to pin the host side (the ``[A | B]`` buffer, the tower-major aggregate buffer
and the scaler-packed post weights, the chain rule of std / var folded into the streams dS / dQ, the routing of every gradient
block) without a GPU; the product never imports it and has no CPU fallback.  The graph is gat_ops_stub's: the HOST structure of the
valued graph.  Arithmetic is float64 internally (the variance in two passes); the interfaces keep the operands' dtype (float32 as
the product runs, float64 where a test pins the host side's algebra).  Every formula is written
out per CSR entry -- no autograd, and no ``index_add_`` outside ``_rowsum``, the stand-in for a kernel's row loop."""
import torch

import gat_ops_stub as _g

DdmpError = _g.DdmpError
on_device, Graph, colsum, _rowsum = _g.on_device, _g.Graph, _g.colsum, _g._rowsum
calls = []                      # names of the entry points reached, in order
want_args = []                  # the want_arg of every gather_moments call
wants = []                      # the want of every gather_moments call
MOMENTS = ("mean", "sum", "max", "min", "std", "var")


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    calls.append("graph_for")
    return _g.graph_for(edge_index, num_nodes, norm, edge_weight, improved, add_self_loops, normalize)


def gemm_nt(a, w, out=None, bias=None):
    calls.append("gemm_nt")
    assert a.shape[1] % 4 == 0 and a.shape[1] == w.shape[1] and w.shape[0] % 4 == 0 and a.stride(1) == 1 and a.stride(0) % 4 == 0
    y = a.double() @ w.double().t()
    return (y if bias is None else y + bias.double()).to(a.dtype)


def gemm_nn(a, w, out=None):
    calls.append("gemm_nn")
    assert a.shape[1] == w.shape[0] and a.shape[1] % 4 == 0 and w.shape[1] % 4 == 0
    return (a.double() @ w.double()).to(a.dtype)


def gemm_tn(g, z, out=None):
    calls.append("gemm_tn")
    assert g.shape[0] == z.shape[0] and g.shape[1] % 4 == 0 and z.shape[1] % 4 == 0
    return (g.double().t() @ z.double()).to(g.dtype)


def _extremum(g, x, sign):
    """sage_ops_stub's, in x's dtype: (value, arg) of max (sign = 1) or min (sign = -1) of x[col e] over each row's entries; 0 / -1
    for a row without entries; the smallest source id wins a tie."""
    n, C = g.n_rows, x.shape[1]
    idx = g.row.view(-1, 1).expand(-1, C)
    vals = sign * x[g.col]
    mx = torch.full((n, C), -float("inf"), dtype=x.dtype).scatter_reduce(0, idx, vals, "amax")
    big = torch.iinfo(torch.int64).max
    cand = torch.where(vals == mx[g.row], g.col.view(-1, 1).expand(-1, C), torch.full((), big, dtype=torch.int64))
    arg = torch.full((n, C), big, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin")
    empty = (g.rowptr[1:] == g.rowptr[:-1]).view(-1, 1)
    return (torch.where(empty, torch.zeros((), dtype=x.dtype), sign * mx),
            torch.where(empty, torch.full((), -1, dtype=torch.int64), arg).to(torch.int32))


def gather_moments(g, b, want=("mean",), root=None, tower_width=None, want_arg=True, out=None):
    calls.append("gather_moments")
    want = (want,) if isinstance(want, str) else tuple(want)
    want_args.append(bool(want_arg))
    wants.append(want)
    assert g.values_key == ("ones",) and g.valued == _g._ops.GV_VALUED and b.dtype in (torch.float32, torch.float64)
    assert want and len(set(want)) == len(want) and set(want) <= set(MOMENTS)
    assert not {"mean", "sum"} <= set(want) and not {"std", "var"} <= set(want)
    n, C = g.n_rows, b.shape[1]
    tw = C if tower_width is None else tower_width
    assert C % tw == 0
    nb, T = len(want), C // tw
    if out is None:
        out = torch.empty((n, nb * C), dtype=b.dtype)
    assert out.shape[0] == n and out.shape[1] >= nb * C
    towers = out[:, :nb * C].unflatten(1, (T, nb, tw))
    deg = _rowsum(g, g.a)
    has = (deg > 0).view(-1, 1)
    invdeg = torch.where(deg > 0, 1.0 / deg, torch.zeros((), dtype=torch.float64)).to(b.dtype)
    b64 = b.double()[:n]
    r64 = torch.zeros((n, C), dtype=torch.float64) if root is None else root.double()[:n]
    zero = torch.zeros((), dtype=torch.float64)
    s = _rowsum(g, g.a.view(-1, 1) * b64[g.col])
    mean = s / deg.clamp(min=1).view(-1, 1)
    args, mu = [], None
    for k, w in enumerate(want):
        arg = None
        if w == "sum":
            v = torch.where(has, s + deg.view(-1, 1) * r64, zero)
        elif w == "mean":
            v = torch.where(has, mean + r64, zero)
        elif w in ("max", "min"):
            v, arg = _extremum(g, b[:n], 1.0 if w == "max" else -1.0)
            v = torch.where(has, v.double() + r64, zero)
            arg = arg if want_arg else None
        else:
            var = _rowsum(g, g.a.view(-1, 1) * (b64[g.col] - mean[g.row]) ** 2) / deg.clamp(min=1).view(-1, 1)
            v = var if w == "var" else torch.where(var > 1e-5, var.sqrt(), zero)
            mu = mean.to(b.dtype)
        towers[:, :, k] = v.to(b.dtype).view(n, T, tw)
        args.append(arg)
    blocks = [out[:, k * C:(k + 1) * C] for k in range(nb)] if T == 1 else [towers[:, :, k] for k in range(nb)]
    return tuple(blocks), tuple(args), invdeg, mu


def gather_moments_bwd(g, ds=None, dq=None, b=None, invdeg=None, dmx=None, argmx=None, dmn=None, argmn=None, out=None):
    calls.append("gather_moments_bwd")
    first = next(t for t in (ds, dmx, dmn) if t is not None)
    assert (dmx is None) == (argmx is None) and (dmn is None) == (argmn is None) and (dq is None) == (b is None)
    assert ds is not None or (dq is None and invdeg is None)
    n, C = g.n_rows, first.shape[1]
    f = g.a[g.mirror]
    if invdeg is not None:
        f = f * invdeg.double()[g.col]
    acc = torch.zeros((n, C), dtype=torch.float64)
    if ds is not None:
        acc = acc + _rowsum(g, f.view(-1, 1) * ds.double()[g.col])
    if dq is not None:
        acc = acc + b.double()[:n] * _rowsum(g, f.view(-1, 1) * dq.double()[g.col])
    for dm, arg in ((dmx, argmx), (dmn, argmn)):
        if dm is not None:
            assert arg.dtype == torch.int32 and arg.shape == dm.shape
            hit = arg.long()[g.col] == g.row.view(-1, 1)
            acc = acc + _rowsum(g, torch.where(hit, dm.double()[g.col], torch.zeros((), dtype=torch.float64)))
    if out is None:
        out = torch.empty((n, C), dtype=first.dtype)
    assert tuple(out.shape) == (n, C)
    out.copy_(acc.to(out.dtype))
    return out

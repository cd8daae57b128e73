"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the softmax-aggregation entry points of ``dual_dmp_amd.ops``
(``gather_softmax``, ``gather_softmax_bwd``) and of the few other calls ``nn_ops._GENConvFn`` / ``_LinearFn`` make, with the same
signatures and the same row-buffer conventions.  Tests inject it with ``monkeypatch.setattr(nn_ops, "ops", gen_ops_stub)`` to pin the
host side (the ``[H | D]`` buffer, the fused root, ``Y' = y - root``, the ``[dH | dD]`` gradient buffer, the temperature's gradient,
the routing of every gradient block) without a GPU; the product never imports it and has no CPU fallback.  The graph is
gat_ops_stub's: the HOST structure of the valued graph.  Arithmetic is float64 internally; the interfaces keep the operands' dtype.
Every formula is written out per CSR entry as the kernels compute it -- the backward recomputes the weights from lse, no autograd --
and ``index_add_`` appears only in ``_rowsum``, the stand-in for a kernel's row loop."""
import contextlib

import torch

import gat_ops_stub as _g

DdmpError = _g.DdmpError
on_device, Graph, colsum, _rowsum = _g.on_device, _g.Graph, _g.colsum, _g._rowsum
calls = []                      # names of the entry points reached, in order
want_lses = []                  # the want_lse of every gather_softmax call
roots = []                      # what every gather_softmax / gather_softmax_bwd call got as root (True / False / "add")


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    calls.append("graph_for")
    return _g.graph_for(edge_index, num_nodes, norm, edge_weight, improved, add_self_loops, normalize)


gemm_modes = []                 # the mode of every gemm_mode block entered


@contextlib.contextmanager
def gemm_mode(mode):
    gemm_modes.append(mode)
    yield


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


def _msg(h, eps):
    return h.double() if eps is None else torch.relu(h.double()) + eps


def gather_softmax(g, h, t, msg_eps=None, root=None, out=None, want_lse=True):
    calls.append("gather_softmax")
    want_lses.append(bool(want_lse))
    roots.append(root is not None)
    assert g.values_key == ("ones",) and g.valued == _g._ops.GV_VALUED and isinstance(t, float)
    n, C = g.n_rows, h.shape[1]
    m = _msg(h[:n], msg_eps)
    z = t * m[g.col]
    idx = g.row.view(-1, 1).expand(-1, C)
    mx = torch.full((n, C), -float("inf"), dtype=torch.float64).scatter_reduce(0, idx, z, "amax")
    has = (g.rowptr[1:] > g.rowptr[:-1]).view(-1, 1)
    mx = torch.where(has, mx, torch.zeros((), dtype=torch.float64))
    ex = g.a.view(-1, 1) * torch.exp(z - mx[g.row])
    den = _rowsum(g, ex)
    one, zero = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    y = torch.where(has, _rowsum(g, ex * m[g.col]) / torch.where(has, den, one), zero)
    lse = torch.where(has, mx + torch.log(torch.where(has, den, one)), zero)
    if root is not None:
        y = y + root.double()[:n]
    if out is None:
        out = torch.empty((n, C), dtype=h.dtype)
    assert tuple(out.shape) == (n, C)
    out.copy_(y.to(h.dtype))
    return out, (lse.to(h.dtype) if want_lse else None)


def gather_softmax_bwd(g, dout, h, y, lse, t, msg_eps=None, root=False, want_dt=False, out=None):
    calls.append("gather_softmax_bwd")
    roots.append(root)
    assert root in (False, True, "add") and isinstance(t, float)
    n, C = g.n_rows, dout.shape[1]
    m = _msg(h[:n], msg_eps)
    w = g.a[g.mirror].view(-1, 1)
    p = torch.exp(t * m[g.row] - lse.double()[g.col])
    gd = w * p * dout.double()[g.col]
    s = _rowsum(g, gd)
    r = _rowsum(g, gd * (m[g.row] - y.double()[g.col]))
    dh = s + t * r
    if msg_eps is not None:
        dh = torch.where(h.double()[:n] > 0, dh, torch.zeros((), dtype=torch.float64))
    if root == "add":
        dh = dh + dout.double()[:n]
    wt = C * (2 if root is True else 1)
    if out is None:
        out = torch.empty((n, wt), dtype=dout.dtype)
    assert out.shape[0] == n and out.shape[1] >= wt
    out[:, :C] = dh.to(dout.dtype)
    dr = None
    if root is True:
        out[:, C:2 * C] = dout[:n]
        dr = out[:, C:2 * C]
    return out[:, :C], dr, ((m * r).sum(1).to(dout.dtype) if want_dt else None)

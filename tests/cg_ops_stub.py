"""TEST INFRASTRUCTURE: PyTorch-CPU restatements of the crystal-gate entry points of ``dual_dmp_amd.ops`` (``cgate_fwd``,
``cgate_bwd_row``, ``cgate_bwd_node``) and of the few other calls ``nn_ops._CGConvFn`` makes, with the same signatures.  Tests
inject it with ``monkeypatch.setattr(nn_ops, "ops", cg_ops_stub)`` to pin the host side (the packed ``[Wf_i ; Ws_i ; Wf_j ; Ws_j]``
GEMM, the ``[Af | As | Bf | Bs]`` / ``[dAf | dAs | dBf | dBs]`` row buffers, the transposed edge blocks, the ``[n, 2, dim, C]``
layout of the partials, the ``mirror`` use, where the residual and its gradient go) without a GPU; the product never imports it and
has no CPU fallback.  The graph is gmm_ops_stub's -- the HOST structure of the valued graph plus ``eid``, the entry of every input
edge.  Arithmetic is float64 internally, float32 at the interfaces.  Every formula is written out per CSR entry (dim == 0: an entry
counts with its multiplicity) or per input edge of an entry's span (dim > 0) as the kernels compute it -- no autograd."""
import torch

import gmm_ops_stub as _m

DdmpError = _m.DdmpError
CG_MAX_DIM = 8
Graph = _m.Graph
on_device, gemm_nt, gemm_nn, gemm_tn, colsum, _rowsum = _m.on_device, _m.gemm_nt, _m.gemm_nn, _m.gemm_tn, _m.colsum, _m._rowsum
calls = []                      # names of the entry points reached, in order


def graph_for(edge_index, num_nodes, norm="gcn", edge_weight=None, improved=False, add_self_loops=True, normalize=True):
    assert norm == "gat" and edge_weight is None and not improved and normalize and not add_self_loops
    calls.append("graph_for")
    return Graph(edge_index, num_nodes, 0)


def gatv2_datt(part, heads):
    calls.append("gatv2_datt")
    assert part.shape[1] % heads == 0
    return part.double().sum(0).view(heads, -1).float()


def _put(out, v):
    if out is None:
        return v.float()
    out.copy_(v)
    return out


def _softplus(s):
    return s.clamp(min=0.0) + torch.log1p(torch.exp(-s.abs()))


def _check(g, attr, ef, es, C):
    assert g.values_key == ("ones",) and (attr is None) == (ef is None) == (es is None)
    if attr is not None:
        assert attr.dtype == torch.float32 and attr.shape[0] == g.nnz_in and attr.is_contiguous()
        dim = attr.shape[1]
        assert 1 <= dim <= CG_MAX_DIM and ef.shape == es.shape == (dim, C) and ef.is_contiguous() and es.is_contiguous()


def _terms(g, af, as_, bf, bs, attr, ef, es, mean, node):
    """One term per entry (dim == 0) or per input edge (dim > 0) -> (own, tgt, src, m, F, S, a): the row whose sum the term
    enters -- the target's row e, or (``node``) the source's own entry mirror e --, the target i and the source j, the factor m =
    w_i (x the multiplicity of e when dim == 0) and the gate arguments, all float64."""
    af, as_, bf, bs = (t.double() for t in (af, as_, bf, bs))
    if attr is None:
        e = g.mirror if node else torch.arange(g.nnz)             # (node: own entry e' = 0 .. nnz - 1 reads the entry mirror e')
        own = g.row                                               # the row of the own entry e'
        tgt, src = g.row[e], g.col[e]
        cnt = _rowsum(g, g.a)                                     # the sum of a row's multiplicities
        m, a, F, S = g.a[e], None, af[tgt] + bf[src], as_[tgt] + bs[src]
    else:
        e = g.eid                                                 # the entry of every input edge, in input order
        tgt, src = g.row[e], g.col[e]
        own = g.row[g.mirror[e]] if node else tgt
        cnt = torch.zeros(g.n_rows, dtype=torch.float64).index_add_(0, tgt, torch.ones(g.nnz_in, dtype=torch.float64))
        a = attr.double()
        m, F, S = torch.ones(g.nnz_in, dtype=torch.float64), af[tgt] + bf[src] + a @ ef.double(), as_[tgt] + bs[src] + a @ es.double()
    if node:
        assert torch.equal(own, src)
    if mean:
        m = m / cnt.clamp(min=1.0)[tgt]
    return own, tgt, src, m.unsqueeze(1), F, S, a


def _sum(g, own, v):
    return torch.zeros((g.n_rows,) + tuple(v.shape[1:]), dtype=torch.float64).index_add_(0, own, v)


def cgate_fwd(g, af, as_, bf, bs, attr=None, ef=None, es=None, root=None, mean=False, out=None):
    calls.append("cgate_fwd" + ("+root" if root is not None else ""))
    _check(g, attr, ef, es, af.shape[1])
    own, _, _, m, F, S, _ = _terms(g, af, as_, bf, bs, attr, ef, es, mean, False)
    y = _sum(g, own, m * torch.sigmoid(F) * _softplus(S))
    if root is not None:
        assert root.shape == af.shape
        y = y + root.double()
    return _put(out, y)


def _grad_terms(g, dout, af, as_, bf, bs, attr, ef, es, mean, node):
    own, tgt, _, m, F, S, a = _terms(g, af, as_, bf, bs, attr, ef, es, mean, node)
    f, gd = torch.sigmoid(F), m * dout.double()[tgt]
    return own, gd * _softplus(S) * f * (1 - f), gd * f * torch.sigmoid(S), a


def cgate_bwd_row(g, dout, af, as_, bf, bs, attr=None, ef=None, es=None, mean=False, out_f=None, out_s=None, want_parts=True):
    calls.append("cgate_bwd_row" + ("+parts" if attr is not None and want_parts else ""))
    _check(g, attr, ef, es, af.shape[1])
    own, dF, dS, a = _grad_terms(g, dout, af, as_, bf, bs, attr, ef, es, mean, False)
    parts = None
    if attr is not None and want_parts:                            # [n, 2, dim, C]: [sum dF (x) a | sum dS (x) a]
        both = torch.stack([a.unsqueeze(-1) * dF.unsqueeze(1), a.unsqueeze(-1) * dS.unsqueeze(1)], 1)
        parts = _sum(g, own, both).reshape(g.n_rows, -1).float()
    return _put(out_f, _sum(g, own, dF)), _put(out_s, _sum(g, own, dS)), parts


def cgate_bwd_node(g, dout, af, as_, bf, bs, attr=None, ef=None, es=None, mean=False, out_f=None, out_s=None, out_r=None):
    calls.append("cgate_bwd_node" + ("+root" if out_r is not None else ""))
    _check(g, attr, ef, es, af.shape[1])
    own, dF, dS, _ = _grad_terms(g, dout, af, as_, bf, bs, attr, ef, es, mean, True)
    if out_r is not None:
        out_r.copy_(dout)
    return _put(out_f, _sum(g, own, dF)), _put(out_s, _sum(g, own, dS))

"""Drop-ins for fifteen ``torch_geometric.nn`` 2.2.0 operators on the HIP kernels: same constructor / call signature, parameter names
and initialisation; the dense part goes through the GEMMs, the graph part through one fused gather launch per direction, and no
per-edge feature tensor exists at any point.  Each operator is documented once, at its class: ``GCNConv``, ``ChebConv``,
``GATConv``, ``GATv2Conv``, ``TransformerConv``, ``ResGatedGraphConv``, ``FeaStConv``, ``GMMConv`` (with ``cartesian_pseudo``),
``SplineConv``, ``EdgeConv``, ``PPFConv`` (with ``point_pair_features``), ``SAGEConv``, ``PNAConv`` (with ``degree_histogram``),
``GENConv``, ``CGConv``.

``edge_weight`` (``GCNConv`` and ``ChebConv``; restated from the published PyG 2.2.0 source from memory -- PyG cannot be installed
here, so this could not be checked against it; the pin is the dense float64 restatement ``tests/gcnw_ref.py``):

* ``GCNConv(in, out, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True)``,
  ``forward(x, edge_index, edge_weight=None)``.  ``gcn_norm``: ``fill = 2 if improved else 1``; with ``add_self_loops`` explicit
  self loops leave the edge list and every node gets one loop of weight ``fill`` -- except that a node with explicit loops keeps
  the weight of its LAST explicit loop in input order (``add_remaining_self_loops``); ``deg_i`` = sum of ``w_e`` over the entries
  with target i (loop included), ``s_i = deg_i^-1/2`` (inf -> 0), entry value ``s_i w_e s_j``; duplicate edges each contribute.
  ``normalize=False``: no loops are added and the entry value is ``w_e`` (1 without ``edge_weight``), whatever
  ``add_self_loops`` says.  ``cached`` is accepted and has no effect: the graph is always cached by tensor identity.
  Differentiable w.r.t. ``edge_weight`` (an SDDMM over the CSR + the normalisation's chain rule, ``ops.sddmm`` /
  ``ops.graph_weight_grad``).  The edge STRUCTURE must be symmetric; the weights need not be.
* ``ChebConv.forward(..., edge_weight=w)``: self loops removed, ``S = D^-1/2 A_w D^-1/2``, ChebConv's recurrence on the valued S.
  SYMMETRIC weights only (after coalescing ``w_ij == w_ji`` bit for bit, else ``ValueError``: PyG takes the degree over sources
  here and over targets in ``gcn_norm``; the two agree only for symmetric weights).  No gradient w.r.t. ``edge_weight``.
* Refused with ``ValueError`` before any gather: non-finite weights, a negative weighted degree, a length other than
  ``edge_index.shape[1]``, a dtype other than float32 / float64 (float64 is rounded to float32 once), a weight tensor that is not
  on the GPU, bf16 features.  ``edge_weight=None`` with default options is the unvalued graph and code path, bit for bit.
"""
from __future__ import annotations

import contextlib
import math

import torch
import torch.nn as nn

from . import ops


def _pad_cols(t: torch.Tensor, mult: int = 4) -> torch.Tensor:
    c = t.shape[1]
    if c % mult == 0 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0:
        return t
    cp = (c + mult - 1) // mult * mult
    out = torch.zeros((t.shape[0], cp), dtype=t.dtype, device=t.device)
    out[:, :c] = t
    return out


def _pad_rows_like(wp, dyp, cout):
    """``wp`` ([cout, .]) with zero rows appended to match a ragged output width that ``_pad_cols`` padded (``dyp``)."""
    if dyp.shape[1] == cout:
        return wp
    wrow = torch.zeros((dyp.shape[1], wp.shape[1]), dtype=wp.dtype, device=wp.device)
    wrow[:cout] = wp
    return wrow


def _bias_grad(dy):
    """Column sum of ``dy``: ``ops.colsum`` at the power-of-two widths it takes, torch otherwise."""
    cout = dy.shape[1]
    pow2 = 8 <= cout <= 1024 and (cout & (cout - 1)) == 0
    return ops.colsum(dy).to(dy.dtype) if pow2 else dy.sum(0)


def _pack(blocks, width, device, pad_each=False, dtype=torch.float32):
    """The blocks ([rows_k, <= width] each, ``None`` skipped) stacked into ONE zero-padded matrix (float32 unless ``dtype``) for a single GEMM: end to
    end with the total rounded up to a multiple of 4, or (``pad_each``) every block rounded up on its own.  -> (the matrix, the
    (start, stop) rows of every block in it, ``None`` for a ``None`` block)."""
    spans, rows = [], 0
    for b in blocks:
        if b is None:
            spans.append(None)
            continue
        spans.append((rows, rows + b.shape[0]))
        rows = (rows + b.shape[0] + 3) // 4 * 4 if pad_each else rows + b.shape[0]
    wp = torch.zeros(((rows + 3) // 4 * 4, width), dtype=dtype, device=device)
    for s, b in zip(spans, blocks):
        if s is not None:
            wp[s[0]:s[1], :b.shape[1]] = b
    return wp, spans


def _packed_rows(blocks, width, device, pad_each=False, dtype=torch.float32):
    """``_pack``'s matrix alone."""
    return _pack(blocks, width, device, pad_each, dtype)[0]


def _cols(m, span):
    """The column block ``span`` of a row buffer as a view; ``None`` for an absent block."""
    return None if span is None else m[:, span[0]:span[1]]


def _grad_rows(n, used, padded, device, dtype=torch.float32):
    """An uninitialised [n, padded] gradient row buffer (float32 unless ``dtype``) with the columns outside the ``used`` (start, stop) spans (``None``
    entries skipped) -- the padding the kernels never write -- zeroed."""
    g = torch.empty((n, padded), dtype=dtype, device=device)
    end = 0
    for a, b in [s for s in used if s is not None] + [(padded, padded)]:
        if a > end:
            g[:, end:a] = 0
        end = b
    return g


def _packed_gemm(x, weights, biases=None, pad_each=False, dtype=torch.float32):
    """The packed linear map every drop-in below starts with: ONE ``ops.gemm_nt`` of the padded x (float32 unless ``dtype``) against the weight blocks
    ([rows_k, cin] each; a ``None`` entry is an absent block) stacked by ``_pack``.  ``biases`` is parallel to ``weights``:
    all ``None`` (or no ``biases``) -- the GEMM gets no bias; otherwise they are packed like the weights, with a zero block where a
    present weight has none.  -> (xp, wp, buf, spans): the padded x, the packed weight, the row buffer ``xp @ wp^T + bias`` and
    the column span of every block in ``buf`` -- and in the gradient buffer ``_grad_rows(n, spans, wp.shape[0], device)`` that
    ``_packed_grads`` takes -- ``None`` for an absent block (``_cols(buf, spans[k])`` is block k)."""
    xp = _pad_cols(x.detach().to(dtype))
    wp, spans = _pack([None if w is None else w.detach() for w in weights], xp.shape[1], x.device, pad_each, dtype)
    lb = None
    for s, b in zip(spans, biases or ()):
        if s is not None and b is not None:
            if lb is None:
                lb = torch.zeros(wp.shape[0], dtype=dtype, device=x.device)
            lb[s[0]:s[1]] = b.detach()
    return xp, wp, ops.gemm_nt(xp, wp, bias=lb), spans


def _packed_grads(g, xp, wp, spans, cin, need_w, need_b, need_x):
    """Backward of ``_packed_gemm`` from the gradient row buffer ``g``.  ``need_w`` / ``need_b`` are parallel to ``spans``
    (``need_b=None``: no bias gradient).  -> (dx, [dW_k], [db_k]): the column sums of the blocks whose bias wants a gradient, ONE
    ``ops.gemm_tn`` (only when some block's weight wants a gradient; then every present block gets its ``[rows_k, cin]`` slice)
    and ONE ``ops.gemm_nn`` (``need_x``).  ``None`` where a block is absent or nothing was asked."""
    n = len(spans)
    dw, db, want_w = [None] * n, [None] * n, False
    for k, s in enumerate(spans):
        if s is not None:
            want_w = want_w or bool(need_w[k])
            if need_b is not None and need_b[k]:
                db[k] = _bias_grad(g[:, s[0]:s[1]])
    if want_w:
        dwp = ops.gemm_tn(g, xp)
        dw = [None if s is None else dwp[s[0]:s[1], :cin] for s in spans]
    dx = ops.gemm_nn(g, wp)[:, :cin] if need_x else None
    return dx, dw, db


def _heads_mean(y, heads, add=None):
    """``concat=False``: the mean of y [N, heads * C] over the heads -> [N, C], then ``+ add`` (the bias or the skip) if given."""
    y = y.view(-1, heads, y.shape[1] // heads).mean(1)
    return y if add is None else y + add


def _heads_mean_bwd(dy, heads):
    """Backward of ``_heads_mean``: dy [N, C] / heads, broadcast to every head -> [N, heads * C]."""
    C = dy.shape[1]
    return (dy / heads).unsqueeze(1).expand(-1, heads, C).reshape(-1, heads * C)


class _Fn(torch.autograd.Function):
    """Base of the autograd functions below: ``backward`` enters the gradient's device and runs the subclass's ``_backward``."""

    @classmethod
    def backward(cls, ctx, *dy):
        with ops.on_device(dy[0]):
            return cls._backward(ctx, *dy)


def _bias_param(module, bias, n, init=torch.zeros):
    """``module.bias``: a parameter [n] made by ``init``, or registered as None."""
    if bias:
        module.bias = nn.Parameter(init(n))
    else:
        module.register_parameter("bias", None)


def _glorot_(t):
    """PyG's 'glorot' in place: uniform(+-sqrt(6 / (fan of the last two dims)))."""
    a = math.sqrt(6.0 / (t.shape[-2] + t.shape[-1]))
    return t.uniform_(-a, a)


def _reset_linear(lin):
    """PyG ``Linear``'s default in place: uniform(+-1/sqrt(in)) on the weight and on the bias, where there is one."""
    a = 1.0 / math.sqrt(lin.weight.shape[1])
    lin.weight.uniform_(-a, a)
    if getattr(lin, "bias", None) is not None:
        lin.bias.uniform_(-a, a)


# The refusals.  The operators differ in a few exception types and wordings (a parameter each); tests and users read the texts.

def _no_tuple_channels(name, in_channels):
    if isinstance(in_channels, (tuple, list)):
        raise ValueError("%s: tuple in_channels (bipartite graphs) are not implemented on the HIP path" % name)


def _no_tuple_x(name, x):
    if isinstance(x, (tuple, list)):
        raise ValueError("%s: a tuple x (bipartite graphs) is not implemented on the HIP path" % name)


def _int_ge1(name, what, v, bool_ok=False):
    """``v`` (``heads``, ``K``, ``dim`` ...) must be an int >= 1; ``bool_ok``: GATConv and ChebConv let a bool through."""
    if not isinstance(v, int) or (isinstance(v, bool) and not bool_ok) or v < 1:
        raise ValueError("%s: %s must be an integer >= 1, got %r" % (name, what, v))


def _not_implemented(name, **args):
    """``ValueError`` for the first of the PyG arguments ``args``, in the order given, that is not None."""
    for arg, v in args.items():
        if v is not None:
            what = "edge_dim (edge features)" if arg == "edge_dim" else arg
            raise ValueError("%s: %s is not implemented on the HIP path" % (name, what))


def _no_attention_dropout(name, module):
    if module.dropout != 0.0 and module.training:
        raise ValueError("%s: attention dropout in training mode is not implemented on the HIP path (dropout=%g)" % (name, module.dropout))


def _check_aggr(name, aggr, allowed, kwargs, resgated=False):
    """``aggr`` must be one of ``allowed``, and nothing may be left in the constructor's ``kwargs``.  ``resgated``:
    ResGatedGraphConv's own wording, and a ``ValueError`` for stray arguments where the others raise ``TypeError``."""
    if aggr not in allowed:
        if resgated:
            raise ValueError("%s: aggr must be %r on the HIP path, got %r" % (name, allowed[0], aggr))
        which = " and ".join("aggr=%r" % a for a in allowed) + (" is" if len(allowed) == 1 else " are")
        raise ValueError("%s: only %s implemented on the HIP path, got %r" % (name, which, aggr))
    if kwargs and resgated:
        raise ValueError("%s: unsupported arguments %s" % (name, sorted(kwargs)))
    if kwargs:
        raise TypeError("%s: unexpected keyword arguments %s" % (name, sorted(kwargs)))


def _check_x(name, x, in_channels, bf16=True):
    """The refusals every operator shares for its features: bf16 (``bf16=False``: the operator has its own rule), then the shape."""
    if bf16 and x.dtype == torch.bfloat16:
        raise ValueError("%s: bf16 features are not supported on the HIP path" % name)
    if x.dim() != 2 or x.shape[1] != in_channels:
        raise ValueError("%s: expected x of shape [N, %d]" % (name, in_channels))


def _need_entries(name, edge_index, loops=False):
    """A graph without a single entry -- an empty ``edge_index`` where the operator adds no self loops (``loops``) -- is refused,
    by every operator alike.  PyG returns the root / skip / bias term alone there; here the per-entry arrays would be empty
    tensors whose null pointer the library takes for a missing argument."""
    if isinstance(edge_index, torch.Tensor) and edge_index.dim() == 2 and edge_index.shape[1] == 0 and not loops:
        raise ValueError("%s: edge_index has no edge and no self loops are added: a graph without any entry is not supported on "
                         "the HIP path (the result would be the root / skip / bias term alone)" % name)


def _need_gpu(name, x, edge_attr=None, exc=None):
    """x (and ``edge_attr``, where the operator takes one) must be on the GPU.  ``exc``: ``ops.DdmpError`` unless given (GATv2Conv,
    TransformerConv and ResGatedGraphConv raise ``ValueError``)."""
    if x.is_cuda and (edge_attr is None or edge_attr.is_cuda):
        return
    what = "x must be a CUDA (ROCm) tensor" if edge_attr is None else "x and edge_attr must be CUDA (ROCm) tensors"
    raise (exc or ops.DdmpError)("%s runs on the HIP path only: %s, there is no CPU fallback" % (name, what))


def _check_pseudo(name, x, edge_attr, n_edges, dim, no_grad=False):
    """GMMConv's and SplineConv's refusals for the pseudo-coordinates ``edge_attr`` [E, dim], then the GPU requirement on both
    tensors.  ``no_grad``: SplineConv has no gradient with respect to them."""
    if not isinstance(edge_attr, torch.Tensor):
        raise ValueError("%s: edge_attr (the pseudo-coordinates, [E, %d]) is required" % (name, dim))
    if edge_attr.dim() != 2 or tuple(edge_attr.shape) != (n_edges, dim):
        raise ValueError("%s: edge_attr must be [%d, %d], got %s" % (name, n_edges, dim, tuple(edge_attr.shape)))
    if edge_attr.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: edge_attr must be float32 or float64, got %s" % (name, edge_attr.dtype))
    if no_grad and edge_attr.requires_grad:
        raise ValueError("%s: the gradient with respect to edge_attr is not implemented on the HIP path: pass edge_attr.detach()" % name)
    _need_gpu(name, x, edge_attr)


class _GCNConvFn(_Fn):
    @staticmethod
    def forward(ctx, x, weight, bias, graph):
        cin, cout = weight.shape[1], weight.shape[0]
        xp = _pad_cols(x.detach().to(torch.float32))
        wp = _pad_cols(weight.detach())
        b = bias.detach().contiguous()
        agg_first = xp.shape[1] < cout
        if agg_first:
            p = ops.spmm(graph, xp)
            y = ops.gemm_nt(p, wp, bias=b)
            ctx.save_for_backward(p, wp)
        else:
            h = ops.gemm_nt(xp, wp)
            y = ops.spmm(graph, h, bias=b if cout % 4 == 0 else None)
            if cout % 4 != 0:
                y += b
            ctx.save_for_backward(xp, wp)
        ctx.graph, ctx.agg_first, ctx.cin = graph, agg_first, cin
        return y

    @staticmethod
    def _backward(ctx, dy):
        saved, wp = ctx.saved_tensors
        graph, cin = ctx.graph, ctx.cin
        dy = dy.contiguous()
        cout = dy.shape[1]
        dyp = _pad_cols(dy)
        wrow = _pad_rows_like(wp, dyp, cout)
        need_x = ctx.needs_input_grad[0]
        db = None
        if ctx.needs_input_grad[2]:
            db = _bias_grad(dy)
        if ctx.agg_first:
            dw = ops.gemm_tn(dyp, saved)
            dx = ops.spmm(graph, ops.gemm_nn(dyp, wrow)) if need_x else None
        else:
            dh = ops.spmm(graph, dyp)
            dw = ops.gemm_tn(dh, saved)
            dx = ops.gemm_nn(dh, wrow) if need_x else None
        dw = dw[:cout, :cin]
        if dx is not None:
            dx = dx[:, :cin]
        return dx, dw, db, None


class _GCNConvWFn(_Fn):
    """GCNConv on a VALUED graph (edge_weight and / or non-default options): Y = A (X W^T) + b with A = the graph's current
    values, which need not be symmetric -- the backward gathers with A^T (``transpose=True``: same structure, mirrored values).
    The edge_weight gradient is dL/dA per entry (``ops.sddmm`` of the gather's output gradient and the operand the gather
    consumed) pushed through the normalisation (``ops.graph_weight_grad``); it runs only when edge_weight requires grad.
    The gather's operand is SAVED, not recomputed: aggregate-first it is the padded X (saved anyway when x is not already
    padded: N x C_in x 4 bytes more), aggregate-last it is H = X W^T, kept between forward and backward only when the
    edge_weight gradient is wanted (N x C_out x 4 bytes) instead of a second forward GEMM in the backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, edge_weight, graph):
        cin, cout = weight.shape[1], weight.shape[0]
        xp = _pad_cols(x.detach().to(torch.float32))
        wp = _pad_cols(weight.detach())
        b = None if bias is None else bias.detach().contiguous()
        agg_first = xp.shape[1] < cout
        need_ew = edge_weight is not None and edge_weight.requires_grad
        if agg_first:
            p = ops.spmm(graph, xp)
            y = ops.gemm_nt(p, wp, bias=b)
            ctx.save_for_backward(p, wp, xp if need_ew else None, graph.values_src)
        else:
            h = ops.gemm_nt(xp, wp)
            y = ops.spmm(graph, h, bias=b if cout % 4 == 0 else None)
            if cout % 4 != 0 and b is not None:
                y += b
            ctx.save_for_backward(xp, wp, h if need_ew else None, graph.values_src)
        ctx.graph, ctx.agg_first, ctx.cin, ctx.has_bias = graph, agg_first, cin, bias is not None
        # the values this call ran on: another weight version may have been set on the same structure before the backward (the
        # weights are saved through autograd, so an in-place change of them in between is an error, not a wrong restore)
        ctx.values_key = graph.values_key
        ctx.ew_dtype = None if edge_weight is None else edge_weight.dtype
        return y

    @staticmethod
    def _backward(ctx, dy):
        saved, wp, operand, wsrc = ctx.saved_tensors
        graph, cin = ctx.graph, ctx.cin
        ops.restore_values(graph, ctx.values_key, wsrc)
        dy = dy.contiguous()
        cout = dy.shape[1]
        dyp = _pad_cols(dy)
        wrow = _pad_rows_like(wp, dyp, cout)
        need_x, need_ew = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _bias_grad(dy)
        dew = None
        if ctx.agg_first:
            dw = ops.gemm_tn(dyp, saved)
            dp = ops.gemm_nn(dyp, wrow) if (need_x or need_ew) else None
            dx = ops.spmm(graph, dp, transpose=True) if need_x else None
            if need_ew:
                dew = ops.graph_weight_grad(graph, ops.sddmm(graph, dp, operand))
        else:
            dh = ops.spmm(graph, dyp, transpose=True)
            dw = ops.gemm_tn(dh, saved)
            dx = ops.gemm_nn(dh, wrow) if need_x else None
            if need_ew:
                dew = ops.graph_weight_grad(graph, ops.sddmm(graph, dy, operand))
        dw = dw[:cout, :cin]
        if dx is not None:
            dx = dx[:, :cin]
        if dew is not None:
            dew = dew.to(ctx.ew_dtype)
        return dx, dw, db, dew, None


class _Lin(nn.Module):
    """Holder so that the weight is addressed as ``conv.lin.weight`` like PyG's ``Linear``."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))


class GCNConv(nn.Module):
    """``torch_geometric.nn.GCNConv`` 2.2.0 on the HIP kernels: same constructor / call signature, parameter names and
    initialisation, with the defaults the reference uses (``util/networks.py:15-26``: ``GCNConv(in_channels, out_channels)``;
    ``:51-62``: ``conv(x, edge_index)``): ``lin.weight`` [out, in] Glorot-uniform, ``bias`` [out] zeros,
    ``Y = D^-1/2 (A + I) D^-1/2 (X W^T) + b``, differentiable w.r.t. x, weight and bias.  The normalised graph is built once per
    ``edge_index`` tensor (cached on its storage + version) instead of on every call; aggregation runs on min(in, out) channels.
    The other options and ``edge_weight``: the module docstring."""

    def __init__(self, in_channels: int, out_channels: int, improved: bool = False, cached: bool = False,
                 add_self_loops: bool = True, normalize: bool = True, bias: bool = True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached, self.add_self_loops, self.normalize = bool(improved), bool(cached), bool(add_self_loops), bool(normalize)
        self.lin = _Lin(in_channels, out_channels)
        _bias_param(self, bias, out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            _glorot_(self.lin.weight)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_weight=None) -> torch.Tensor:
        _check_x("GCNConv", x, self.in_channels, bf16=False)
        if edge_weight is not None:
            ops.check_edge_weight(edge_weight, edge_index.shape[1])
            if x.dtype == torch.bfloat16:
                raise ValueError("GCNConv: bf16 features with edge_weight are not supported on the HIP path")
        _need_gpu("GCNConv", x)
        _need_entries("GCNConv", edge_index, loops=self.add_self_loops and self.normalize)
        default = not self.improved and self.add_self_loops and self.normalize
        with ops.on_device(x):
            if edge_weight is None and default and self.bias is not None:
                graph = ops.graph_for(edge_index, x.shape[0])
                return _GCNConvFn.apply(x, self.lin.weight, self.bias, graph)
            if edge_weight is None and default:                  # bias=False alone: still the unvalued graph and gathers
                graph = ops.graph_for(edge_index, x.shape[0])
                zero = self.__dict__.get("_zero_bias")
                if zero is None or zero.device != x.device:
                    zero = self.__dict__["_zero_bias"] = torch.zeros(self.out_channels, dtype=torch.float32, device=x.device)
                return _GCNConvFn.apply(x, self.lin.weight, zero, graph)
            graph = ops.graph_for(edge_index, x.shape[0], "gcn", edge_weight, self.improved, self.add_self_loops, self.normalize)
            return _GCNConvWFn.apply(x, self.lin.weight, self.bias, edge_weight, graph)

    def extra_repr(self):
        return "%d, %d" % (self.in_channels, self.out_channels)


class _ChebConvFn(_Fn):
    """K - 1 fused Chebyshev steps (``ops.spmm_axpby``: gather + three-term recurrence in one launch) into the column
    blocks of ONE [N, K * Cp] buffer, then ONE GEMM against the packed [out, K * Cp] weight.  Backward: one dgrad GEMM,
    one wgrad GEMM, and dX by the Clenshaw recurrence on the same (symmetric) graph, in place in the dgrad's buffer."""

    @staticmethod
    def forward(ctx, x, bias, graph, alpha, beta, *weights):
        K = len(weights)
        cout, cin = weights[0].shape
        cp = (cin + 3) // 4 * 4
        n = x.shape[0]
        t = torch.empty((n, K * cp), dtype=torch.float32, device=x.device)
        if cp != cin:
            t[:, cin:cp] = 0
        t[:, :cin] = x.detach()
        wp = torch.zeros((cout, K * cp), dtype=torch.float32, device=x.device)
        for k, w in enumerate(weights):
            wp[:, k * cp:k * cp + cin] = w.detach()
        blk = lambda m, k: m[:, k * cp:(k + 1) * cp]
        for k in range(1, K):
            if k == 1:
                ops.spmm_axpby(graph, blk(t, 0), out=blk(t, 1), a=alpha, b=beta)
            else:
                ops.spmm_axpby(graph, blk(t, k - 1), out=blk(t, k), z=blk(t, k - 2), a=2 * alpha, b=2 * beta, c=-1.0)
        y = ops.gemm_nt(t, wp, bias=None if bias is None else bias.detach().contiguous())
        # a valued graph (edge_weight) holds the values of the LAST weight version set on its structure: record this call's
        valued = graph is not None and getattr(graph, "valued", 0)
        ctx.save_for_backward(t, wp, graph.values_src if valued else None)
        ctx.values_key = graph.values_key if valued else None
        ctx.graph, ctx.coef, ctx.dims, ctx.has_bias = graph, (alpha, beta), (K, cin, cp), bias is not None
        return y

    @staticmethod
    def _backward(ctx, dy):
        t, wp, wsrc = ctx.saved_tensors
        graph, (alpha, beta), (K, cin, cp) = ctx.graph, ctx.coef, ctx.dims
        if ctx.values_key is not None:
            ops.restore_values(graph, ctx.values_key, wsrc)
        dy = dy.contiguous()
        cout = dy.shape[1]
        dyp = _pad_cols(dy)
        db = None
        if ctx.has_bias and ctx.needs_input_grad[1]:
            db = _bias_grad(dy)
        dwp = ops.gemm_tn(dyp, t)
        dws = tuple(dwp[:cout, k * cp:k * cp + cin] if ctx.needs_input_grad[5 + k] else None for k in range(K))
        dx = None
        if ctx.needs_input_grad[0]:
            g = ops.gemm_nn(dyp, _pad_rows_like(wp, dyp, cout))     # blocks G_k = dY . W_k
            blk = lambda k: g[:, k * cp:(k + 1) * cp] if k < K else None
            # Clenshaw: B_k = G_k + 2 L^ B_{k+1} - B_{k+2} (B_K = B_{K+1} = 0), dX = G_0 + L^ B_1 - B_2; B_k overwrites G_k
            for k in range(K - 2, 0, -1):
                ops.spmm_axpby(graph, blk(k + 1), out=blk(k), z=blk(k), z2=blk(k + 2), a=2 * alpha, b=2 * beta, c=1.0, d=-1.0)
            if K > 1:
                ops.spmm_axpby(graph, blk(1), out=blk(0), z=blk(0), z2=blk(2), a=alpha, b=beta, c=1.0, d=-1.0)
            dx = g[:, :cin]
        return (dx, db, None, None, None) + dws


class ChebConv(nn.Module):
    """``torch_geometric.nn.ChebConv`` 2.2.0 on the HIP kernels, ``ChebConv(in_channels, out_channels, K,
    normalization="sym", bias=True)``: parameters ``lins.0.weight`` ... ``lins.{K-1}.weight`` [out, in] Glorot-uniform and ``bias``
    [out] zeros, ``forward(x, edge_index, edge_weight=None, batch=None, lambda_max=None)`` with ``lambda_max`` a float (default
    2.0), ``Y = sum_k T_k W_k^T + b``, ``T_0 = X``, ``T_1 = L^ X``, ``T_k = 2 L^ T_{k-1} - T_{k-2}``,
    ``L^ = -(2 / lambda_max) D^-1/2 A D^-1/2 + (2 / lambda_max - 1) I`` (no self loops; symmetric ``edge_index`` only).
    ``batch``, a tensor ``lambda_max`` and other normalisations raise.  ``edge_weight``: the module docstring."""

    def __init__(self, in_channels: int, out_channels: int, K: int, normalization: str = "sym", bias: bool = True):
        super().__init__()
        _int_ge1("ChebConv", "K", K, bool_ok=True)
        if normalization != "sym":
            raise ValueError("ChebConv: only normalization='sym' is implemented on the HIP path, got %r" % (normalization,))
        self.in_channels, self.out_channels, self.K, self.normalization = in_channels, out_channels, K, normalization
        self.lins = nn.ModuleList([_Lin(in_channels, out_channels) for _ in range(K)])
        _bias_param(self, bias, out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            for lin in self.lins:
                _glorot_(lin.weight)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x: torch.Tensor, edge_index: torch.Tensor, edge_weight=None, batch=None, lambda_max=None) -> torch.Tensor:
        """``edge_index`` must be symmetric (both directions of every edge present)."""
        _not_implemented("ChebConv", batch=batch)
        if edge_weight is not None:
            ops.check_edge_weight(edge_weight, edge_index.shape[1])
            if edge_weight.requires_grad:
                raise ValueError("ChebConv: the gradient with respect to edge_weight is not implemented on the HIP path "
                                 "(detach the weights; GCNConv has it)")
        if lambda_max is None:
            lambda_max = 2.0
        if isinstance(lambda_max, torch.Tensor) or not isinstance(lambda_max, (int, float)):
            raise ValueError("ChebConv: lambda_max must be a float (a tensor-valued lambda_max is not implemented)")
        if not lambda_max > 0:
            raise ValueError("ChebConv: lambda_max must be positive")
        _check_x("ChebConv", x, self.in_channels, bf16=False)
        _need_gpu("ChebConv", x)
        alpha, beta = -2.0 / lambda_max, 2.0 / lambda_max - 1.0
        with ops.on_device(x):
            graph = None                                         # K = 1 needs no graph
            if self.K > 1 or edge_weight is not None:            # (the weights are validated even then)
                graph = ops.graph_for(edge_index, x.shape[0], norm="sym", edge_weight=edge_weight)
            return _ChebConvFn.apply(x.to(torch.float32), self.bias, graph, alpha, beta, *[lin.weight for lin in self.lins])

    def extra_repr(self):
        return "%d, %d, K=%d, normalization=%s" % (self.in_channels, self.out_channels, self.K, self.normalization)


class _GATConvFn(_Fn):
    """Hf = X W^T (GEMM), the scores, then ONE launch for edge softmax + gather (``ops.gat_fwd``).  Saved: the padded x and weight,
    Hf, the scores and alpha [entries, heads].  Backward: the edge-side launch (ds per entry, ds_dst per node), the node-side launch
    (dHf completely, ds_src), the attention-vector reduction, then the two GEMMs of the linear map.  ``concat=False``: the mean
    over heads and its broadcast backward are torch ops around the kernels (``_heads_mean``)."""

    @staticmethod
    def forward(ctx, x, weight, att_src, att_dst, bias, graph, heads, concat, slope):
        cin, hc = weight.shape[1], weight.shape[0]
        C = hc // heads
        xp = _pad_cols(x.detach().to(torch.float32))
        wp = _pad_cols(weight.detach())
        asrc = att_src.detach().reshape(heads, C).contiguous()
        adst = att_dst.detach().reshape(heads, C).contiguous()
        hf = ops.gemm_nt(xp, wp)
        s_src, s_dst = ops.gat_scores(hf, asrc, adst, heads)
        b = None if bias is None else bias.detach().contiguous()
        y, alpha = ops.gat_fwd(graph, hf, s_src, s_dst, heads, slope, bias=b if concat else None)
        if not concat:
            y = _heads_mean(y, heads, b)
        ctx.save_for_backward(xp, wp, hf, s_src, s_dst, alpha, asrc, adst)
        ctx.graph, ctx.dims, ctx.has_bias = graph, (cin, heads, C, concat, slope), bias is not None
        return y

    @staticmethod
    def _backward(ctx, dy):
        xp, wp, hf, s_src, s_dst, alpha, asrc, adst = ctx.saved_tensors
        graph, (cin, heads, C, concat, slope) = ctx.graph, ctx.dims
        hc = heads * C
        dy = dy.contiguous().to(torch.float32)
        db = None
        if ctx.has_bias and ctx.needs_input_grad[4]:
            db = _bias_grad(dy)
        dout = dy if concat else _heads_mean_bwd(dy, heads)
        ds, ds_dst = ops.gat_bwd_edge(graph, dout, hf, s_src, s_dst, alpha, heads, slope)
        dhf, ds_src = ops.gat_bwd_node(graph, dout, alpha, ds, ds_dst, asrc, adst, heads)
        datt_src = datt_dst = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            datt_src, datt_dst = ops.gat_datt(hf, ds_src, ds_dst, heads)
            datt_src, datt_dst = datt_src.view(1, heads, C), datt_dst.view(1, heads, C)
        dhp = _pad_cols(dhf)
        dw = ops.gemm_tn(dhp, xp)[:hc, :cin] if ctx.needs_input_grad[1] else None
        dx = ops.gemm_nn(dhp, _pad_rows_like(wp, dhp, hc))[:, :cin] if ctx.needs_input_grad[0] else None
        return dx, dw, datt_src, datt_dst, db, None, None, None, None


class GATConv(nn.Module):
    """``torch_geometric.nn.GATConv`` 2.2.0 on the HIP kernels, ``GATConv(in_channels, out_channels, heads=1,
    concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True, edge_dim=None, fill_value="mean", bias=True)``,
    ``forward(x, edge_index, edge_attr=None, size=None, return_attention_weights=None)`` (written from the published source from
    memory -- PyG cannot be installed here, so this could not be checked against it; the pin is the float64 restatement
    ``tests/gat_ref.py``):

    * parameters ``lin_src.weight`` [heads * out, in] Glorot-uniform (``a = sqrt(6 / (in + heads * out))``); ``lin_dst`` IS
      ``lin_src`` (``in_channels`` is an int), so ``state_dict()`` carries both keys and ``parameters()`` yields the weight once;
      ``att_src`` / ``att_dst`` [1, heads, out] Glorot (``a = sqrt(6 / (heads + out))``); ``bias`` zeros, [heads * out] when
      ``concat``, else [out].
    * ``Hf = x lin_src.weight^T`` viewed [N, heads, C]; ``s_src[j,h] = sum_c Hf[j,h,c] att_src[h,c]``, ``s_dst`` likewise; with
      ``add_self_loops`` explicit self loops are removed and every node gets exactly one loop; for an edge j -> i
      ``z = leaky_relu(s_src[j,h] + s_dst[i,h], negative_slope)``; ``alpha`` = softmax of z over ALL edges with target i, per head
      (duplicate edges each take part); ``out[i,h,:] = sum alpha Hf[j,h,:]``; ``concat``: [N, heads * C], else the mean over heads;
      the bias is added last.  A node without incoming entries (``add_self_loops=False`` only) gets a zero aggregate plus bias.
    * one launch for scores, one for edge softmax + gather (``ops.gat_fwd``), two for the backward of the graph part
      (``ops.gat_bwd_edge`` / ``ops.gat_bwd_node``), a two-stage reduction for the attention vectors; the dense part goes through
      the GEMMs.  The graph is ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=...)``: the coalesced structure whose
      per-entry multiplicity weighs the softmax terms -- exact for duplicate edges.  Symmetric edge STRUCTURE only.
    * differentiable w.r.t. x, ``lin_src.weight``, ``att_src``, ``att_dst`` and ``bias``; float32, bitwise reproducible.
    * refused with ``ValueError`` before any launch: ``dropout != 0`` in training mode, ``edge_dim`` / ``edge_attr``, tuple
      ``in_channels`` or a tuple ``x`` (bipartite), ``size``, ``return_attention_weights``, bf16 features."""

    def __init__(self, in_channels, out_channels: int, heads: int = 1, concat: bool = True, negative_slope: float = 0.2,
                 dropout: float = 0.0, add_self_loops: bool = True, edge_dim=None, fill_value="mean", bias: bool = True):
        super().__init__()
        _no_tuple_channels("GATConv", in_channels)
        _not_implemented("GATConv", edge_dim=edge_dim)
        _int_ge1("GATConv", "heads", heads, bool_ok=True)
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = bool(concat), float(negative_slope), float(dropout)
        self.add_self_loops, self.edge_dim, self.fill_value = bool(add_self_loops), None, fill_value
        self.lin_src = _Lin(in_channels, heads * out_channels)
        self.lin_dst = self.lin_src                              # PyG: one Linear under both names when in_channels is an int
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        _bias_param(self, bias, heads * out_channels if concat else out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            _glorot_(self.lin_src.weight)
            _glorot_(self.att_src)
            _glorot_(self.att_dst)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x, edge_index, edge_attr=None, size=None, return_attention_weights=None) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present)."""
        _no_tuple_x("GATConv", x)
        _not_implemented("GATConv", edge_attr=edge_attr, size=size, return_attention_weights=return_attention_weights)
        _no_attention_dropout("GATConv", self)
        _check_x("GATConv", x, self.in_channels)
        _need_gpu("GATConv", x)
        _need_entries("GATConv", edge_index, loops=self.add_self_loops)
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=self.add_self_loops)
            return _GATConvFn.apply(x, self.lin_src.weight, self.att_src, self.att_dst, self.bias, graph, self.heads, self.concat,
                                    self.negative_slope)

    def extra_repr(self):
        return "%d, %d, heads=%d" % (self.in_channels, self.out_channels, self.heads)


class _GATv2ConvFn(_Fn):
    """ONE GEMM against the packed weight [lin_l.weight ; lin_r.weight] (``wr`` None = ``share_weights``: lin_l.weight alone) with
    the packed lin biases as a row broadcast gives the row buffer [Xl | Xr], then ONE launch for the per-edge scores + edge softmax
    + gather (``ops.gatv2_fwd``).  Saved: the padded x, the packed weight, the row buffer, alpha [entries, heads] and att.
    Backward: the edge-side launch (dz per entry, dXr, the rows' shares of datt), the node-side launch (dXl), both into ONE row
    buffer [dXl | dXr] (shared weights: dXr is added into dXl), the datt column sum, the lin bias gradients as column sums of that
    buffer, then ONE wgrad and ONE dgrad GEMM on it.  ``concat=False``: the mean over heads and its broadcast backward are torch
    ops around the kernels, as in ``_GATConvFn``."""

    @staticmethod
    def forward(ctx, x, wl, bl, wr, br, att, bias, graph, heads, concat, slope):
        xp, wp, buf, spans = _packed_gemm(x, (wl, wr), (bl, br))   # buf [N, hc or 2 hc, rounded up to 4]: Xl | Xr | zero padding
        xl = _cols(buf, spans[0])
        xr = xl if wr is None else _cols(buf, spans[1])
        a = att.detach().reshape(heads, wl.shape[0] // heads).contiguous()
        b = None if bias is None else bias.detach().contiguous()
        y, alpha = ops.gatv2_fwd(graph, xl, xr, a, heads, slope, bias=b if concat else None)
        if not concat:
            y = _heads_mean(y, heads, b)
        ctx.save_for_backward(xp, wp, buf, alpha, a)
        ctx.graph, ctx.spans, ctx.dims = graph, spans, (wl.shape[1], heads, concat, slope)
        return y

    @staticmethod
    def _backward(ctx, dy):
        xp, wp, buf, alpha, a = ctx.saved_tensors
        graph, (sl, sr), (cin, heads, concat, slope) = ctx.graph, ctx.spans, ctx.dims
        need = ctx.needs_input_grad
        dy = dy.contiguous().to(torch.float32)
        db = _bias_grad(dy) if need[6] else None
        dout = dy if concat else _heads_mean_bwd(dy, heads)
        xl = _cols(buf, sl)
        xr = xl if sr is None else _cols(buf, sr)
        g = _grad_rows(dy.shape[0], ctx.spans, wp.shape[0], dy.device)         # [dXl | dXr | 0]
        dz, dxr, part = ops.gatv2_bwd_edge(graph, dout, xl, xr, a, alpha, heads, slope, out=_cols(g, sr), want_datt=need[5])
        ops.gatv2_bwd_node(graph, dout, xl, xr, a, alpha, dz, heads, slope, out=_cols(g, sl))
        if sr is None:                                           # share_weights: Xr is Xl
            g[:, :sl[1]] += dxr
        datt = ops.gatv2_datt(part, heads).view(1, heads, -1) if need[5] else None
        dx, (dwl, dwr), (dbl, dbr) = _packed_grads(g, xp, wp, ctx.spans, cin, (need[1], need[3]), (need[2], need[4]), need[0])
        return dx, dwl, dbl, dwr, dbr, datt, db, None, None, None, None


class _LinB(_Lin):
    """``_Lin`` with PyG ``Linear``'s optional bias [out]."""

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__(in_channels, out_channels)
        _bias_param(self, bias, out_channels, torch.empty)


class GATv2Conv(nn.Module):
    """``torch_geometric.nn.GATv2Conv`` 2.2.0 on the HIP kernels (restated from the published source from memory --
    PyG cannot be installed here, so this could not be checked against it; the pin is the float64 restatement
    ``tests/gatv2_ref.py``).

    * parameters ``lin_l`` / ``lin_r``: ``weight`` [heads * out, in] Glorot-uniform and ``bias`` [heads * out]
      uniform(-1/sqrt(in), 1/sqrt(in)) (absent with ``bias=False``); ``share_weights=True``: ONE module under both names; ``att``
      [1, heads, out] Glorot; ``bias`` zeros, [heads * out] when ``concat``, else [out].
    * ``Xl = lin_l(x)``, ``Xr = lin_r(x)`` viewed [N, heads, C]; with ``add_self_loops`` explicit self loops are removed and every
      node gets exactly one; for an edge j -> i ``z[h] = sum_c att[h,c] leaky_relu(Xl[j,h,c] + Xr[i,h,c], negative_slope)``;
      ``alpha`` = softmax of z over ALL edges with target i, per head (duplicate edges each take part);
      ``out[i,h,:] = sum alpha Xl[j,h,:]``; ``concat``: [N, heads * C], else the mean over heads; the bias is added last.
    * differentiable w.r.t. x, the ``lin_*`` weights and biases, ``att`` and ``bias``; float32, bitwise reproducible.  The graph is
      GATConv's: ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=...)``.  Symmetric edge STRUCTURE only.
    * refused with ``ValueError`` before any launch: tuple ``in_channels`` or a tuple ``x`` (bipartite), ``edge_dim`` /
      ``edge_attr``, ``size``, ``return_attention_weights``, ``dropout != 0`` in training mode, bf16 features, CPU tensors."""

    def __init__(self, in_channels, out_channels: int, heads: int = 1, concat: bool = True, negative_slope: float = 0.2,
                 dropout: float = 0.0, add_self_loops: bool = True, edge_dim=None, fill_value="mean", bias: bool = True,
                 share_weights: bool = False):
        super().__init__()
        _no_tuple_channels("GATv2Conv", in_channels)
        _not_implemented("GATv2Conv", edge_dim=edge_dim)
        _int_ge1("GATv2Conv", "heads", heads)
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = bool(concat), float(negative_slope), float(dropout)
        self.add_self_loops, self.edge_dim, self.fill_value = bool(add_self_loops), None, fill_value
        self.share_weights = bool(share_weights)
        self.lin_l = _LinB(in_channels, heads * out_channels, bias)
        self.lin_r = self.lin_l if self.share_weights else _LinB(in_channels, heads * out_channels, bias)
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        _bias_param(self, bias, heads * out_channels if concat else out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        c = 1.0 / math.sqrt(self.in_channels)
        with torch.no_grad():
            for lin in (self.lin_l,) if self.share_weights else (self.lin_l, self.lin_r):
                _glorot_(lin.weight)
                if lin.bias is not None:
                    lin.bias.uniform_(-c, c)
            _glorot_(self.att)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x, edge_index, edge_attr=None, size=None, return_attention_weights=None) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present)."""
        _no_tuple_x("GATv2Conv", x)
        _not_implemented("GATv2Conv", edge_attr=edge_attr, size=size, return_attention_weights=return_attention_weights)
        _no_attention_dropout("GATv2Conv", self)
        _check_x("GATv2Conv", x, self.in_channels)
        _need_gpu("GATv2Conv", x, exc=ValueError)
        _need_entries("GATv2Conv", edge_index, loops=self.add_self_loops)
        share = self.share_weights
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=self.add_self_loops)
            return _GATv2ConvFn.apply(x, self.lin_l.weight, self.lin_l.bias, None if share else self.lin_r.weight,
                                      None if share else self.lin_r.bias, self.att, self.bias, graph, self.heads, self.concat,
                                      self.negative_slope)

    def extra_repr(self):
        return "%d, %d, heads=%d, share_weights=%s" % (self.in_channels, self.out_channels, self.heads, self.share_weights)


class _TransformerConvFn(_Fn):
    """ONE GEMM against the packed weight [lin_query.weight ; lin_key.weight ; lin_value.weight ; lin_skip.weight] (``ws`` None =
    ``root_weight=False``: no skip block) with the packed lin biases as a row broadcast gives the row buffer [Q | K | V | S], then
    ONE launch for the dot-product scores + edge softmax + gather (``ops.tconv_fwd``).  Saved: the padded x, the packed weight, the
    row buffer and alpha [entries, heads].  Backward: the edge-side launch (dz per entry, dQ) and the node-side launch (dK, dV),
    both into ONE row buffer [dQ | dK | dV | dS], the lin bias gradients as column sums of that buffer, then ONE wgrad and ONE
    dgrad GEMM on it.  Where the skip goes: ``concat`` without ``beta`` -- added in the forward kernel's epilogue, dS filled by
    the node-side launch; ``concat=False`` -- the mean over heads, its broadcast backward and the [N, C] skip add are torch ops
    around the kernels, as in ``_GATv2ConvFn``; ``beta`` -- the function returns (m, x_r) with x_r a view of the S block, and the
    gradient of x_r lands in the dS block (the gate itself is the module's)."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, bv, ws, bs, graph, heads, concat, beta):
        # buf [N, 3 hc + the skip's width (hc when concat, else C; absent without root), rounded up to 4]: Q | K | V | S | zero padding
        xp, wp, buf, spans = _packed_gemm(x, (wq, wk, wv, ws), (bq, bk, bv, bs))
        q, k, v, s = (_cols(buf, sp) for sp in spans)
        fused_skip = bool(concat and s is not None and not beta)
        y, alpha = ops.tconv_fwd(graph, q, k, v, heads, skip=s if fused_skip else None)
        if not concat:
            y = _heads_mean(y, heads, None if beta else s)
        ctx.save_for_backward(xp, wp, buf, alpha)
        ctx.graph, ctx.spans, ctx.dims = graph, spans, (wq.shape[1], heads, concat, beta, fused_skip)
        return (y, s) if beta else y

    @staticmethod
    def _backward(ctx, dy, dxr=None):
        xp, wp, buf, alpha = ctx.saved_tensors
        graph, spans, (cin, heads, concat, beta, fused_skip) = ctx.graph, ctx.spans, ctx.dims
        need = ctx.needs_input_grad
        dy = dy.contiguous().to(torch.float32)
        dout = dy if concat else _heads_mean_bwd(dy, heads)
        q, k, v, _ = (_cols(buf, sp) for sp in spans)
        g = _grad_rows(dy.shape[0], spans, wp.shape[0], dy.device)             # [dQ | dK | dV | dS | 0]
        gq, gk, gv, gs = (_cols(g, sp) for sp in spans)
        dz, _ = ops.tconv_bwd_edge(graph, dout, k, v, alpha, heads, out=gq)
        ops.tconv_bwd_node(graph, dout, q, alpha, dz, heads, out_k=gk, out_v=gv, out_s=gs if fused_skip else None)
        if gs is not None and not fused_skip:
            gs.copy_(dxr.to(torch.float32) if beta else dy)
        dx, (dwq, dwk, dwv, dws), (dbq, dbk, dbv, dbs) = _packed_grads(g, xp, wp, spans, cin, need[1:8:2], need[2:9:2], need[0])
        return dx, dwq, dbq, dwk, dbk, dwv, dbv, dws, dbs, None, None, None, None


class TransformerConv(nn.Module):
    """``torch_geometric.nn.TransformerConv`` 2.2.0 (Shi et al., "Masked Label Prediction", IJCAI 2021) on the HIP kernels
    (restated from the published source from memory -- PyG cannot be installed here, so this could not be checked
    against it; the pin is the float64 restatement ``tests/transformer_ref.py``).  It is the one operator here whose scored
    stream (K) differs from its gathered stream (V).

    * parameters ``lin_key`` / ``lin_query`` / ``lin_value``: ``weight`` [heads * out, in] and ``bias`` [heads * out] (always
      present); ``lin_skip``: ``weight`` [heads * out, in] when ``concat``, else [out, in], its ``bias`` only with ``bias=True`` (the
      module exists whatever ``root_weight`` says); ``lin_beta.weight`` [1, 3 * heads * out] when ``concat``, else [1, 3 * out],
      no bias, only with ``beta=True`` and ``root_weight=True`` (else registered as None); ``lin_edge`` is registered as None.
      Everything is uniform(-1/sqrt(in), 1/sqrt(in)) with "in" the layer's own input width.
    * ``Q = lin_query(x)``, ``K = lin_key(x)``, ``V = lin_value(x)`` viewed [N, heads, C]; for an edge j -> i
      ``z[h] = Q[i,h,:] . K[j,h,:] / sqrt(C)``; ``alpha`` = softmax of z over ALL edges with target i, per head (duplicate edges
      each take part); ``m[i,h,:] = sum alpha V[j,h,:]``; ``concat``: [N, heads * C], else the mean over heads.  No self loops are
      added, an explicit loop is an ordinary edge, a node without incoming edges has ``m = 0``.
    * ``root_weight``: ``x_r = lin_skip(x)``; ``out = m + x_r``, or with ``beta``
      ``b = sigmoid(lin_beta(cat[m, x_r, m - x_r]))`` (one scalar per node) and ``out = b x_r + (1 - b) m``.  The gate is torch
      elementwise ops on [N, .] tensors; no per-edge tensor and no ``index_add_`` exist at any point.
    * differentiable w.r.t. x and every parameter in use; float32, bitwise reproducible.  The graph is EdgeConv's and GMMConv's:
      ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=False)``.  Symmetric edge STRUCTURE only.
    * refused with ``ValueError`` before any launch: ``edge_dim`` / ``edge_attr``, ``dropout != 0`` in training mode, tuple
      ``in_channels`` or a tuple ``x`` (bipartite), ``return_attention_weights``, bf16 features, CPU tensors, ``heads < 1``, an
      ``x`` that is not [N, in]."""

    def __init__(self, in_channels, out_channels: int, heads: int = 1, concat: bool = True, beta: bool = False,
                 dropout: float = 0.0, edge_dim=None, bias: bool = True, root_weight: bool = True):
        super().__init__()
        _no_tuple_channels("TransformerConv", in_channels)
        _not_implemented("TransformerConv", edge_dim=edge_dim)
        _int_ge1("TransformerConv", "heads", heads)
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.root_weight, self.dropout, self.edge_dim = bool(concat), bool(root_weight), float(dropout), None
        self.beta = bool(beta) and self.root_weight
        hc = heads * out_channels
        sw = hc if self.concat else out_channels
        self.lin_key = _LinB(in_channels, hc)
        self.lin_query = _LinB(in_channels, hc)
        self.lin_value = _LinB(in_channels, hc)
        self.register_parameter("lin_edge", None)
        self.lin_skip = _LinB(in_channels, sw, bias)
        if self.beta:
            self.lin_beta = _LinB(3 * sw, 1, bias=False)
        else:
            self.register_parameter("lin_beta", None)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip, self.lin_beta):
                if lin is not None:
                    _reset_linear(lin)

    def forward(self, x, edge_index, edge_attr=None, return_attention_weights=None) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present)."""
        _no_tuple_x("TransformerConv", x)
        _not_implemented("TransformerConv", edge_attr=edge_attr, return_attention_weights=return_attention_weights)
        _no_attention_dropout("TransformerConv", self)
        _check_x("TransformerConv", x, self.in_channels)
        _need_gpu("TransformerConv", x, exc=ValueError)
        _need_entries("TransformerConv", edge_index)
        root = self.root_weight
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=False)
            out = _TransformerConvFn.apply(x, self.lin_query.weight, self.lin_query.bias, self.lin_key.weight, self.lin_key.bias,
                                           self.lin_value.weight, self.lin_value.bias, self.lin_skip.weight if root else None,
                                           self.lin_skip.bias if root else None, graph, self.heads, self.concat, self.beta)
        if not self.beta:
            return out
        m, x_r = out
        b = torch.sigmoid(torch.cat([m, x_r, m - x_r], dim=-1) @ self.lin_beta.weight.t())
        return b * x_r + (1 - b) * m

    def extra_repr(self):
        return "%d, %d, heads=%d, concat=%s, beta=%s, root_weight=%s" % (self.in_channels, self.out_channels, self.heads,
                                                                          self.concat, self.beta, self.root_weight)


class _ResGatedFn(_Fn):
    """ONE GEMM against the packed weight [lin_key.weight ; lin_query.weight ; lin_value.weight ; lin_skip.weight] (``ws`` None =
    ``root_weight=False``: no skip block) with the packed lin biases as a row broadcast (a zero block for the skip) gives the row
    buffer [K | Q | V | S], then ONE launch for the per-channel gate + gather with S and ``bias`` as the start of the sums
    (``ops.rgate_fwd``).  Saved: the padded x, the packed weight and the row buffer -- nothing per entry.  Backward: the row-side
    launch (dK) and the node-side launch (dQ, dV, and dS = dy copied into the skip block), both recomputing the gate, into ONE
    row buffer [dK | dQ | dV | dS], the lin bias gradients as column sums of its blocks, then ONE wgrad and ONE dgrad GEMM on
    it."""

    @staticmethod
    def forward(ctx, x, wk, bk, wq, bq, wv, bv, ws, bias, graph):
        xp, wp, buf, spans = _packed_gemm(x, (wk, wq, wv, ws), (bk, bq, bv, None))   # buf: K | Q | V | S | zero padding
        k, q, v, s = (_cols(buf, sp) for sp in spans)
        b = None if bias is None else bias.detach().to(torch.float32).contiguous()
        y = ops.rgate_fwd(graph, k, q, v, skip=s, bias=b)
        ctx.save_for_backward(xp, wp, buf)
        ctx.graph, ctx.spans, ctx.cin = graph, spans, wk.shape[1]
        return y

    @staticmethod
    def _backward(ctx, dy):
        xp, wp, buf = ctx.saved_tensors
        graph, spans, need = ctx.graph, ctx.spans, ctx.needs_input_grad
        dy = dy.contiguous().to(torch.float32)
        k, q, v, _ = (_cols(buf, sp) for sp in spans)
        g = _grad_rows(dy.shape[0], spans, wp.shape[0], dy.device)             # [dK | dQ | dV | dS | 0]
        gk, gq, gv, gs = (_cols(g, sp) for sp in spans)
        ops.rgate_bwd_row(graph, dy, k, q, v, out=gk)
        ops.rgate_bwd_node(graph, dy, k, q, v, out_q=gq, out_v=gv, out_s=gs)
        # the lin bias gradients here, not in _packed_grads: they come before db, as they always have (same launches, same order)
        dbk, dbq, dbv = (_bias_grad(b) if n else None for b, n in zip((gk, gq, gv), need[2:7:2]))
        db = _bias_grad(dy) if need[8] else None
        dx, (dwk, dwq, dwv, dws), _ = _packed_grads(g, xp, wp, spans, ctx.cin, need[1:8:2], None, need[0])
        return dx, dwk, dbk, dwq, dbq, dwv, dbv, dws, db, None


class ResGatedGraphConv(nn.Module):
    """``torch_geometric.nn.ResGatedGraphConv`` 2.2.0 (Bresson & Laurent, "Residual Gated Graph ConvNets", 2017) on the HIP
    kernels (restated from the published source from memory -- PyG cannot be installed here, so this could not be
    checked against it; the pin is the float64 restatement ``tests/resgated_ref.py``).  It is the one operator here whose edge
    weight is as wide as the features: a per-channel gate, not a scalar per head.

    * parameters ``lin_key`` / ``lin_query`` / ``lin_value``: ``weight`` [out, in] and ``bias`` [out] (always present);
      ``lin_skip``: ``weight`` [out, in], no bias, registered as None with ``root_weight=False``; ``bias`` [out] zeros, registered
      as None with ``bias=False``.  The linear layers are uniform(-1/sqrt(in), 1/sqrt(in)).
    * ``K = lin_key(x)``, ``Q = lin_query(x)``, ``V = lin_value(x)``; for an edge j -> i the gate is PER CHANNEL,
      ``g = sigmoid(K[i,:] + Q[j,:])``; ``out[i,:] = lin_skip(x_i) + bias + sum_{j -> i} g * V[j,:]`` (duplicate edges each
      count).  No self loops are added, an explicit loop is an ordinary edge, a node without incoming edges returns
      ``lin_skip(x_i) + bias``.  No per-edge tensor and no ``index_add_`` exist at any point, in the backward either: it
      recomputes the gate.
    * differentiable w.r.t. x and every parameter in use; float32, bitwise reproducible.  The graph is EdgeConv's and
      TransformerConv's: ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=False)``.  Symmetric edge STRUCTURE only.
    * refused with ``ValueError`` before any launch: an ``act`` that is not a ``torch.nn.Sigmoid`` instance, ``aggr`` other than
      ``"add"``, tuple ``in_channels`` or a tuple ``x`` (bipartite), bf16 features, CPU tensors, an ``x`` that is not [N, in]."""

    def __init__(self, in_channels, out_channels: int, act=nn.Sigmoid(), root_weight: bool = True, bias: bool = True, **kwargs):
        super().__init__()
        _no_tuple_channels("ResGatedGraphConv", in_channels)
        if not isinstance(act, nn.Sigmoid):
            raise ValueError("ResGatedGraphConv: the gate of the HIP path is the sigmoid, act must be a torch.nn.Sigmoid, got %r"
                             % (act,))
        _check_aggr("ResGatedGraphConv", kwargs.pop("aggr", "add"), ("add",), kwargs, resgated=True)
        self.in_channels, self.out_channels, self.act, self.root_weight = in_channels, out_channels, act, bool(root_weight)
        self.lin_key = _LinB(in_channels, out_channels)
        self.lin_query = _LinB(in_channels, out_channels)
        self.lin_value = _LinB(in_channels, out_channels)
        if self.root_weight:
            self.lin_skip = _LinB(in_channels, out_channels, bias=False)
        else:
            self.register_parameter("lin_skip", None)
        _bias_param(self, bias, out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip):
                if lin is not None:
                    _reset_linear(lin)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x, edge_index) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present)."""
        _no_tuple_x("ResGatedGraphConv", x)
        _check_x("ResGatedGraphConv", x, self.in_channels)
        _need_gpu("ResGatedGraphConv", x, exc=ValueError)
        _need_entries("ResGatedGraphConv", edge_index)
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=False)
            return _ResGatedFn.apply(x, self.lin_key.weight, self.lin_key.bias, self.lin_query.weight, self.lin_query.bias,
                                     self.lin_value.weight, self.lin_value.bias,
                                     self.lin_skip.weight if self.root_weight else None, self.bias, graph)

    def extra_repr(self):
        return "%d, %d, root_weight=%s, bias=%s" % (self.in_channels, self.out_channels, self.root_weight, self.bias is not None)


class _FeaStConvFn(_Fn):
    """ONE GEMM against the packed weight [lin.weight; u.weight] (rows padded to a multiple of 4) gives the row buffer [Hf | P],
    then ONE launch for head softmax + gather (``ops.feast_fwd``).  Saved: the padded x, the packed weight, the [Hf | P] buffer and
    beta [entries, heads].  Backward: the edge-side launch (dz per entry, its row sums rs), the node-side launch that writes
    [dHf | dP] into one row buffer, the offset reduction dc = colsum(rs), then ONE wgrad GEMM ([dW; dU]) and ONE dgrad GEMM (dx)."""

    @staticmethod
    def forward(ctx, x, weight, u, c, bias, graph, heads):
        xp, wp, buf, spans = _packed_gemm(x, (weight, u))         # buf [N, hc + heads rounded up to 4]: Hf | P | zero padding
        b = None if bias is None else bias.detach().contiguous()
        y, beta = ops.feast_fwd(graph, _cols(buf, spans[0]), _cols(buf, spans[1]), c.detach().contiguous(), heads, bias=b)
        ctx.save_for_backward(xp, wp, buf, beta)
        ctx.graph, ctx.spans, ctx.dims = graph, spans, (weight.shape[1], heads)
        return y

    @staticmethod
    def _backward(ctx, dy):
        xp, wp, buf, beta = ctx.saved_tensors
        graph, spans, (cin, heads), need = ctx.graph, ctx.spans, ctx.dims, ctx.needs_input_grad
        dy = dy.contiguous().to(torch.float32)
        db = _bias_grad(dy) if need[4] else None
        dz, rs = ops.feast_bwd_edge(graph, dy, _cols(buf, spans[0]), beta, heads)
        g = _grad_rows(dy.shape[0], spans, wp.shape[0], dy.device)
        ops.feast_bwd_node(graph, dy, beta, dz, rs, heads, out=g)          # g = [dHf | dP | 0]
        dc = ops.feast_dc(rs, heads) if need[3] else None
        dx, (dw, du), _ = _packed_grads(g, xp, wp, spans, cin, need[1:3], None, need[0])
        return dx, dw, du, dc, db, None, None


class FeaStConv(nn.Module):
    """``torch_geometric.nn.FeaStConv`` 2.2.0 (Verma et al., FeaStNet, CVPR 2018) on the HIP kernels,
    ``FeaStConv(in_channels, out_channels, heads=1, add_self_loops=True, bias=True)``, ``forward(x, edge_index)`` (written from the
    published source from memory -- PyG cannot be installed here, so this could not be checked against it; the pin is the float64
    restatement ``tests/feast_ref.py``):

    * parameters ``lin.weight`` [heads * out, in] and ``u.weight`` [heads, in], both uniform(-1/sqrt(in), 1/sqrt(in)) and without
      bias; ``c`` [heads] and ``bias`` [out] normal(0, 0.1).  The initialisations are from memory too; the arithmetic is what the
      tests pin.
    * ``Hf = x lin.weight^T`` viewed [N, heads, out], ``P = x u.weight^T`` [N, heads]; with ``add_self_loops`` explicit self loops
      are removed and every node gets exactly one loop; for an edge j -> i ``q[h]`` = softmax over the HEADS of
      ``P[j,h] - P[i,h] + c[h]`` (translation invariant in x); ``out[i,:] = (1 / deg_i) sum_{j -> i} sum_h q[h] Hf[j,h,:] + bias``
      with ``deg_i`` the number of edges with target i (duplicates each count, the added loop counts).  A node without incoming
      edges (``add_self_loops=False`` only) gets the bias.  With ``heads=1`` this is the plain mean of ``x lin.weight^T`` over the
      neighbourhood.
    * one GEMM against the packed ``[lin.weight; u.weight]`` for ``[Hf | P]``, one launch for head softmax + gather
      (``ops.feast_fwd``), two for the backward of the graph part (``ops.feast_bwd_edge`` / ``ops.feast_bwd_node``), a two-stage
      reduction for ``c`` (``ops.feast_dc``), one wgrad GEMM for ``[dW; dU]`` and one dgrad GEMM for ``dx``.  No [E, heads * out]
      tensor exists at any point.  The graph is GATConv's: ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=...)``, same
      handle and cache key.  Symmetric edge STRUCTURE only.
    * differentiable w.r.t. x, ``lin.weight``, ``u.weight``, ``c`` and ``bias``; float32, bitwise reproducible.
    * refused with ``ValueError`` before any launch: tuple ``in_channels`` or a tuple ``x`` (bipartite), an ``aggr`` other than
      ``"mean"``, bf16 features, ``heads < 1``, an ``x`` that is not [N, in]."""

    def __init__(self, in_channels, out_channels: int, heads: int = 1, add_self_loops: bool = True, bias: bool = True, **kwargs):
        super().__init__()
        _no_tuple_channels("FeaStConv", in_channels)
        _check_aggr("FeaStConv", kwargs.pop("aggr", "mean"), ("mean",), kwargs)
        _int_ge1("FeaStConv", "heads", heads)
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.add_self_loops = bool(add_self_loops)
        self.lin = _Lin(in_channels, heads * out_channels)
        self.u = _Lin(in_channels, heads)
        self.c = nn.Parameter(torch.empty(heads))
        _bias_param(self, bias, out_channels, torch.empty)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            _reset_linear(self.lin)                              # (from memory of the published source, like the arithmetic)
            _reset_linear(self.u)
            self.c.normal_(0.0, 0.1)
            if self.bias is not None:
                self.bias.normal_(0.0, 0.1)

    def forward(self, x, edge_index) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present)."""
        _no_tuple_x("FeaStConv", x)
        _check_x("FeaStConv", x, self.in_channels)
        _need_gpu("FeaStConv", x)
        _need_entries("FeaStConv", edge_index, loops=self.add_self_loops)
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=self.add_self_loops)
            return _FeaStConvFn.apply(x, self.lin.weight, self.u.weight, self.c, self.bias, graph, self.heads)

    def extra_repr(self):
        return "%d, %d, heads=%d" % (self.in_channels, self.out_channels, self.heads)


class _GMMConvFn(_Fn):
    """ONE GEMM against the packed weight [g^T ; root.weight] (rows padded to a multiple of 4) gives the row buffer [Hf | R], then
    ONE launch for the per-edge Gaussians + gather + root + bias (``ops.gmm_fwd``).  Saved: the padded x, the packed weight, the
    [Hf | R] buffer, w [entries, K], the float32 pseudo-coordinates (and mu / sigma).  Backward: the edge-side launch (per-row
    partials of dmu / dsigma, dattr when wanted), the node-side launch that writes [dHf | dOut] into one row buffer, the column sum
    of the partials, then ONE wgrad GEMM ([dg^T ; droot]) and ONE dgrad GEMM (dx)."""

    @staticmethod
    def forward(ctx, x, g, mu, sigma, root, bias, attr, graph, K):
        xp, wp, buf, spans = _packed_gemm(x, (g.t(), root))       # buf [N, K * out (+ out) rounded up to 4]: Hf | R | zero padding
        b = None if bias is None else bias.detach().contiguous()
        a32 = attr.detach().to(torch.float32).contiguous()       # (float64 pseudo-coordinates are rounded once)
        m, s = mu.detach().contiguous(), sigma.detach().contiguous()
        y, w = ops.gmm_fwd(graph, _cols(buf, spans[0]), a32, m, s, K, root=_cols(buf, spans[1]), bias=b)
        ctx.save_for_backward(xp, wp, buf, w, a32, m, s)
        ctx.graph, ctx.spans, ctx.dims, ctx.attr_dtype = graph, spans, (g.shape[0], K), attr.dtype
        return y

    @staticmethod
    def _backward(ctx, dy):
        xp, wp, buf, w, a32, m, s = ctx.saved_tensors
        graph, spans, (cin, K), need = ctx.graph, ctx.spans, ctx.dims, ctx.needs_input_grad
        kd = m.numel()
        dy = dy.contiguous().to(torch.float32)
        db = _bias_grad(dy) if need[5] else None
        parts, dattr = ops.gmm_bwd_edge(graph, dy, _cols(buf, spans[0]), a32, m, s, K, want_dattr=need[6])
        gb = _grad_rows(dy.shape[0], spans, wp.shape[0], dy.device)
        ops.gmm_bwd_node(graph, dy, w, K, out=gb, root=spans[1] is not None)   # gb = [dHf | dOut | 0]
        dmu = dsigma = None
        if need[2] or need[3]:
            dms = ops.feast_dc(parts, 2 * kd)                    # [dmu | dsigma]
            dmu, dsigma = dms[:kd].view_as(m), dms[kd:].view_as(s)
        dx, (dgt, droot), _ = _packed_grads(gb, xp, wp, spans, cin, (need[1], need[4]), None, need[0])   # [dg^T ; droot]
        if dattr is not None:
            dattr = dattr.to(ctx.attr_dtype)
        return dx, None if dgt is None else dgt.t(), dmu, dsigma, droot, db, dattr, None, None


class GMMConv(nn.Module):
    """``torch_geometric.nn.GMMConv`` 2.2.0 (Monti et al., MoNet, CVPR 2017) on the HIP kernels, with
    ``separate_gaussians=False`` and mean aggregation: parameters ``g`` [in, K * out], ``mu`` / ``sigma`` [K, dim], ``root.weight``
    [out, in] (absent with ``root_weight=False``), all Glorot-uniform, and ``bias`` [out] zeros.  With ``Hf = x g`` viewed
    [N, K, out] and an edge t: j -> i with pseudo-coordinates ``a_t``:
    ``gamma_t[k] = exp(-1/2 sum_d (a_t[d] - mu[k,d])^2 / (1e-15 + sigma[k,d]^2))``,
    ``out[i] = (1 / deg_i) sum_{t -> i} sum_k gamma_t[k] Hf[j,k,:] + root(x_i) + bias``; no self loops are added, duplicate edges
    each count, a node without incoming edges gets ``root(x_i) + bias``.  Written from the published PyG source from memory --
    PyG cannot be installed here, so this could not be checked against it; the pin is the float64 restatement
    ``tests/gmm_ref.py``.  Differentiable w.r.t. x, every parameter, and ``edge_attr`` when it requires grad.

    * it is the one operator here that consumes the GEOMETRY of an edge: ``forward(x, edge_index, edge_attr, size=None)`` with
      ``edge_attr`` the per-edge pseudo-coordinates ([E, dim]; ``cartesian_pseudo`` below restates PyG's ``Cartesian`` transform).
      K = ``kernel_size``; an explicit loop is an ordinary edge; ``deg_i`` is the number of edges with target i.
    * the launches: ``_GMMConvFn``.  No [E, K * out] tensor and no ``index_add_`` exist at any point.  The graph is GATConv's
      without loops: ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=False)``, same handle and cache key; a coalesced
      entry sums the Gaussians of its input edges in input order, so duplicate edges with different pseudo-coordinates are exact.
      Symmetric edge STRUCTURE only.  float32, bitwise reproducible.
    * refused with ``ValueError`` before any launch: ``separate_gaussians=True``, ``aggr != "mean"``, tuple ``in_channels`` or a
      tuple ``x`` (bipartite), ``size``, bf16 features, ``edge_attr`` missing, not [E, dim] or not float32 / float64 (float64 is
      rounded to float32 once), ``kernel_size < 1``, ``dim < 1``, ``2 * kernel_size * dim > 256``."""

    def __init__(self, in_channels, out_channels: int, dim: int, kernel_size: int, separate_gaussians: bool = False,
                 aggr: str = "mean", root_weight: bool = True, bias: bool = True, **kwargs):
        super().__init__()
        _no_tuple_channels("GMMConv", in_channels)
        if separate_gaussians:
            raise ValueError("GMMConv: separate_gaussians=True is not implemented on the HIP path")
        _check_aggr("GMMConv", aggr, ("mean",), kwargs)
        _int_ge1("GMMConv", "kernel_size", kernel_size)
        _int_ge1("GMMConv", "dim", dim)
        if 2 * kernel_size * dim > 256:
            raise ValueError("GMMConv: 2 * kernel_size * dim must be <= 256 on the HIP path (the dmu / dsigma reduction), got %d"
                             % (2 * kernel_size * dim))
        self.in_channels, self.out_channels, self.dim, self.kernel_size = in_channels, out_channels, dim, kernel_size
        self.separate_gaussians, self.aggr = False, aggr
        self.g = nn.Parameter(torch.empty(in_channels, kernel_size * out_channels))
        self.mu = nn.Parameter(torch.empty(kernel_size, dim))
        self.sigma = nn.Parameter(torch.empty(kernel_size, dim))
        if root_weight:
            self.root = _Lin(in_channels, out_channels)
        else:
            self.register_parameter("root", None)
        _bias_param(self, bias, out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            _glorot_(self.g)
            _glorot_(self.mu)
            _glorot_(self.sigma)
            if self.root is not None:
                _glorot_(self.root.weight)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x, edge_index, edge_attr=None, size=None) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present); ``edge_attr``: [E, dim]
        pseudo-coordinates, float32 or float64 (rounded to float32 once)."""
        _no_tuple_x("GMMConv", x)
        _not_implemented("GMMConv", size=size)
        _check_x("GMMConv", x, self.in_channels)
        _check_pseudo("GMMConv", x, edge_attr, edge_index.shape[1], self.dim)
        _need_entries("GMMConv", edge_index)
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=False)
            return _GMMConvFn.apply(x, self.g, self.mu, self.sigma, None if self.root is None else self.root.weight, self.bias,
                                    edge_attr, graph, self.kernel_size)

    def extra_repr(self):
        return "%d, %d, dim=%d, kernel_size=%d" % (self.in_channels, self.out_channels, self.dim, self.kernel_size)


def cartesian_pseudo(pos: torch.Tensor, edge_index: torch.Tensor, norm: bool = True, max_value=None) -> torch.Tensor:
    """PyG's ``Cartesian`` transform in plain torch (any device; it runs once per mesh, not on the hot path):
    ``pos[edge_index[0]] - pos[edge_index[1]]`` per edge; with ``norm`` divided by ``2 * max|.|`` (or by ``2 * max_value``) and
    shifted by 0.5, i.e. into [0, 1]."""
    cart = pos[edge_index[0]] - pos[edge_index[1]]
    if cart.dim() == 1:
        cart = cart.view(-1, 1)
    if norm and cart.numel() > 0:
        m = cart.abs().max() if max_value is None else max_value
        cart = cart / (2 * m) + 0.5
    return cart


class _SplineConvFn(_Fn):
    """ONE GEMM against the packed weight [weight.permute(0, 2, 1).reshape(K * out, in) ; lin.weight] (rows padded to a multiple of
    4) gives the row buffer [Hf | R], then ONE launch for the B-spline basis + block gather + root + bias (``ops.spline_fwd``).
    Saved: the padded x, the packed weight and the float32 pseudo-coordinates -- not the row buffer and nothing per edge: the
    backward launch evaluates the basis again.  Backward: ONE launch writes [dHf | dOut] into one row buffer
    (``ops.spline_bwd_node``), then ONE wgrad GEMM ([dweight blocks ; dlin]) and ONE dgrad GEMM (dx)."""

    @staticmethod
    def forward(ctx, x, weight, root, bias, attr, graph, kernel_size, is_open, mean):
        K, cin, C = weight.shape
        # buf [N, K * out (+ out) rounded up to 4]: Hf | R | zero padding
        xp, wp, buf, spans = _packed_gemm(x, (weight.permute(0, 2, 1).reshape(K * C, cin), root))
        b = None if bias is None else bias.detach().contiguous()
        a32 = attr.detach().to(torch.float32).contiguous()       # (float64 pseudo-coordinates are rounded once)
        y = ops.spline_fwd(graph, _cols(buf, spans[0]), a32, kernel_size, is_open, root=_cols(buf, spans[1]), bias=b, mean=mean)
        ctx.save_for_backward(xp, wp, a32)
        ctx.graph, ctx.spans, ctx.dims, ctx.spline = graph, spans, (cin, K, C), (kernel_size, is_open, mean)
        return y

    @staticmethod
    def _backward(ctx, dy):
        xp, wp, a32 = ctx.saved_tensors
        graph, spans, (cin, K, C), need = ctx.graph, ctx.spans, ctx.dims, ctx.needs_input_grad
        kernel_size, is_open, mean = ctx.spline
        dy = dy.contiguous().to(torch.float32)
        db = _bias_grad(dy) if need[3] else None
        gb = _grad_rows(dy.shape[0], spans, wp.shape[0], dy.device)
        ops.spline_bwd_node(graph, dy, a32, kernel_size, is_open, C, mean=mean, out=gb, root=spans[1] is not None)   # gb = [dHf | dOut | 0]
        dx, (dwt, droot), _ = _packed_grads(gb, xp, wp, spans, cin, need[1:3], None, need[0])   # [dweight as [K * out, in] ; dlin]
        return dx, None if dwt is None else dwt.reshape(K, C, cin).permute(0, 2, 1), droot, db, None, None, None, None, None


def _spline_sizes(dim, kernel_size, is_open_spline):
    """-> (kernel_size, is_open_spline) as tuples of ``dim`` ints / bools, or ``ValueError``."""
    _int_ge1("SplineConv", "dim", dim)
    if dim > ops.SPLINE_MAX_DIM:
        raise ValueError("SplineConv: dim must be <= %d on the HIP path (2^dim blocks per edge), got %d" % (ops.SPLINE_MAX_DIM, dim))
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    ks = (kernel_size,) * dim if is_int(kernel_size) else kernel_size
    if not isinstance(ks, (tuple, list)) or len(ks) != dim or not all(is_int(k) and k >= 1 for k in ks):
        raise ValueError("SplineConv: kernel_size must be an integer >= 1 or a sequence of dim (%d) of them, got %r" % (dim, kernel_size))
    op = (is_open_spline,) * dim if isinstance(is_open_spline, bool) else is_open_spline
    if not isinstance(op, (tuple, list)) or len(op) != dim or not all(isinstance(o, bool) for o in op):
        raise ValueError("SplineConv: is_open_spline must be a bool or a sequence of dim (%d) bools, got %r" % (dim, is_open_spline))
    return tuple(ks), tuple(op)


class SplineConv(nn.Module):
    """``torch_geometric.nn.SplineConv`` 2.2.0 (Fey et al., SplineCNN, CVPR 2018) with ``degree=1`` on the HIP kernels
    (DESIGN.md 4.15), without the ``torch_spline_conv`` extension: parameters ``weight`` [K, in, out] with K = prod(kernel_size),
    uniform(+-1/sqrt(in K)), ``lin.weight`` [out, in] (the root, no bias of its own, uniform(+-1/sqrt(in)); registered as None with
    ``root_weight=False``) and ``bias`` [out] zeros.  For an edge t: j -> i with pseudo-coordinates ``a_t`` in [0,1]^dim and
    s in [0, 2^dim) with bits s_d: ``v_d = a_t[d] (kernel_size[d] - is_open_spline[d])``, ``f_d = v_d - floor(v_d)``,
    ``b_{t,s} = prod_d (s_d ? f_d : 1 - f_d)``, ``k_{t,s} = sum_d ((floor(v_d) + s_d) mod kernel_size[d]) prod_{d' < d}
    kernel_size[d']``; with ``Hf = x weight`` viewed [N, K, out]:
    ``out[i] = (1 / n_i) sum_{t -> i} sum_s b_{t,s} Hf[j_t, k_{t,s}, :] + lin(x_i) + bias``, n_i the number of edges into i
    (``aggr="mean"``) or 1 (``aggr="add"``).  No self loops are added, an explicit loop is an ordinary edge, duplicate edges each
    count with their own pseudo-coordinates, a node without incoming edges gets ``lin(x_i) + bias``.  Written from the published
    sources from memory -- PyG cannot be installed here, so this could not be checked against it; the pin is the float64
    restatement ``tests/spline_ref.py``.  Differentiable w.r.t. x and every parameter, NOT w.r.t. ``edge_attr`` (refused when it
    requires grad); pseudo-coordinates outside [0, 1] are memory-safe but otherwise unspecified."""

    def __init__(self, in_channels, out_channels: int, dim: int, kernel_size, is_open_spline=True, degree: int = 1,
                 aggr: str = "mean", root_weight: bool = True, bias: bool = True, **kwargs):
        super().__init__()
        _no_tuple_channels("SplineConv", in_channels)
        if degree != 1:
            raise ValueError("SplineConv: only degree=1 is implemented on the HIP path, got %r" % (degree,))
        _check_aggr("SplineConv", aggr, ("mean", "add"), kwargs)
        ks, op = _spline_sizes(dim, kernel_size, is_open_spline)
        self.in_channels, self.out_channels, self.dim, self.degree, self.aggr = in_channels, out_channels, dim, 1, aggr
        self.kernel_size, self.is_open_spline, self.K = ks, op, math.prod(ks)
        if self.K * out_channels >= 1 << 24:
            raise ValueError("SplineConv: prod(kernel_size) * out_channels must be below 2^24 on the HIP path, got %d"
                             % (self.K * out_channels))
        self.weight = nn.Parameter(torch.empty(self.K, in_channels, out_channels))
        if root_weight:
            self.lin = _Lin(in_channels, out_channels)
        else:
            self.register_parameter("lin", None)
        _bias_param(self, bias, out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            a = 1.0 / math.sqrt(self.in_channels * self.K)
            self.weight.uniform_(-a, a)
            if self.lin is not None:
                _reset_linear(self.lin)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x, edge_index, edge_attr=None, size=None) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present); ``edge_attr``: [E, dim]
        pseudo-coordinates in [0, 1], float32 or float64 (rounded to float32 once), not requiring grad."""
        _no_tuple_x("SplineConv", x)
        _not_implemented("SplineConv", size=size)
        _check_x("SplineConv", x, self.in_channels)
        _check_pseudo("SplineConv", x, edge_attr, edge_index.shape[1], self.dim, no_grad=True)
        _need_entries("SplineConv", edge_index)
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=False)
            return _SplineConvFn.apply(x, self.weight, None if self.lin is None else self.lin.weight, self.bias, edge_attr, graph,
                                       self.kernel_size, self.is_open_spline, self.aggr == "mean")

    def extra_repr(self):
        return "%d, %d, dim=%d, kernel_size=%s, aggr=%s" % (self.in_channels, self.out_channels, self.dim, list(self.kernel_size),
                                                            self.aggr)


class _EdgeConvFn(_Fn):
    """ONE GEMM against the packed weight [Wa - Wb ; Wb] (each block's rows padded to a multiple of 4) with the bias [b ; 0] gives
    the row buffer [A | B], then ONE launch gathers the per-column maximum of B and who won (``ops.gather_max``).  Saved: the
    padded x, the packed weight and arg [N, out] -- not the row buffer.  Backward: one launch writes [dA | dB]
    (``ops.gather_max_bwd``), ONE wgrad GEMM gives [dM ; dN] (dWa = dM, dWb = dN - dM), ONE dgrad GEMM gives dx; db = colsum(dA).
    ``want_arg``: whether a backward can follow (grad mode cannot be read inside ``forward``: ``_edge_conv`` passes it in)."""

    @staticmethod
    def forward(ctx, x, weight, bias, graph, want_arg):
        cin = weight.shape[1] // 2
        w = weight.detach()
        xp, wp, buf, spans = _packed_gemm(x, (w[:, :cin] - w[:, cin:], w[:, cin:]), (bias, None), pad_each=True)   # buf [N, 2 cp]: A | padding | B | padding
        want = bool(want_arg) and any(ctx.needs_input_grad[:3])
        y, arg = ops.gather_max(graph, _cols(buf, spans[1]), a=_cols(buf, spans[0]), want_arg=want)
        ctx.save_for_backward(xp, wp, arg)
        ctx.graph, ctx.spans, ctx.cin = graph, spans, cin
        return y

    @staticmethod
    def _backward(ctx, dy):
        xp, wp, arg = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy = dy.contiguous().to(torch.float32)
        g = _grad_rows(dy.shape[0], ctx.spans, wp.shape[0], dy.device)
        ops.gather_max_bwd(ctx.graph, dy, arg, out=g)            # g = [dA | 0 | dB | 0]
        dx, (dm, dn), (db, _) = _packed_grads(g, xp, wp, ctx.spans, ctx.cin, (need[1], need[1]), (need[2], False), need[0])   # [dM ; dN]
        return dx, torch.cat([dm, dn - dm], 1) if need[1] else None, db, None, None


def _edge_conv(x, weight, bias, graph):
    want = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias))
    return _EdgeConvFn.apply(x, weight, bias, graph, want)


_EDGE_NN_MSG = ("%s: on the HIP path %s must be a torch.nn.Linear(%s, out), or a torch.nn.Sequential of one followed by ReLU, "
                "LeakyReLU(negative_slope >= 0) or Identity modules only (elementwise, non-decreasing, 0 -> 0: they commute with the "
                "maximum); got %s")


def _edge_nn(module, who=("EdgeConv", "nn", "2 * in")):
    """-> (the ``Linear`` of an accepted edge function, the elementwise modules behind it), or ``ValueError``.  ``who``: the
    operator, its argument and the ``Linear``'s input width, for the message (EdgeConv: an even width; PPFConv: at least 4)."""
    lin, rest = module, []
    if isinstance(module, nn.Sequential) and len(module) > 0:
        lin, rest = module[0], list(module)[1:]
    if type(lin) is not nn.Linear or lin.weight.dtype != torch.float32:
        raise ValueError(_EDGE_NN_MSG % (who + (module,)))
    if who[0] == "EdgeConv" and lin.in_features % 2:
        raise ValueError("EdgeConv: the Linear takes cat[x_i, x_j - x_i], so its in_features must be even, got %d" % lin.in_features)
    if who[0] == "PPFConv" and lin.in_features < 4:
        raise ValueError("PPFConv: the Linear takes cat[x_j, f_ij] with four point-pair features, so its in_features must be >= 4, "
                         "got %d" % lin.in_features)
    for m in rest:
        if not (type(m) in (nn.ReLU, nn.Identity) or (type(m) is nn.LeakyReLU and m.negative_slope >= 0)):
            raise ValueError(_EDGE_NN_MSG % (who + (module,)))
    return lin, rest


class EdgeConv(nn.Module):
    """``torch_geometric.nn.EdgeConv`` 2.2.0 (Wang et al., Dynamic Graph CNN, 2019) on the HIP kernels,
    ``EdgeConv(nn, aggr="max")``, ``forward(x, edge_index)`` (written from the published source from memory -- PyG cannot be
    installed here, so this could not be checked against it; the pin is the float64 restatement ``tests/edgeconv_ref.py``):

    * ``out[i] = max over the edges j -> i of nn(cat[x_i, x_j - x_i])``, a node without incoming edges gets 0.  No self loops are
      added; an explicit loop is an ordinary edge (it contributes ``nn(cat[x_i, 0])``); a duplicate edge changes nothing.
    * accepted ``nn``: a ``torch.nn.Linear(2 * in, out)`` with or without bias, or a ``torch.nn.Sequential`` whose first module is
      such a ``Linear`` and whose other modules are all ``ReLU``, ``LeakyReLU(negative_slope >= 0)`` or ``Identity``.  Those are
      elementwise, non-decreasing in floating point and map 0 to 0, so ``max_j act(z_j) == act(max_j z_j)`` bit for bit and an
      empty neighbourhood stays 0: they run as ordinary torch modules after the fused core.  (A ``Sigmoid`` fails the second
      condition, a ``BatchNorm`` the first.)  The module is kept as given under ``self.nn``: ``state_dict()`` has PyG's keys
      (``nn.weight``, ``nn.bias`` or ``nn.0.weight`` ...) and ``parameters()`` are the user's own tensors.
    * with ``W = [Wa | Wb]``: ``W [x_i ; x_j - x_i] + b = (Wa - Wb) x_i + b + Wb x_j = A[i] + B[j]``, so
      ``out[i] = A[i] + max_j B[j]``: one GEMM against the packed ``[Wa - Wb ; Wb]`` for the row buffer ``[A | B]``, one launch for
      the per-column maximum and its winner (``ops.gather_max``; the winner is kept only when a gradient is wanted), one launch for
      the backward of the graph part (``ops.gather_max_bwd`` -> ``[dA | dB]``), one wgrad GEMM (``dWa = dM``, ``dWb = dN - dM``)
      and one dgrad GEMM.  No [E, .] tensor exists at any point.  The graph is GATConv's without loops:
      ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=False)``.  Symmetric edge STRUCTURE only.
    * differentiable w.r.t. x and the ``Linear``'s weight and bias; float32, bitwise reproducible.  Deviation: with exact ties
      PyG's winner is unspecified, ours is the smallest source id -- either one is a valid subgradient.
    * refused with ``ValueError`` before any launch: any other ``nn`` (an arbitrary MLP; a ``Linear`` whose ``in_features`` is
      odd), ``aggr != "max"``, a tuple ``x`` (bipartite), bf16 features, an ``x`` that is not [N, in].  Not implemented:
      ``DynamicEdgeConv`` / kNN graphs."""

    def __init__(self, nn, aggr: str = "max", **kwargs):
        super().__init__()
        _check_aggr("EdgeConv", aggr, ("max",), kwargs)
        lin, _ = _edge_nn(nn)
        self.aggr = aggr
        self.in_channels, self.out_channels = lin.in_features // 2, lin.out_features
        self.nn = nn                                             # kept as given: PyG's state_dict keys, the user's own parameters

    def reset_parameters(self):
        for m in self.nn.modules():
            if m is not self.nn and hasattr(m, "reset_parameters"):
                m.reset_parameters()
        if hasattr(self.nn, "reset_parameters"):
            self.nn.reset_parameters()

    def forward(self, x, edge_index) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present)."""
        _no_tuple_x("EdgeConv", x)
        _check_x("EdgeConv", x, self.in_channels)
        _edge_nn(self.nn)                                        # (the module is the user's: it may have been edited since)
        _need_gpu("EdgeConv", x)
        _need_entries("EdgeConv", edge_index)
        return self._core(x, edge_index)

    def _core(self, x, edge_index):
        lin, rest = _edge_nn(self.nn)
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=False)
            y = _edge_conv(x, lin.weight, lin.bias, graph)
        for m in rest:
            y = m(y)
        return y

    def extra_repr(self):
        return "aggr=%s" % self.aggr


def point_pair_features(pos: torch.Tensor, normal: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
    """The four rigid-motion-invariant point-pair features of PyG's ``PointPairFeatures`` transform in plain torch (any device; not
    on the hot path), one row per INPUT edge, in ``PPFConv``'s orientation -- ``edge_index[0] = j`` the source, ``edge_index[1] = i``
    the target: ``d = pos[j] - pos[i]``, ``[|d|, angle(n_i, d), angle(n_j, d), angle(n_i, n_j)]`` with ``angle(a, b) =
    atan2(|a x b|, a . b)`` -> [E, 4].  Usable as ``edge_attr`` of ``GMMConv`` / ``CGConv`` (``dim=4``)."""
    j, i = edge_index[0], edge_index[1]
    d = pos[j] - pos[i]
    ni, nj = normal[i], normal[j]
    angle = lambda a, b: torch.atan2(torch.cross(a, b, dim=1).norm(dim=1), (a * b).sum(1))
    return torch.stack([d.norm(dim=1), angle(ni, d), angle(nj, d), angle(ni, nj)], 1)


class _PPFConvFn(_Fn):
    """With ``W = [Wx | Wp]`` ([out, in + 4]): ONE GEMM gives ``B = x Wx^T + b`` (none when ``x`` is None: the message is
    ``Wp f``), then ONE launch takes the per-column maximum of ``B[j] + F[e] Wp^T`` over the entries and who won
    (``ops.gather_max_attr`` with ``E = Wp^T``).  Saved: the padded x, the packed weight, arg [N, out] and F [entries, 4] -- not the
    row buffer and nothing out-wide per edge.  Backward: ONE launch writes dB and the 8-row partials of dE
    (``ops.gather_max_attr_bwd``), ``dWp = gatv2_datt(parts, 4)^T``, ``db = colsum(dB)`` (every non-empty output lands on exactly
    one winner), ONE wgrad GEMM (dWx) and ONE dgrad GEMM (dx).  ``want_arg``: whether a backward can follow (``_ppf_conv``)."""

    @staticmethod
    def forward(ctx, x, weight, bias, f, graph, want_arg):
        C, cin = weight.shape[0], weight.shape[1] - 4
        w = weight.detach()
        e = w[:, cin:].t().contiguous()                          # [4, out]
        xp = wp = b = spans = None
        if x is not None:
            xp, wp, buf, spans = _packed_gemm(x, (w[:, :cin],), (bias,))   # buf [N, out rounded up to 4]: B | zero padding
            b = _cols(buf, spans[0])
        want = bool(want_arg) and any(ctx.needs_input_grad[:3])
        y, arg = ops.gather_max_attr(graph, b, f, e, want_arg=want)
        ctx.save_for_backward(xp, wp, arg, f)
        ctx.graph, ctx.spans, ctx.dims = graph, spans, (cin, C)
        return y

    @staticmethod
    def _backward(ctx, dy):
        xp, wp, arg, f = ctx.saved_tensors
        need, (cin, C) = ctx.needs_input_grad, ctx.dims
        dy = dy.contiguous().to(torch.float32)
        g = out = None
        if xp is not None:
            g = _grad_rows(dy.shape[0], ctx.spans, wp.shape[0], dy.device)
            out = _cols(g, ctx.spans[0])                         # g = [dB | 0]
        db_rows, parts = ops.gather_max_attr_bwd(ctx.graph, dy, arg, f, out=out, want_parts=need[1])
        dwp = ops.gatv2_datt(parts, 4).t() if need[1] else None  # [out, 4]
        db = _bias_grad(db_rows) if need[2] else None
        dx = dw = None
        if xp is not None:
            dx, (dwx,), _ = _packed_grads(g, xp, wp, ctx.spans, cin, (need[1],), None, need[0])
            dw = torch.cat([dwx, dwp], 1) if need[1] else None
        elif need[1]:
            dw = dwp.contiguous()
        return dx, dw, db, None, None, None


def _ppf_conv(x, weight, bias, f, graph):
    want = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias))
    return _PPFConvFn.apply(x, weight, bias, f, graph, want)


_PPF_NN = ("PPFConv", "local_nn", "in + 4")


def _ppf_geometry(name, t, n):
    if isinstance(t, (tuple, list)):
        raise ValueError("PPFConv: a tuple %s (bipartite graphs) is not implemented on the HIP path" % name)
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3 or (n is not None and t.shape[0] != n):
        raise ValueError("PPFConv: %s must be a tensor of shape [N, 3], got %s" % (name, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError("PPFConv: %s must be float32 or float64, got %s" % (name, t.dtype))
    if t.requires_grad:
        raise ValueError("PPFConv: the gradient with respect to %s is not implemented on the HIP path: pass %s.detach()" % (name, name))


class PPFConv(nn.Module):
    """``torch_geometric.nn.PPFConv`` 2.2.0 (Deng et al., PPFNet, CVPR 2018) on the HIP kernels,
    ``PPFConv(local_nn=None, global_nn=None, add_self_loops=True)``, ``forward(x, pos, normal, edge_index)`` (written from the
    published source from memory -- PyG cannot be installed here, so this could not be checked against it; the pin is the float64
    restatement ``tests/ppf_ref.py``):

    * ``out[i] = global_nn(max over the edges j -> i of local_nn(cat[x_j, f_ij]))`` with the point-pair features
      ``f_ij = [|d|, angle(n_i, d), angle(n_j, d), angle(n_i, n_j)]``, ``d = pos_j - pos_i``, ``angle(a, b) = atan2(|a x b|, a . b)``
      (``point_pair_features``).  ``x`` may be None: the message is ``local_nn(f_ij)``.  With ``add_self_loops`` explicit loops are
      removed and every node gets exactly one loop, whose features are 0; without it an explicit loop is an ordinary edge (its
      features are 0 too), and a node without incoming edges gets ``global_nn(0)``.  A duplicate edge changes nothing.
    * accepted ``local_nn``: a float32 ``torch.nn.Linear(in + 4, out)`` with or without bias, or a ``torch.nn.Sequential`` whose
      first module is one and whose other modules are all ``ReLU``, ``LeakyReLU(negative_slope >= 0)`` or ``Identity`` (EdgeConv's
      rule: they commute with the maximum bit for bit and keep an empty neighbourhood at 0, and run as torch modules after the
      fused core).  It is kept as given under ``self.local_nn``: ``state_dict()`` has PyG's keys (``local_nn.weight`` or
      ``local_nn.0.weight`` ..., ``global_nn.*``) and ``parameters()`` are the user's own tensors.  ``global_nn``: any module or
      None; torch runs it on the result.
    * with ``W = [Wx | Wp]``: ``W [x_j ; f_ij] + b = B[j] + Wp f_ij``, ``B = x Wx^T + b``: one GEMM, one launch for the maximum and
      its winner (``ops.gather_max_attr``), one launch for the graph part of the backward (``ops.gather_max_attr_bwd``), the column
      sum of its 8-row partials for ``dWp``, one wgrad and one dgrad GEMM.  The features of the coalesced entries come from ONE
      launch (``ops.ppf_entries``) cached on the graph by the identity and version of ``pos`` and ``normal``: keep the tensors
      (float64 geometry is rounded to float32 once per call, which defeats that cache).  No [E, out] tensor exists at any point.
      The graph is GATConv's: ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=...)``.  Symmetric edge STRUCTURE only.
    * differentiable w.r.t. x and the ``Linear``'s weight and bias, NOT w.r.t. ``pos`` / ``normal`` (refused when they require
      grad); float32, bitwise reproducible.  Deviation: with exact ties PyG's winner is unspecified, ours is the smallest source id.
    * refused with ``ValueError`` before any launch: ``local_nn=None`` (the raw ``cat[x_j, f_ij]`` maximum), any other
      ``local_nn``, ``aggr != "max"``, tuple ``x`` / ``pos`` / ``normal`` (bipartite), bf16 features, ``pos`` / ``normal`` that are
      not [N, 3] float32 / float64 or require grad, an ``x`` whose width is not ``in``, CPU tensors."""

    def __init__(self, local_nn=None, global_nn=None, add_self_loops: bool = True, **kwargs):
        super().__init__()
        _check_aggr("PPFConv", kwargs.pop("aggr", "max"), ("max",), kwargs)
        if local_nn is None:
            raise ValueError("PPFConv: local_nn=None (the maximum of the raw cat[x_j, f_ij]) is not implemented on the HIP path: "
                             "pass a torch.nn.Linear(in + 4, out)")
        lin, _ = _edge_nn(local_nn, _PPF_NN)
        self.aggr = "max"
        self.in_channels, self.out_channels = lin.in_features - 4, lin.out_features
        self.local_nn = local_nn                                 # kept as given: PyG's state_dict keys, the user's own parameters
        self.global_nn = global_nn
        self.add_self_loops = bool(add_self_loops)

    def reset_parameters(self):
        for top in (self.local_nn, self.global_nn):
            if top is None:
                continue
            for m in top.modules():
                if hasattr(m, "reset_parameters"):
                    m.reset_parameters()

    def forward(self, x, pos, normal, edge_index) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present); ``x``: [N, in] or None;
        ``pos``, ``normal``: [N, 3], float32 or float64 (rounded to float32 once), not requiring grad."""
        _no_tuple_x("PPFConv", x)
        _ppf_geometry("pos", pos, None)
        _ppf_geometry("normal", normal, pos.shape[0])
        lin, _ = _edge_nn(self.local_nn, _PPF_NN)                # (the module is the user's: it may have been edited since)
        if x is None:
            if self.in_channels != 0:
                raise ValueError("PPFConv: x=None needs a local_nn of in_features 4, got %d: expected x of shape [N, %d]"
                                 % (lin.in_features, self.in_channels))
        else:
            _check_x("PPFConv", x, self.in_channels)
            if self.in_channels == 0 or x.shape[0] != pos.shape[0]:
                raise ValueError("PPFConv: expected x of shape [%d, %d] (None for a local_nn of in_features 4), got %s"
                                 % (pos.shape[0], self.in_channels, tuple(x.shape)))
        for t in (x, pos, normal):
            if t is not None:
                _need_gpu("PPFConv", t, exc=ValueError)
        _need_entries("PPFConv", edge_index, loops=self.add_self_loops)
        return self._core(x, pos, normal, edge_index)

    def _core(self, x, pos, normal, edge_index):
        lin, rest = _edge_nn(self.local_nn, _PPF_NN)
        n = pos.shape[0]
        with ops.on_device(pos):
            graph = ops.graph_for(edge_index, n, norm="gat", add_self_loops=self.add_self_loops)
            with torch.no_grad():
                f = ops.ppf_entries(graph, pos if pos.dtype == torch.float32 else pos.to(torch.float32),
                                    normal if normal.dtype == torch.float32 else normal.to(torch.float32))
            if x is not None:
                y = _ppf_conv(x, lin.weight, lin.bias, f, graph)
            else:
                y = _ppf_conv(None, lin.weight, None, f, graph)
                if lin.bias is not None:                         # after the launch; an empty neighbourhood stays 0
                    if self.add_self_loops:
                        y = y + lin.bias
                    else:
                        has = torch.zeros(n, dtype=torch.bool, device=y.device)
                        has[edge_index[1]] = True
                        y = torch.where(has.unsqueeze(1), y + lin.bias, y)
        for m in rest:
            y = m(y)
        return y if self.global_nn is None else self.global_nn(y)

    def extra_repr(self):
        return "add_self_loops=%s" % self.add_self_loops


_SAGE_AGGRS = ("mean", "add", "sum", "max", "min")


def _sage_aggrs(aggr, kwargs):
    """-> the aggregators of a SAGEConv as a tuple of names out of mean / add / max / min (``"sum"`` is ``"add"``), in the
    order given, or ``ValueError``: a name outside that list (``"lstm"``, ``"std"``, ``"var"`` ...), an empty list, a repeat, or
    mean and add together."""
    given = list(aggr) if isinstance(aggr, (list, tuple)) else [aggr]
    if not given:
        raise ValueError("SAGEConv: an empty list of aggregators")
    for a in given:
        _check_aggr("SAGEConv", a, _SAGE_AGGRS, kwargs)          # (and nothing may be left in the constructor's kwargs)
    names = tuple("add" if a == "sum" else a for a in given)
    if len(set(names)) != len(names):
        raise ValueError("SAGEConv: an aggregator is listed twice in %r" % (list(aggr),))
    if "mean" in names and "add" in names:
        raise ValueError("SAGEConv: mean and add together are not implemented on the HIP path (one sum per launch), got %r" % (list(aggr),))
    return names


class _SAGEConvFn(_Fn):
    """Both directions of the GCNConv trade, every one with ONE graph launch per direction (``ops.gather_stats`` /
    ``ops.gather_stats_bwd``):

    * aggregate-first (the only form for max, min and lists): one launch writes ``[A_1 | ... | A_k | X]`` into one row buffer
      (the X block only with a root weight), ONE GEMM against the column-packed ``[lin_l.weight | lin_r.weight]`` with the bias.
      Saved: the row buffer, the packed weight, the args of max / min and 1 / deg of mean.  Backward: ONE wgrad GEMM
      (``[dlin_l | dlin_r]``), ONE dgrad GEMM (``[dA_1 | ... | dA_k | dX0]``) and one launch that scatters every block back to dx.
    * transform-first (a single mean / add whose padded ``out`` is narrower than the padded ``in``): ONE GEMM against the
      row-packed ``[lin_l.weight ; lin_r.weight]`` gives ``[L | R]``, one launch computes ``mean(L) + R + bias``.  Saved: the padded
      x, the packed weight and 1 / deg.  Backward: one launch writes ``[dL | dR]``, then ONE wgrad and ONE dgrad GEMM.

    ``want_arg``: whether a backward can follow (grad mode cannot be read inside ``forward``: ``_sage_conv`` passes it in)."""

    @staticmethod
    def forward(ctx, x, wl, bl, wr, graph, aggrs, want_arg):
        n, cin, cout, k = x.shape[0], x.shape[1], wl.shape[0], len(aggrs)
        b = None if bl is None else bl.detach().contiguous()
        pad4 = lambda c: (c + 3) // 4 * 4
        ctx.graph, ctx.aggrs, ctx.dims, ctx.has_root = graph, aggrs, (cin, cout), wr is not None
        ctx.first = k == 1 and aggrs[0] in ("mean", "add") and pad4(cout) < pad4(cin)
        if ctx.first:
            xp, wp, buf, spans = _packed_gemm(x, (wl, wr))       # buf [N, (1 or 2) out rounded up to 4]: L | R | zero padding
            (y,), _, invdeg = ops.gather_stats(graph, _cols(buf, spans[0]), want=aggrs, root=_cols(buf, spans[1]), bias=b)
            ctx.save_for_backward(xp, wp, invdeg)
            ctx.spans = spans
            return y
        want = bool(want_arg) and any(ctx.needs_input_grad[:4])
        used = (k + (wr is not None)) * cin
        buf = _grad_rows(n, [(0, used)], pad4(used), x.device)   # [A_1 | ... | A_k | X | zero padding]
        _, args, invdeg = ops.gather_stats(graph, x.detach().to(torch.float32).contiguous(), want=aggrs, copy_x=wr is not None,
                                           want_arg=want, out=buf)
        wp = _pad_cols(wl.detach() if wr is None else torch.cat([wl.detach(), wr.detach()], 1))
        y = ops.gemm_nt(buf, wp, bias=b)
        ctx.save_for_backward(buf, wp, invdeg, *[a for a in args if a is not None])
        return y

    @staticmethod
    def _backward(ctx, dy):
        graph, aggrs, (cin, cout), need = ctx.graph, ctx.aggrs, ctx.dims, ctx.needs_input_grad
        dy = dy.contiguous().to(torch.float32)
        db = _bias_grad(dy) if need[2] else None
        if ctx.first:
            xp, wp, invdeg = ctx.saved_tensors
            gb = _grad_rows(dy.shape[0], ctx.spans, wp.shape[0], dy.device)
            ops.gather_stats_bwd(graph, ds=dy, invdeg=invdeg, root=ctx.has_root, out=gb)         # gb = [dL | dR | 0]
            dx, (dwl, dwr), _ = _packed_grads(gb, xp, wp, ctx.spans, cin, (need[1], need[3]), None, need[0])
            return dx, dwl, db, dwr, None, None, None
        buf, wp, invdeg, *args = ctx.saved_tensors
        k = len(aggrs)
        dyp = _pad_cols(dy)
        dwl = dwr = dx = None
        if need[1] or (ctx.has_root and need[3]):
            dwp = ops.gemm_tn(dyp, buf)                          # [dlin_l | dlin_r]
            dwl, dwr = dwp[:cout, :k * cin], (dwp[:cout, k * cin:(k + 1) * cin] if ctx.has_root else None)
        if need[0]:
            g = ops.gemm_nn(dyp, _pad_rows_like(wp, dyp, cout))  # [dA_1 | ... | dA_k | dX0 | .]
            args, op = list(args), {}
            for i, a in enumerate(aggrs):
                blk = g[:, i * cin:(i + 1) * cin]
                if a in ("max", "min"):
                    op["d" + ("mx" if a == "max" else "mn")], op["arg" + ("mx" if a == "max" else "mn")] = blk, args.pop(0)
                else:
                    op["ds"], op["invdeg"] = blk, invdeg
            dx, _ = ops.gather_stats_bwd(graph, dx0=g[:, k * cin:(k + 1) * cin] if ctx.has_root else None, **op)
        return dx, dwl, db, dwr, None, None, None


def _sage_conv(x, wl, bl, wr, graph, aggrs):
    want = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, wl, bl, wr))
    return _SAGEConvFn.apply(x, wl, bl, wr, graph, aggrs, want)


class SAGEConv(nn.Module):
    """``torch_geometric.nn.SAGEConv`` 2.2.0 (Hamilton et al., GraphSAGE, NeurIPS 2017) on the HIP kernels,
    ``SAGEConv(in_channels, out_channels, aggr="mean", normalize=False, root_weight=True, project=False, bias=True)``,
    ``forward(x, edge_index, size=None)`` (restated from the published source from memory -- PyG cannot be installed here, so this
    could not be checked against it; the pin is the float64 restatement ``tests/sage_ref.py``):

    * ``out[i] = lin_l(cat_k aggr_k({x_j : j -> i})) + lin_r(x_i)``, with ``normalize`` followed by
      ``F.normalize(out, p=2, dim=-1)`` (torch elementwise work on [N, out], not fused).  Parameters: ``lin_l.weight``
      [out, k * in] for k aggregators and ``lin_l.bias`` [out] (only with ``bias=True``), ``lin_r.weight`` [out, in] without a bias
      (the attribute is absent with ``root_weight=False``), all uniform(+-1/sqrt(fan-in)).
    * ``aggr``: ``"mean"``, ``"add"`` / ``"sum"``, ``"max"``, ``"min"``, or a list of those, concatenated in list order (PyG's
      ``MultiAggregation`` in ``cat`` mode).  No self loops are added, an explicit loop is an ordinary edge, duplicate edges each
      count in mean / add and cannot change max / min, a node without incoming edges aggregates to 0.
    * the launches: ``_SAGEConvFn`` -- ONE gather launch per direction whatever the number of aggregators: every neighbour row is
      read once and feeds all of them (``ops.gather_stats``).  No [E, .] tensor and no ``index_add_`` / ``scatter`` exist at any
      point.  The graph is GATConv's without loops: ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=False)``.  Symmetric
      edge STRUCTURE only.
    * differentiable w.r.t. x and every parameter; float32, bitwise reproducible.  Deviation: with exact ties PyG's max / min
      winner is unspecified, ours is the smallest source id -- either one is a valid subgradient.
    * refused with ``ValueError`` before any launch: ``project=True``, any other aggregator (``"lstm"``, ``"std"``, ``"var"`` ...), a
      list with a repeat or with both mean and add, tuple ``in_channels`` or a tuple ``x`` (bipartite), ``size``, bf16 features, a
      CPU ``x``, an ``x`` that is not [N, in]."""

    def __init__(self, in_channels, out_channels: int, aggr="mean", normalize: bool = False, root_weight: bool = True,
                 project: bool = False, bias: bool = True, **kwargs):
        super().__init__()
        _no_tuple_channels("SAGEConv", in_channels)
        if project:
            raise ValueError("SAGEConv: project=True is not implemented on the HIP path")
        self._aggrs = _sage_aggrs(aggr, kwargs)
        self.in_channels, self.out_channels, self.aggr = in_channels, out_channels, aggr
        self.normalize, self.root_weight, self.project = bool(normalize), bool(root_weight), False
        self.lin_l = _LinB(len(self._aggrs) * in_channels, out_channels, bias=bias)
        if root_weight:
            self.lin_r = _Lin(in_channels, out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            _reset_linear(self.lin_l)
            if self.root_weight:
                _reset_linear(self.lin_r)

    def forward(self, x, edge_index, size=None) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present)."""
        _no_tuple_x("SAGEConv", x)
        _not_implemented("SAGEConv", size=size)
        _check_x("SAGEConv", x, self.in_channels)
        _need_gpu("SAGEConv", x, exc=ValueError)
        _need_entries("SAGEConv", edge_index)
        return self._core(x, edge_index)

    def _core(self, x, edge_index):
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=False)
            y = _sage_conv(x, self.lin_l.weight, self.lin_l.bias, self.lin_r.weight if self.root_weight else None, graph, self._aggrs)
        return torch.nn.functional.normalize(y, p=2.0, dim=-1) if self.normalize else y

    def extra_repr(self):
        return "%d, %d, aggr=%s" % (self.in_channels, self.out_channels, self.aggr)


_PNA_AGGRS = ("mean", "sum", "max", "min", "std", "var")
_PNA_SCALERS = ("identity", "amplification", "attenuation", "linear", "inverse_linear")


def _pna_names(what, given, allowed, pairs=()):
    """-> ``given`` (a list or tuple of names) as a tuple, or ``ValueError``: not a list, empty, a name outside ``allowed``, a
    repeat, or both names of one of ``pairs``."""
    if not isinstance(given, (list, tuple)) or not given:
        raise ValueError("PNAConv: %s must be a non-empty list of names out of %r, got %r" % (what, allowed, given))
    names = tuple(given)
    for a in names:
        if not isinstance(a, str) or a not in allowed:
            raise ValueError("PNAConv: only the %s %r are implemented on the HIP path, got %r" % (what, allowed, a))
    if len(set(names)) != len(names):
        raise ValueError("PNAConv: one of the %s is listed twice in %r" % (what, list(given)))
    for a, b in pairs:
        if a in names and b in names:
            raise ValueError("PNAConv: %s and %s together are not implemented on the HIP path (one %s per launch), got %r"
                             % (a, b, "sum" if a == "mean" else "second moment", list(given)))
    return names


def degree_histogram(edge_index: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """The in-degree histogram ``PNAConv``'s ``deg`` expects (as in PyG's own PNA example): int64 [max in-degree + 1], entry k =
    the number of nodes with k incoming edges (duplicate edges and explicit loops count)."""
    d = torch.bincount(edge_index[1], minlength=int(num_nodes))
    return torch.bincount(d)


def _pna_scaler_table(graph, edge_index, n, scalers, delta, dtype):
    """[N, len(scalers)] in the parameters' dtype: every scaler's per-row factor, with ``d_i = max(in-degree_i, 1)``.  It depends
    on the graph alone, so it is computed once per graph handle (and per scaler set) and kept on it."""
    tables = graph.__dict__.setdefault("_pna_tables", {})
    key = (scalers, delta, str(edge_index.device), dtype)
    if key not in tables:
        d = torch.bincount(edge_index[1], minlength=n).clamp_(min=1).to(torch.float64)
        logd = torch.log(d + 1.0)
        col = {"identity": torch.ones_like(d), "amplification": logd / delta[1], "attenuation": delta[1] / logd,
               "linear": d / delta[0], "inverse_linear": delta[0] / d}
        tables[key] = torch.stack([col[s] for s in scalers], 1).to(dtype).contiguous()
    return tables[key]


def _pna_aggr_bwd(graph, aggrs, grads, args, invdeg, mu, values, b, out_a, out_b):
    """The chain rule of the aggregators of ``A[i] + aggr_j B[j]``.  ``grads``: the gradient reaching every aggregate block, [N, C]
    each, parallel to ``aggrs``; ``args``: the saved winners of the max / min blocks, in order; ``values``: the forward's blocks
    ([N, T, F] views; read for std); ``b``: B.  Writes dA into ``out_a`` and dB into ``out_b`` ([N, C] column blocks of one row
    buffer): torch elementwise work on [N, C] forms dA and the two streams dS / dQ, ONE ``ops.gather_moments_bwd`` launch gathers."""
    has = (invdeg > 0).view(-1, 1)
    zero = torch.zeros((), dtype=out_a.dtype, device=out_a.device)
    weighted = any(a in ("mean", "std", "var") for a in aggrs)   # the dS stream's coefficient: a w_i (else a: the sum alone)
    args, op, da, ds = list(args), {}, None, None
    for a, d, v in zip(aggrs, grads, values):
        if a in ("max", "min"):
            key = "mx" if a == "max" else "mn"
            op["d" + key], op["arg" + key] = d, args.pop(0)
            da = d if da is None else da + d
        elif a == "mean":
            ds = d if ds is None else ds + d
            da = d if da is None else da + d
        elif a == "sum":
            # deg_i x dSum is dA's share; next to a mean / std / var it is also the sum's share of the a w_i stream
            dd = d * torch.where(has, torch.round(1.0 / invdeg.view(-1, 1)), zero)
            ds = (dd if weighted else d) if ds is None else ds + dd
            da = dd if da is None else da + dd
        else:
            v = v.reshape(d.shape)
            g = torch.where(v > 0, d / v, zero) if a == "std" else 2.0 * d
            op["dq"], op["b"] = g, b
            ds = -(g * mu) if ds is None else ds - g * mu
    out_a.copy_(zero if da is None else da * has)
    ops.gather_moments_bwd(graph, ds=ds, invdeg=invdeg if weighted else None, out=out_b, **op)


class _PNAConvFn(_Fn):
    """``PNAConv``'s route (see the class).  Inputs: x, the graph, the [N, S] scaler table, the aggregators, ``want_arg``, then the
    parameters ``pre_w[T], pre_b[T], post_w[T], post_b[T], lin_w, lin_b``.  Saved: the padded x and centred x, the packed pre weight, the
    ``[A | B]`` row buffer (the backward multiplies by the row's own B), the tower-major aggregate buffer, the padded ``H = cat_t
    out_t``, the args, ``mu`` and ``invdeg``.  The chain rule of the aggregators is ``_pna_aggr_bwd``."""

    @staticmethod
    def forward(ctx, x, graph, sc, aggrs, want_arg, *params):
        T = (len(params) - 2) // 4
        pre_w, pre_b, post_w, post_b = (params[k * T:(k + 1) * T] for k in range(4))
        lin_w, lin_b = params[4 * T:]
        n, F, fo, A, S = x.shape[0], x.shape[1], post_w[0].shape[0], len(aggrs), sc.shape[1]
        dev, dt = x.device, lin_w.dtype                         # (float32; the kernels refuse anything else)
        wa = torch.cat([w.detach()[:, :F] for w in pre_w], 0)
        wb = torch.cat([w.detach()[:, F:] for w in pre_w], 0)
        # the message is invariant to a per-column constant c: x_i Wa + x_j Wb + b = (x_i - c) Wa + (x_j - c) Wb + (b + (Wa + Wb) c).
        # With c = x[0] B is of the size of the features' SPREAD, so a column far from 0 costs std / var and their gradient nothing
        xd = x.detach().to(dt)
        c = xd[:1]
        xp = _pad_cols(xd)
        bc = torch.cat([b.detach() for b in pre_b]) + ((wa + wb) * c).sum(1)
        xcp, wp, buf, spans = _packed_gemm(xd - c, (wa, wb), (bc, None), pad_each=True, dtype=dt)   # [A | B]
        want = bool(want_arg) and (ctx.needs_input_grad[0] or any(ctx.needs_input_grad[5:]))
        agg = torch.empty((n, T * A * F), dtype=dt, device=dev)                  # [tower][aggregator][F]
        _, args, invdeg, mu = ops.gather_moments(graph, _cols(buf, spans[1]), want=aggrs, root=_cols(buf, spans[0]),
                                                 tower_width=F, want_arg=want, out=agg)
        # the x columns of every tower's post weight in ONE GEMM, with the post biases
        wx = _packed_rows([torch.cat([w.detach()[:, :F] for w in post_w], 0)], xp.shape[1], dev, dtype=dt)
        bx = torch.zeros(wx.shape[0], dtype=dt, device=dev)
        bx[:T * fo] = torch.cat([b.detach() for b in post_b])
        hx = ops.gemm_nt(xp, wx, bias=bx)
        hp = torch.zeros((n, (T * fo + 3) // 4 * 4), dtype=dt, device=dev)       # H = cat_t out_t, zero padding
        wz = []
        for t in range(T):
            # tower t's scaler-packed post weight [S * F_out, A * F]: row s * F_out + o = post_w[t][o, F + s * A * F : F + (s + 1) * A * F]
            w = post_w[t].detach()[:, F:].reshape(fo, S, A * F).transpose(0, 1).reshape(S * fo, A * F)
            wz.append(_packed_rows([_pad_cols(w)], (A * F + 3) // 4 * 4, dev, dtype=dt))
            z = ops.gemm_nt(_pad_cols(agg[:, t * A * F:(t + 1) * A * F]), wz[t])            # Z_t [N, S * F_out (+ padding)]
            hp[:, t * fo:(t + 1) * fo] = hx[:, t * fo:(t + 1) * fo] + (z[:, :S * fo].reshape(n, S, fo) * sc.unsqueeze(-1)).sum(1)
        wl = _pad_cols(_packed_rows([lin_w.detach()], lin_w.shape[1], dev, dtype=dt))
        bl = torch.zeros(wl.shape[0], dtype=dt, device=dev)
        bl[:T * fo] = lin_b.detach()
        y = ops.gemm_nt(hp, wl, bias=bl)[:, :T * fo]
        ctx.save_for_backward(xp, xcp, c, wp, buf, agg, hp, sc, wx, wl, invdeg, mu, *wz, *[a for a in args if a is not None])
        ctx.graph, ctx.aggrs, ctx.spans, ctx.dims = graph, aggrs, spans, (T, F, fo)
        return y.contiguous()

    @staticmethod
    def _backward(ctx, dy):
        xp, xcp, c, wp, buf, agg, hp, sc, wx, wl, invdeg, mu, *rest = ctx.saved_tensors
        (T, F, fo), aggrs, graph, spans = ctx.dims, ctx.aggrs, ctx.graph, ctx.spans
        wz, args = rest[:T], list(rest[T:])
        n, A, S, C, dev, dt = dy.shape[0], len(aggrs), sc.shape[1], T * F, dy.device, hp.dtype
        dyp = _pad_cols(dy.contiguous().to(dt))
        # lin
        dlin_b = _bias_grad(dyp)[:T * fo]
        dlin_w = ops.gemm_tn(dyp, hp)[:T * fo, :T * fo]
        dh = ops.gemm_nn(dyp, wl)                               # [N, out (+ padding)], padding columns 0
        # the x columns of the post weights
        dpost_b = _bias_grad(dh)[:T * fo]
        dwx = ops.gemm_tn(dh, xp)[:T * fo, :F]
        dx = ops.gemm_nn(dh, wx)[:, :F]
        # per tower: the scaler-weighted gradient of Z_t, its wgrad and dgrad on the tower's columns of the aggregate buffer
        dblk = torch.empty((n, A * C), dtype=dt, device=dev)                     # [aggregator][tower][F]: plain [N, C] blocks
        dpost_w = []
        for t in range(T):
            dz = torch.zeros((n, wz[t].shape[0]), dtype=dt, device=dev)
            dz[:, :S * fo] = (dh[:, t * fo:(t + 1) * fo].unsqueeze(1) * sc.unsqueeze(-1)).reshape(n, S * fo)
            aggt = _pad_cols(agg[:, t * A * F:(t + 1) * A * F])
            dwz = ops.gemm_tn(dz, aggt)[:S * fo, :A * F]                                      # [S * F_out, A * F]
            dpost_w.append(torch.cat([dwx[t * fo:(t + 1) * fo], dwz.reshape(S, fo, A * F).transpose(0, 1).reshape(fo, S * A * F)], 1))
            dagg = ops.gemm_nn(dz, wz[t])                                                    # [N, A * F (+ padding)]
            dblk.view(n, A, T, F)[:, :, t] = dagg[:, :A * F].reshape(n, A, F)
        gb = _grad_rows(n, spans, wp.shape[0], dev, dt)
        _pna_aggr_bwd(graph, aggrs, [dblk[:, k * C:(k + 1) * C] for k in range(A)], args, invdeg, mu,
                      [agg.view(n, T, A, F)[:, :, k] for k in range(A)], _cols(buf, spans[1]), _cols(gb, spans[0]), _cols(gb, spans[1]))
        # x was centred: dW = g^T (x - c) + colsum(g) c^T.  colsum(dB) = colsum(dA) (every aggregator hands on all it receives, and
        # std / var nothing), and dA's is the well-conditioned one: the column sum of the std / var part of dB is an exact 0
        dxp, (dwa, dwb), (dba, _) = _packed_grads(gb, xcp, wp, spans, F, (True, True), (True, False), True)
        dx = dx + dxp
        shift = dba.view(-1, 1) * c
        dwa, dwb = dwa + shift, dwb + shift
        dpre_w = [torch.cat([dwa[t * F:(t + 1) * F], dwb[t * F:(t + 1) * F]], 1) for t in range(T)]
        dpre_b = [dba[t * F:(t + 1) * F] for t in range(T)]
        dpost_b = [dpost_b[t * fo:(t + 1) * fo] for t in range(T)]
        return (dx, None, None, None, None, *dpre_w, *dpre_b, *dpost_w, *dpost_b, dlin_w, dlin_b)


class _Seq1(nn.Sequential):
    """A ``Sequential`` of ONE ``Linear`` with a bias: PyG's single-layer pre / post MLP, whose parameters are ``0.weight`` / ``0.bias``."""

    def __init__(self, in_channels, out_channels):
        super().__init__(_LinB(in_channels, out_channels))


class PNAConv(nn.Module):
    """``torch_geometric.nn.PNAConv`` 2.2.0 (Corso et al., Principal Neighbourhood Aggregation, NeurIPS 2020) on the HIP kernels
    (DESIGN.md 4.17), ``PNAConv(in_channels, out_channels, aggregators, scalers, deg, edge_dim=None, towers=1, pre_layers=1,
    post_layers=1, divide_input=False, act="relu", act_kwargs=None)``, ``forward(x, edge_index, edge_attr=None)`` (restated from
    the published 2.2.0 source, not checked against an installed PyG; the pin is the float64 restatement ``tests/pna_ref.py``):

    * per tower t: the message ``h_t(j -> i) = pre_nns[t](cat[x_i, x_j])``, aggregated over each target's incoming edges with every
      aggregator (``mean``, ``sum``, ``max``, ``min``, ``std``, ``var``), multiplied by every scaler (``identity``,
      ``amplification``, ``attenuation``, ``linear``, ``inverse_linear``; concatenated scaler-major, then aggregator, then F),
      ``out_t = post_nns[t](cat[x_i, that])``, ``y = lin(cat_t out_t)``.  Parameters: ``pre_nns.{t}.0.weight`` [F, 2 F] and
      ``.bias``, ``post_nns.{t}.0.weight`` [F_out, (len(aggregators) * len(scalers) + 1) * F] and ``.bias``, ``lin.weight``
      [out, out] and ``.bias``, with F = in_channels and F_out = out_channels // towers, all uniform(+-1/sqrt(fan-in)).
      ``act`` / ``act_kwargs`` are accepted and unused: a single-layer MLP has no activation.
    * scalers: with ``d_i = max(in-degree_i, 1)`` and, from the histogram ``deg`` (``degree_histogram``), ``delta_lin = sum k deg[k]
      / sum deg`` and ``delta_log = sum log(k + 1) deg[k] / sum deg``: amplification ``log(d + 1) / delta_log``, attenuation
      ``delta_log / log(d + 1)``, linear ``d / delta_lin``, inverse_linear ``delta_lin / d``.
    * std: ``sqrt(max(var, 1e-5))``, then 0 where that is ``<= sqrt(1e-5)``, gradient 0 there (``StdAggregation``); var:
      ``mean(h^2) - mean(h)^2``.  Here both come from sums shifted by the row's first entry (exact where PyG's form cancels).
    * the route (``_PNAConvFn``): with ``W_t = [Wa_t | Wb_t]`` the message is ``A_t[i] + B_t[j]``, every aggregator of it over j is
      ``A_t[i] + aggr_j B_t[j]`` (``deg_i A_t[i] +`` for the sum) and std / var do not see ``A`` at all.  ONE GEMM of x against the
      packed ``[Wa_1; ..; Wa_T; Wb_1; ..; Wb_T]`` gives ``[A | B]``; ONE ``ops.gather_moments`` launch over B with root A writes
      every aggregator of every tower into one tower-major row buffer; the scalers are per-row scalars, so they are applied AFTER
      the post GEMM: per tower one GEMM of its ``[N, len(aggregators) * F]`` columns against the scaler-packed post weight gives
      ``Z_t`` [N, len(scalers) * F_out], one GEMM ``x @ W_x`` covers the x columns of all towers, ``out_t = x W_x + b + sum_s
      s_s(i) Z_{t,s}[i]`` is elementwise work, then the ``lin`` GEMM.  The [N, len(scalers)] scaler table is computed once per
      graph.  Backward: the mirrored wgrad / dgrad GEMMs, the chain rule of std / var as torch elementwise work on [N, .], and ONE
      ``ops.gather_moments_bwd`` launch -> ``[dA | dB]`` for one wgrad and one dgrad GEMM against the packed pre weights.  No
      [E, .] tensor (PyG holds [E, towers, F]) and no ``index_add_`` / ``scatter`` exist at any point.  The graph is GATConv's
      without loops: ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=False)``.  Symmetric edge STRUCTURE only.
    * duplicate edges count in the degree, mean, sum, std and var and cannot change max / min; a node without incoming edges gets
      ``post(cat[x_i, 0])``.  Differentiable w.r.t. x and every parameter; float32, bitwise reproducible; a forward without a
      gradient stores no args.  Deviation: with exact ties PyG's max / min winner is unspecified, ours is the smallest source id.
    * refused with ``ValueError`` before any launch: ``edge_dim`` / ``edge_attr``, ``pre_layers > 1`` (a per-edge MLP),
      ``post_layers > 1``, ``divide_input=True``, ``out_channels % towers != 0``, an aggregator or scaler outside the lists above, a
      repeat, mean and sum together, std and var together, an empty list, tuple inputs, bf16 features, a CPU ``x``, an ``x`` that
      is not [N, in]."""

    def __init__(self, in_channels, out_channels: int, aggregators, scalers, deg, edge_dim=None, towers: int = 1, pre_layers: int = 1,
                 post_layers: int = 1, divide_input: bool = False, act="relu", act_kwargs=None, **kwargs):
        super().__init__()
        _no_tuple_channels("PNAConv", in_channels)
        _not_implemented("PNAConv", edge_dim=edge_dim)
        _int_ge1("PNAConv", "towers", towers)
        if pre_layers != 1:
            raise ValueError("PNAConv: pre_layers > 1 (a per-edge MLP) is not implemented on the HIP path, got %r" % (pre_layers,))
        if post_layers != 1:
            raise ValueError("PNAConv: post_layers > 1 is not implemented on the HIP path, got %r" % (post_layers,))
        if divide_input:
            raise ValueError("PNAConv: divide_input=True is not implemented on the HIP path")
        if out_channels % towers != 0:
            raise ValueError("PNAConv: out_channels (%d) must be a multiple of towers (%d)" % (out_channels, towers))
        self._aggrs = _pna_names("aggregators", aggregators, _PNA_AGGRS, (("mean", "sum"), ("std", "var")))
        self._scalers = _pna_names("scalers", scalers, _PNA_SCALERS)
        if kwargs:
            raise TypeError("PNAConv: unexpected keyword arguments %s" % sorted(kwargs))
        if not isinstance(deg, torch.Tensor) or deg.dim() != 1 or deg.numel() == 0 or float(deg.sum()) <= 0:
            raise ValueError("PNAConv: deg must be the in-degree histogram, a 1-D tensor with a positive sum (degree_histogram)")
        h = deg.detach().to("cpu", torch.float64)
        k = torch.arange(h.numel(), dtype=torch.float64)
        self.avg_deg = {"lin": float((k * h).sum() / h.sum()), "log": float((torch.log(k + 1) * h).sum() / h.sum())}
        self.in_channels, self.out_channels, self.towers = in_channels, out_channels, towers
        self.aggregators, self.scalers, self.edge_dim, self.divide_input = list(aggregators), list(scalers), None, False
        self.F_in, self.F_out = in_channels, out_channels // towers
        self.pre_nns = nn.ModuleList([_Seq1(2 * self.F_in, self.F_in) for _ in range(towers)])
        self.post_nns = nn.ModuleList([_Seq1((len(self._aggrs) * len(self._scalers) + 1) * self.F_in, self.F_out) for _ in range(towers)])
        self.lin = _LinB(out_channels, out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            for seq in list(self.pre_nns) + list(self.post_nns):
                _reset_linear(seq[0])
            _reset_linear(self.lin)

    def forward(self, x, edge_index, edge_attr=None) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present)."""
        _no_tuple_x("PNAConv", x)
        _not_implemented("PNAConv", edge_attr=edge_attr)
        _check_x("PNAConv", x, self.in_channels)
        _need_gpu("PNAConv", x, exc=ValueError)
        _need_entries("PNAConv", edge_index)
        return self._core(x, edge_index)

    def _core(self, x, edge_index):
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=False)
            sc = _pna_scaler_table(graph, edge_index, x.shape[0], self._scalers, (self.avg_deg["lin"], self.avg_deg["log"]), self.lin.weight.dtype)
            params = ([s[0].weight for s in self.pre_nns] + [s[0].bias for s in self.pre_nns] + [s[0].weight for s in self.post_nns]
                      + [s[0].bias for s in self.post_nns] + [self.lin.weight, self.lin.bias])
            want = torch.is_grad_enabled() and any(t.requires_grad for t in [x] + params)
            return _PNAConvFn.apply(x, graph, sc, self._aggrs, want, *params)

    def extra_repr(self):
        return "%d, %d, towers=%d, aggregators=%s, scalers=%s" % (self.in_channels, self.out_channels, self.towers, self.aggregators,
                                                                self.scalers)


class _LinearFn(_Fn):
    """``x @ w^T + b`` on the project's GEMMs (GENConv's MLP): ``ops.gemm_nt`` forward, ``ops.gemm_tn`` (wgrad) and ``ops.gemm_nn``
    (dgrad) backward, the operands zero-padded to multiples of 4 columns / rows.  ``strict``: the three run with float32-input
    MFMA (GEMM mode 0) instead of the split-precision default, whose f32-class error has a part that is the same in every row."""

    @staticmethod
    def forward(ctx, x, w, b, strict=False):
        ctx.strict = bool(strict)
        with (ops.gemm_mode(0) if strict else contextlib.nullcontext()):
            return _LinearFn._forward(ctx, x, w, b)

    @staticmethod
    def _forward(ctx, x, w, b):
        dt, cin, cout = x.dtype, w.shape[1], w.shape[0]
        xp = _pad_cols(x.detach())
        wp = _packed_rows([w.detach()], xp.shape[1], x.device, dtype=dt)
        lb = None
        if b is not None:
            lb = torch.zeros(wp.shape[0], dtype=dt, device=x.device)
            lb[:cout] = b.detach()
        ctx.save_for_backward(xp, wp)
        ctx.dims = (cin, cout)
        return ops.gemm_nt(xp, wp, bias=lb)[:, :cout]

    @staticmethod
    def _backward(ctx, dy):
        xp, wp = ctx.saved_tensors
        (cin, cout), need = ctx.dims, ctx.needs_input_grad
        dyp = torch.zeros((dy.shape[0], wp.shape[0]), dtype=xp.dtype, device=dy.device)
        dyp[:, :cout] = dy
        with (ops.gemm_mode(0) if ctx.strict else contextlib.nullcontext()):
            dw = ops.gemm_tn(dyp, xp)[:cout, :cin] if need[1] else None
            dx = ops.gemm_nn(dyp, wp)[:, :cin] if need[0] else None
        db = _bias_grad(dyp)[:cout] if need[2] else None
        return dx, dw, db, None


class _BatchNorm1d64(nn.BatchNorm1d):
    """``nn.BatchNorm1d`` (same parameters, buffers and ``state_dict``) that normalises float32 input in float64 and rounds the
    result once, as the project's own BatchNorm kernels take their column statistics in float64.  In float32 the column means of
    the backward carry an error that is the SAME for every row; a gradient that sums over all rows against weights of one sign
    (``msg_norm.scale``'s, whose terms otherwise cancel a thousand to one) collects it N times over."""

    def forward(self, x):
        if x.dtype != torch.float32:
            return super().forward(x)
        self._check_input_dim(x)
        momentum = 0.0 if self.momentum is None else self.momentum
        if self.training and self.track_running_stats and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
            if self.momentum is None:
                momentum = 1.0 / float(self.num_batches_tracked)
        training = self.training or self.running_mean is None
        stats = self.running_mean is not None and (not self.training or self.track_running_stats)
        rm, rv = (self.running_mean.double(), self.running_var.double()) if stats else (None, None)
        w, b = (self.weight.double(), self.bias.double()) if self.affine else (None, None)
        y = torch.nn.functional.batch_norm(x.double(), rm, rv, w, b, training, momentum, self.eps)
        if training and stats:
            self.running_mean.copy_(rm)
            self.running_var.copy_(rv)
        return y.to(x.dtype)


class _GENLinear(_LinB):
    """A ``Linear`` of GENConv's MLP: PyG's parameter names, ``_LinearFn``'s GEMMs (``strict``: see there)."""
    strict = False

    def forward(self, x):
        return _LinearFn.apply(x, self.weight, self.bias, self.strict)


class _GENConvFn(_Fn):
    """The graph part of ``GENConv``, ONE launch per direction (``ops.gather_softmax`` / ``ops.gather_softmax_bwd``).  Inputs: x,
    ``lin_src`` / ``lin_dst`` weights and biases (None with in == out), the temperature parameter (None unless learnt), the graph, the
    temperature's value, the message eps, ``fuse_root`` (False with ``msg_norm``: the root add is torch work around the launch) and
    ``want`` (whether a backward can follow).

    * in != out: ONE GEMM against ``[lin_src.weight ; lin_dst.weight]`` gives the row buffer ``[H | D]``; the launch gives
      ``D + agg`` (``fuse_root``) or ``agg`` -- then the function returns ``(agg, D)``.  Backward: the launch writes ``[dH | dD]`` into
      one gradient row buffer (without ``fuse_root`` the ``dD`` block is a copy of the second output's gradient), then ONE wgrad and
      ONE dgrad GEMM.
    * in == out: no GEMM; the launch runs on x with ``root = x``, and ``dx = dOut + scatter`` comes from the one backward launch.

    The backward's ``Y'`` (the aggregate without the root) is ``y - root``, one torch elementwise op, where the root was fused.
    The temperature's gradient is the float64 sum of the launch's per-row partials (they are of both signs), rounded once.
    Saved: the padded x and packed weight (in != out), H (x itself with in == out), y, lse."""

    @staticmethod
    def forward(ctx, x, ws, bs, wd, bd, tpar, graph, t, eps, fuse_root, want):
        dt = x.dtype
        need = bool(want) and any(ctx.needs_input_grad[:6])
        ctx.graph, ctx.scal, ctx.fuse, ctx.lin = graph, (t, eps), bool(fuse_root), ws is not None
        if ctx.lin:
            xp, wp, buf, spans = _packed_gemm(x, (ws, wd), (bs, bd), dtype=dt)   # buf [N, 2 out rounded up to 4]: H | D | zero padding
            h, d = _cols(buf, spans[0]), _cols(buf, spans[1])
            ctx.spans, ctx.cin = spans, x.shape[1]
        else:
            h = d = x.detach().contiguous()
        y, lse = ops.gather_softmax(graph, h, t, msg_eps=eps, root=d if fuse_root else None, want_lse=need)
        if need:
            ctx.save_for_backward(*((xp, wp) if ctx.lin else ()), h, d, y, lse)
        if fuse_root:
            return y
        if ctx.lin:
            return y, d
        return y

    @staticmethod
    def _backward(ctx, dy, dd=None):
        graph, (t, eps), need = ctx.graph, ctx.scal, ctx.needs_input_grad
        *lin, h, d, y, lse = ctx.saved_tensors
        dy = dy.contiguous().to(h.dtype)
        yp = y - d if ctx.fuse else y
        if not ctx.lin:
            dx, _, dtr = ops.gather_softmax_bwd(graph, dy, h, yp, lse, t, msg_eps=eps, root="add" if ctx.fuse else False,
                                                want_dt=need[5])
            return dx, None, None, None, None, (dtr.double().sum().to(dtr.dtype).view(1) if need[5] else None), None, None, None, None, None
        xp, wp = lin
        gb = _grad_rows(dy.shape[0], ctx.spans, wp.shape[0], dy.device, h.dtype)
        _, _, dtr = ops.gather_softmax_bwd(graph, dy, h, yp, lse, t, msg_eps=eps, root=ctx.fuse, want_dt=need[5], out=gb)   # gb = [dH | dD | 0]
        if not ctx.fuse:
            _cols(gb, ctx.spans[1]).copy_(dd)
        dx, (dws, dwd), (dbs, dbd) = _packed_grads(gb, xp, wp, ctx.spans, ctx.cin, (need[1], need[3]), (need[2], need[4]), need[0])
        return dx, dws, dbs, dwd, dbd, (dtr.double().sum().to(dtr.dtype).view(1) if need[5] else None), None, None, None, None, None


class _SoftmaxAggr(nn.Module):
    """PyG's ``SoftmaxAggregation(t, learn)`` as a parameter holder: ``t`` is a [1] parameter with ``learn``, else a float."""

    def __init__(self, t, learn):
        super().__init__()
        self._init_t, self.learn = float(t), bool(learn)
        self.t = nn.Parameter(torch.full((1,), float(t))) if learn else float(t)

    def reset_parameters(self):
        if self.learn:
            with torch.no_grad():
                self.t.fill_(self._init_t)


class _ScaleFn(torch.autograd.Function):
    """``u * scale`` with ``scale`` [1].  The gradient of the scale is the sum of N x C signed terms that largely cancel: it is
    accumulated in float64 (one elementwise pass over [N, C]) and rounded once."""

    @staticmethod
    def forward(ctx, u, scale):
        ctx.save_for_backward(u, scale)
        return u * scale

    @staticmethod
    def backward(ctx, dy):
        u, scale = ctx.saved_tensors
        ds = (dy.double() * u.double()).sum().to(scale.dtype).view(1) if ctx.needs_input_grad[1] else None
        return (dy * scale if ctx.needs_input_grad[0] else None), ds


class _MessageNorm(nn.Module):
    """PyG's ``MessageNorm(learn_scale)``: ``normalize(msg, p=2, dim=-1) * ||x||_2 * scale``; ``scale`` [1], initialised to 1, always in
    the ``state_dict``, ``requires_grad = learn_scale``."""

    def __init__(self, learn_scale=False):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(1), requires_grad=bool(learn_scale))

    def reset_parameters(self):
        with torch.no_grad():
            self.scale.fill_(1.0)

    def forward(self, x, msg):
        return _ScaleFn.apply(torch.nn.functional.normalize(msg, p=2.0, dim=-1) * x.norm(p=2, dim=-1, keepdim=True), self.scale)


class GENConv(nn.Module):
    """``torch_geometric.nn.GENConv`` 2.2.0 (Li et al., DeeperGCN, 2020) on the HIP kernels,
    ``GENConv(in_channels, out_channels, aggr="softmax", t=1.0, learn_t=False, p=1.0, learn_p=False, msg_norm=False,
    learn_msg_scale=False, norm="batch", num_layers=2, expansion=2, eps=1e-7, bias=False, edge_dim=None)``,
    ``forward(x, edge_index, edge_attr=None, size=None)`` (restated from the published 2.2.0 source from memory -- PyG cannot be
    installed here, so this could not be checked against it; the pin is the float64 restatement ``tests/gen_ref.py``):

    * ``h = lin_src(x)`` (in != out, else x); ``agg_i = sum_j softmax_j(t m_j) m_j`` per channel over the edges j -> i with the message
      ``m_j = relu(h_j) + eps`` (PyG's ``SoftmaxAggregation``: the mean at t = 0, the max as t -> inf); with ``msg_norm``
      ``agg = normalize(agg, p=2, dim=-1) * ||x_i||_2 * msg_norm.scale`` (the RAW x); ``out = agg + lin_dst(x)`` (in != out, else
      ``+ x``); ``return mlp(out)``.  Parameters: ``lin_src.weight`` / ``lin_dst.weight`` [out, in] (only with in != out; ``.bias``
      with ``bias=True``), ``aggr_module.t`` [1] (only with ``learn_t``), ``msg_norm.scale`` [1] (only with ``msg_norm``; always in
      the ``state_dict``, trained with ``learn_msg_scale``), and the MLP, an ``nn.Sequential`` of ``num_layers - 1`` hidden blocks
      ``Linear(., out * expansion)``, the norm (``BatchNorm1d`` for ``"batch"``, ``LayerNorm`` for ``"layer"``, absent for None),
      ``ReLU``, ``Dropout(0.)`` and a last ``Linear(., out)``: ``mlp.0``, ``mlp.1``, ``mlp.4`` for two layers.  Every Linear is
      uniform(+-1/sqrt(fan-in)) and has a bias only with ``bias=True``.
    * the launches (``_GENConvFn``): in != out -- ONE GEMM against the packed ``[lin_src.weight ; lin_dst.weight]`` gives ``[H | D]``,
      ONE ``ops.gather_softmax`` launch gives ``D + agg`` (the message is formed in registers), ONE ``ops.gather_softmax_bwd`` launch
      writes ``[dH | dD]``, then one wgrad and one dgrad GEMM; in == out -- no GEMM in the graph part, the launch runs on x with root x.
      With ``msg_norm`` the launch runs without root and the normalisation and the root add are torch work on [N, .] around it.  The
      MLP's Linears go through the project's GEMMs (``_LinearFn``); the norm and the ReLU are torch modules.  With ``msg_norm`` and
      ``learn_msg_scale`` alone the Linears run in GEMM mode 0 and the BatchNorm normalises in float64 (``_BatchNorm1d64``): the
      scale's scalar gradient cancels a thousand to one.  ``aggr_module.t``'s
      gradient is the sum of the backward launch's per-row partials.  No [E, .] tensor and no ``index_add_`` / ``scatter`` exist at
      any point.  The graph is GATConv's without loops: ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=False)``.
      Symmetric edge STRUCTURE only.  A learnt temperature is read back to the host once per forward (its value is a launch argument).
    * no self loops are added, an explicit loop is an ordinary edge, a duplicate edge counts twice in the softmax, a node without
      incoming edges gets ``mlp(lin_dst(x_i))``.  Differentiable w.r.t. x and every parameter; float32, bitwise reproducible; a
      forward without a gradient stores no ``lse``.
    * refused with ``ValueError`` before any launch: ``aggr`` other than ``"softmax"`` (``"powermean"`` / ``"power"`` is the named
      follow-up: a second mode of the same sweep; ``"softmax_sg"`` too), ``edge_dim`` / ``edge_attr`` (the message becomes
      per-edge), ``learn_p=True``, ``norm="instance"`` or any other name, ``num_layers < 1``, tuple ``in_channels`` or a tuple ``x``
      (bipartite), ``size``, bf16 features, a CPU ``x``, an ``x`` that is not [N, in]."""

    def __init__(self, in_channels, out_channels: int, aggr="softmax", t: float = 1.0, learn_t: bool = False, p: float = 1.0,
                 learn_p: bool = False, msg_norm: bool = False, learn_msg_scale: bool = False, norm="batch", num_layers: int = 2,
                 expansion: int = 2, eps: float = 1e-7, bias: bool = False, edge_dim=None, **kwargs):
        super().__init__()
        _no_tuple_channels("GENConv", in_channels)
        if aggr != "softmax":
            raise ValueError("GENConv: only aggr='softmax' is implemented on the HIP path ('powermean' is the named follow-up), got %r"
                             % (aggr,))
        _not_implemented("GENConv", edge_dim=edge_dim)
        if learn_p:
            raise ValueError("GENConv: learn_p=True belongs to the power-mean aggregation, which is not implemented on the HIP path")
        if norm not in ("batch", "layer", None):
            raise ValueError("GENConv: norm must be 'batch', 'layer' or None on the HIP path, got %r" % (norm,))
        _int_ge1("GENConv", "num_layers", num_layers)
        _int_ge1("GENConv", "expansion", expansion)
        if not math.isfinite(float(t)) or not math.isfinite(float(eps)) or float(eps) < 0:
            raise ValueError("GENConv: t must be finite and eps a finite float >= 0, got t=%r, eps=%r" % (t, eps))
        if kwargs:
            raise TypeError("GENConv: unexpected keyword arguments %s" % sorted(kwargs))
        self.in_channels, self.out_channels, self.aggr, self.eps = in_channels, out_channels, aggr, float(eps)
        self.aggr_module = _SoftmaxAggr(t, learn_t)
        if in_channels != out_channels:
            self.lin_src = _LinB(in_channels, out_channels, bias=bias)
            self.lin_dst = _LinB(in_channels, out_channels, bias=bias)
        widths = [out_channels] + [out_channels * expansion] * (num_layers - 1) + [out_channels]
        # msg_norm.scale's gradient is ONE scalar, sum_i,c dOut u with u >= 0, whose terms cancel about a thousand to one: an error of
        # dOut that is the same in every row (1e-8 of its size is enough) is collected N times over.  Where that scalar exists, the
        # MLP that produces dOut takes its BatchNorm in float64 and runs its GEMMs in the strict mode (Accuracy).
        sensitive = bool(msg_norm and learn_msg_scale)
        layers = []
        for i in range(1, len(widths)):
            layers.append(_GENLinear(widths[i - 1], widths[i], bias=bias))
            if i < len(widths) - 1:
                if norm == "batch":
                    layers.append((_BatchNorm1d64 if sensitive else nn.BatchNorm1d)(widths[i], affine=True))
                elif norm == "layer":
                    layers.append(nn.LayerNorm(widths[i], elementwise_affine=True))
                layers += [nn.ReLU(), nn.Dropout(0.0)]
        self.mlp = nn.Sequential(*layers)
        if msg_norm:
            self.msg_norm = _MessageNorm(learn_msg_scale)
        for m in self.mlp:
            if isinstance(m, _GENLinear):
                m.strict = sensitive
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, _Lin):
                    _reset_linear(m)
                elif isinstance(m, (nn.BatchNorm1d, nn.LayerNorm, _SoftmaxAggr, _MessageNorm)):
                    m.reset_parameters()

    def forward(self, x, edge_index, edge_attr=None, size=None) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present)."""
        _no_tuple_x("GENConv", x)
        _not_implemented("GENConv", edge_attr=edge_attr, size=size)
        _check_x("GENConv", x, self.in_channels)
        _need_gpu("GENConv", x, exc=ValueError)
        _need_entries("GENConv", edge_index)
        return self._core(x, edge_index)

    def _core(self, x, edge_index):
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=False)
            lin = self.in_channels != self.out_channels
            ws, bs, wd, bd = (self.lin_src.weight, self.lin_src.bias, self.lin_dst.weight, self.lin_dst.bias) if lin else (None,) * 4
            tpar = self.aggr_module.t if self.aggr_module.learn else None
            t = float(tpar.detach()) if tpar is not None else self.aggr_module.t
            fuse = not hasattr(self, "msg_norm")
            want = torch.is_grad_enabled() and any(v is not None and v.requires_grad for v in (x, ws, bs, wd, bd, tpar))
            out = _GENConvFn.apply(x, ws, bs, wd, bd, tpar, graph, t, self.eps, fuse, want)
            if not fuse:
                agg, root = out if lin else (out, x)
                out = self.msg_norm(x, agg) + root
            return self.mlp(out)

    def extra_repr(self):
        return "%d, %d, aggr=%s" % (self.in_channels, self.out_channels, self.aggr)


class _CGConvFn(_Fn):
    """With ``lin_f.weight = [Wf_i | Wf_j | Ef]`` and ``lin_s.weight = [Ws_i | Ws_j | Es]`` (columns ``x_i | x_j | edge_attr``) the
    linear layers on ``cat[x_i, x_j, e_ij]`` split by columns: ONE GEMM against the packed weight [Wf_i ; Ws_i ; Wf_j ; Ws_j] with
    the lin biases on the first two blocks gives the row buffer [Af | As | Bf | Bs], then ONE launch forms both gates of every edge
    in registers -- ``sigmoid(Af[i] + Bf[j] + Ef e_ij) * softplus(As[i] + Bs[j] + Es e_ij)`` -- and gathers (``ops.cgate_fwd``;
    ``root``: the residual x_i rides in as the start of the sums).  Saved: the padded x, the packed weight, the row buffer, the
    float32 attributes and the two transposed [dim, C] edge blocks -- nothing per edge.  Backward: the row-side launch (dAf, dAs and
    the rows' shares of dEf / dEs) and the node-side launch (dBf, dBs), both recomputing the gates, into ONE row buffer
    [dAf | dAs | dBf | dBs]; the lin bias gradients are column sums of its first two blocks, dEf / dEs the column sum of the shares,
    then ONE wgrad and ONE dgrad GEMM on it; the residual's gradient is added to dx."""

    @staticmethod
    def forward(ctx, x, wf, bf, ws, bs, attr, graph, dim, mean, root):
        C = x.shape[1]
        blocks = (wf[:, :C], ws[:, :C], wf[:, C:2 * C], ws[:, C:2 * C])
        xp, wp, buf, spans = _packed_gemm(x, blocks, (bf, bs, None, None))    # buf: Af | As | Bf | Bs | zero padding
        a32 = eft = est = None
        if dim > 0:
            a32 = attr.detach().to(torch.float32).contiguous()    # (float64 attributes are rounded once)
            eft = wf.detach()[:, 2 * C:].t().to(torch.float32).contiguous()
            est = ws.detach()[:, 2 * C:].t().to(torch.float32).contiguous()
        y = ops.cgate_fwd(graph, *(_cols(buf, sp) for sp in spans), attr=a32, ef=eft, es=est, root=xp[:, :C] if root else None,
                          mean=mean)
        ctx.save_for_backward(xp, wp, buf, a32, eft, est)
        ctx.graph, ctx.spans, ctx.opts = graph, spans, (C, dim, mean, root)
        return y

    @staticmethod
    def _backward(ctx, dy):
        xp, wp, buf, a32, eft, est = ctx.saved_tensors
        graph, spans, (C, dim, mean, root), need = ctx.graph, ctx.spans, ctx.opts, ctx.needs_input_grad
        dy = dy.contiguous().to(torch.float32)
        blocks = tuple(_cols(buf, sp) for sp in spans)
        g = _grad_rows(dy.shape[0], spans, wp.shape[0], dy.device)             # [dAf | dAs | dBf | dBs | 0]
        gaf, gas, gbf, gbs = (_cols(g, sp) for sp in spans)
        want_e = dim > 0 and (need[1] or need[3])
        _, _, parts = ops.cgate_bwd_row(graph, dy, *blocks, attr=a32, ef=eft, es=est, mean=mean, out_f=gaf, out_s=gas,
                                        want_parts=want_e)
        ops.cgate_bwd_node(graph, dy, *blocks, attr=a32, ef=eft, es=est, mean=mean, out_f=gbf, out_s=gbs)
        dbf = _bias_grad(gaf) if need[2] else None
        dbs = _bias_grad(gas) if need[4] else None
        de = ops.gatv2_datt(parts, 2 * dim) if want_e else None                # [dEf^T ; dEs^T], [dim, C] each
        dx, (dfi, dsi, dfj, dsj), _ = _packed_grads(g, xp, wp, spans, C, (need[1], need[3], need[1], need[3]), None, need[0])
        dwf = dws = None
        if need[1]:
            dwf = torch.cat([dfi, dfj] + ([de[:dim].t()] if dim > 0 else []), 1)
        if need[3]:
            dws = torch.cat([dsi, dsj] + ([de[dim:].t()] if dim > 0 else []), 1)
        if dx is not None and root:
            dx = dx + dy
        return dx, dwf, dbf, dws, dbs, None, None, None, None, None


class CGConv(nn.Module):
    """``torch_geometric.nn.CGConv`` 2.2.0 (Xie & Grossman, "Crystal Graph Convolutional Neural Networks", PRL 2018) on the HIP
    kernels (restated from the published source from memory -- PyG cannot be installed here, so this could not be
    checked against it; the pin is the float64 restatement ``tests/cg_ref.py``),
    ``CGConv(channels, dim=0, aggr="add", batch_norm=False, bias=True)``, ``forward(x, edge_index, edge_attr=None)``.  It is the
    one operator here in which a learned function of the edge attribute enters a per-channel nonlinearity, and it is
    width-preserving and residual.

    * parameters ``lin_f`` / ``lin_s``: ``weight`` [C, 2 C + dim] with the columns ``x_i | x_j | edge_attr`` and ``bias`` [C]
      (registered as None with ``bias=False``), uniform(+-1/sqrt(2 C + dim)); ``bn``: a ``torch.nn.BatchNorm1d(C)`` with
      ``batch_norm`` (same parameters, buffers and ``state_dict``; it normalises in float64 and rounds once), else None.
    * for an edge j -> i with ``z = cat[x_i, x_j, e_ij]``: ``out_i = x_i + sum_{j -> i} sigmoid(lin_f(z)) * softplus(lin_s(z))``
      (``aggr="mean"``: the sum divided by the number of edges into i); with ``batch_norm`` the sum goes through ``bn`` before
      ``x_i`` is added, in PyG's order.  No self loops are added, an explicit loop is an ordinary edge, duplicate edges each count
      with their own attributes, a node without incoming edges returns ``x_i`` (``bn`` of a zero row with ``batch_norm``).
    * the launches: ``_CGConvFn``.  No [E, 2 C + dim] concatenation, no [E, C] pre-activation, gate or message and no
      ``index_add_`` exist at any point, in the backward either: it recomputes both gates.  The graph is
      ``ops.graph_for(edge_index, N, norm="gat", add_self_loops=False)``, same handle and cache key as the other operators on it.
      Symmetric edge STRUCTURE only.
    * differentiable w.r.t. x and every parameter; float32, bitwise reproducible.
    * refused with ``ValueError`` before any launch: tuple ``channels`` or a tuple ``x`` (bipartite), ``dim`` that is not an integer
      in [0, ``ops.CG_MAX_DIM``], ``aggr`` other than ``"add"`` / ``"sum"`` / ``"mean"``, ``edge_attr`` missing with ``dim > 0``,
      given with ``dim == 0``, not [E, dim], not float32 / float64 (float64 is rounded to float32 once) or requiring grad (the
      gradient w.r.t. ``edge_attr`` is not implemented), bf16 features, CPU tensors, an ``x`` that is not [N, channels]."""

    def __init__(self, channels, dim: int = 0, aggr: str = "add", batch_norm: bool = False, bias: bool = True, **kwargs):
        super().__init__()
        if isinstance(channels, (tuple, list)):
            raise ValueError("CGConv: tuple channels (bipartite graphs) are not implemented on the HIP path")
        _int_ge1("CGConv", "channels", channels)
        if not isinstance(dim, int) or isinstance(dim, bool) or not 0 <= dim <= ops.CG_MAX_DIM:
            raise ValueError("CGConv: dim must be an integer in [0, %d] on the HIP path, got %r" % (ops.CG_MAX_DIM, dim))
        _check_aggr("CGConv", aggr, ("add", "sum", "mean"), kwargs)
        self.channels, self.dim, self.aggr, self.batch_norm = channels, dim, aggr, bool(batch_norm)
        self.lin_f = _LinB(2 * channels + dim, channels, bias=bias)
        self.lin_s = _LinB(2 * channels + dim, channels, bias=bias)
        # The lin biases' gradients sum dOut over ALL rows against weights of one sign (f (1 - f) s and f sigmoid(S) are positive),
        # and a BatchNorm backward gives dOut a zero column sum: the terms cancel a hundred to one and more, and the float32
        # BatchNorm's column means carry an error that is the same in every row and is collected N times over (measured: 1.6e-5 of
        # lin_s.bias's gradient on a 1800-node graph).  So ``bn`` takes its statistics in float64, as GENConv's does.
        self.bn = _BatchNorm1d64(channels) if batch_norm else None
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            _reset_linear(self.lin_f)
            _reset_linear(self.lin_s)
        if self.bn is not None:
            self.bn.reset_parameters()

    def forward(self, x, edge_index, edge_attr=None) -> torch.Tensor:
        """``edge_index`` must have a symmetric structure (both directions of every edge present); ``edge_attr``: [E, dim], float32
        or float64 (rounded to float32 once), not requiring grad -- None with ``dim == 0``."""
        _no_tuple_x("CGConv", x)
        _check_x("CGConv", x, self.channels)
        if self.dim == 0:
            if edge_attr is not None:
                raise ValueError("CGConv: edge_attr given but the layer was built with dim=0")
        else:
            if not isinstance(edge_attr, torch.Tensor):
                raise ValueError("CGConv: edge_attr ([E, %d]) is required" % self.dim)
            if edge_attr.dim() != 2 or tuple(edge_attr.shape) != (edge_index.shape[1], self.dim):
                raise ValueError("CGConv: edge_attr must be [%d, %d], got %s" % (edge_index.shape[1], self.dim, tuple(edge_attr.shape)))
            if edge_attr.dtype not in (torch.float32, torch.float64):
                raise ValueError("CGConv: edge_attr must be float32 or float64, got %s" % edge_attr.dtype)
            if edge_attr.requires_grad:
                raise ValueError("CGConv: the gradient with respect to edge_attr is not implemented on the HIP path: pass "
                                 "edge_attr.detach()")
        _need_gpu("CGConv", x, edge_attr, exc=ValueError)
        _need_entries("CGConv", edge_index)
        with ops.on_device(x):
            graph = ops.graph_for(edge_index, x.shape[0], norm="gat", add_self_loops=False)
            out = _CGConvFn.apply(x, self.lin_f.weight, self.lin_f.bias, self.lin_s.weight, self.lin_s.bias, edge_attr, graph,
                                  self.dim, self.aggr == "mean", self.bn is None)
        return out if self.bn is None else self.bn(out) + x

    def extra_repr(self):
        return "%d, dim=%d, aggr=%s, batch_norm=%s" % (self.channels, self.dim, self.aggr, self.bn is not None)

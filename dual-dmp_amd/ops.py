"""Tensor-level wrappers over the C ABI (``include/ddmp_hip.h``).

PyTorch is plumbing here: it owns device memory and the stream; every wrapper passes raw device
pointers + sizes to ``libddmp_hip.so`` and enqueues on ``torch.cuda.current_stream()``.
No wrapper has a CPU path: a non-CUDA tensor raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import threading
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import DdmpError, check

SLOPE = 0.01        # nn.LeakyReLU() default, util/networks.py:44
BN_EPS = 1e-5       # nn.BatchNorm1d defaults
BN_MOMENTUM = 0.1


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream on the current device.  The raw getter (what torch's own extensions use) is
    ~20x cheaper than building a torch.cuda.Stream object per launch: 350 launches per iteration made that 2.7 ms of
    host time per step (scripts/host_profile.py)."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_device(dev):
    """Context manager: make ``dev`` (a tensor or a device) the current HIP device.  The C ABI launches on the current
    device's stream and ``ddmp_graph`` allocates there; every module-level entry point (nets, GCNConv, losses,
    trainers) enters this, so ``PosNet(torch.device("cuda:1"))`` works without a ``torch.cuda.set_device`` by the
    caller (as the reference's ``PosNet(device)`` does)."""
    if isinstance(dev, torch.Tensor):
        dev = dev.device
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise DdmpError("the HIP path needs a CUDA (ROCm) device, got %s: there is no CPU fallback" % dev)
    return torch.cuda.device(dev)


class Profiler:
    """Per-call timing with HIP events recorded on the stream the kernels are launched on
    (torch's current stream), plus the ALGORITHMIC bytes / flops of each call.
    Off by default: ``ops.PROF = ops.Profiler()`` switches it on."""

    def __init__(self):
        self.records = []          # (name, key, alg_bytes, flops, survey_bytes, ev0, ev1)

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for name, key, b, f, b8, e0, e1 in self.records:
            a = agg.setdefault((name, key), dict(calls=0, ms=0.0, bytes=0.0, flops=0.0, bytes8d=0.0))
            a["calls"] += 1
            a["ms"] += e0.elapsed_time(e1)
            a["bytes"] += b
            a["flops"] += f
            a["bytes8d"] += b8
        return agg


PROF = None


class _timed:
    __slots__ = ("args", "e0")

    def __init__(self, name, key, alg_bytes=0.0, flops=0.0, survey=None):
        # survey: SURVEY.md 8d's count for the op (gather: every row read once + written once + CSR; GEMM: N (C_in + C_out) s),
        # which leaves out the extra operand streams of the fused forms that alg_bytes includes; default = alg_bytes
        self.args = (name, key, alg_bytes, flops, alg_bytes if survey is None else survey)

    def __enter__(self):
        if PROF is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if PROF is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            PROF.records.append(self.args + (self.e0, e1))
        return False


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def trace_marker():
    """Launch the library's marker kernel on the current stream (cuts a rocprofv3 trace to a region: bench.py)."""
    check(_lib.lib().ddmp_trace_marker(_stream()), "ddmp_trace_marker")


def copy_probe(src, dst, mode=0):
    """Streaming device copy on the library's own kernel (bench.py's yardstick; mode 1: nontemporal)."""
    assert src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous()
    nbytes = src.numel() * src.element_size()
    assert dst.numel() * dst.element_size() >= nbytes
    check(_lib.lib().ddmp_copy_probe(_p(src), _p(dst), nbytes, int(mode), _stream()), "ddmp_copy_probe")


def copy_probe_rows(src, dst):
    """The copy in the gather's access pattern (64-row chunks, one 128-byte slab at a time) of a 2-D row-major tensor."""
    assert src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous() and src.dim() == 2 and dst.shape == src.shape
    check(_lib.lib().ddmp_copy_probe_rows(_p(src), _p(dst), src.shape[0], src.shape[1] * src.element_size(), _stream()),
          "ddmp_copy_probe_rows")


def set_gemm_mode(mode: int):
    """6 = bf16x6 split MFMA (f32-class accuracy), 3 = bf16x3 (~2^-16), 0 = f32-input MFMA; 13 = f16x3 split MFMA
    in the row-panel kernels (f32-class accuracy, scaled operands: the ``scales=`` option of the GEMM calls), bf16x6 elsewhere."""
    check(_lib.lib().ddmp_set_gemm_mode(int(mode)), "ddmp_set_gemm_mode")


def get_gemm_mode() -> int:
    return int(_lib.lib().ddmp_get_gemm_mode())


@contextlib.contextmanager
def gemm_mode(mode: int):
    """The GEMM calls made inside run in ``mode`` (``set_gemm_mode``); the mode that was set before is restored on the way out.  The
    mode is read on the host when a GEMM is dispatched, so this covers exactly the launches enqueued inside the block.  The mode
    is process-wide: a GEMM that ANOTHER host thread dispatches while the block is open runs in ``mode`` too."""
    old = get_gemm_mode()
    if old != mode:
        set_gemm_mode(mode)
    try:
        yield
    finally:
        if old != mode:
            set_gemm_mode(old)


def unfused(name: str) -> bool:
    """DDMP_UNFUSE=name[,name...]: fused routes switched OFF for A/B runs and the fused-vs-composed identity tests (the library
    reads the same variable: csrc/ddmp_common.h).  Engine names: stats, gather_bwd, bnbwd_l0, dgrad_red, tail, wprep, bf16_gemm,
    bf16_spmm_red, equal_width; library names: bnbwd_narrow, dgrad_red_narrow."""
    v = os.environ.get("DDMP_UNFUSE", "")
    return bool(v) and name in v.split(",")


def next_pending() -> int:
    """Diagnostic of the C ABI for per-call options "still recorded for this host thread".  Always 0: the options of an ``_o``
    entry point are arguments of that call and are recorded nowhere."""
    return int(_lib.lib().ddmp_next_pending())


def gemm_forget_planes(planes=None):
    """The prepared-planes registry forgets ``planes`` (a buffer about to be freed; None: everything)."""
    _lib.lib().ddmp_gemm_forget_planes(_p(planes))


# ---------------------------------------------------------------------------------------- per-call options (ABI 3)
class _Opts(ctypes.Structure):
    """``ddmp_opts`` of include/ddmp_hip.h."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("bn_n_total", ctypes.c_double),
                ("bn_C", ctypes.c_int32), ("bn_eps", ctypes.c_float), ("bn_momentum", ctypes.c_float), ("prime", ctypes.c_int32),
                ("bn_in", ctypes.c_void_p * 3), ("bn_out", ctypes.c_void_p * 6), ("slot_a", ctypes.c_void_p),
                ("slot_b", ctypes.c_void_p)]


OPT_BN_FWD, OPT_BN_BWD, OPT_SCALES, OPT_PREPARED = 1, 2, 4, 8


class BnFwd:
    """``bn=`` of a statistics-producing call (bn_stats / gemm_nt_stats / spmm_stats): the second stage of that call's
    reduction also writes what bn_prepare would (out4 rows = scale, shift, mean, rstd; running statistics updated) -- one
    launch less, bitwise the same coefficients.  Explicit per-call option (DDMP_OPT_BN_FWD)."""
    flag = OPT_BN_FWD

    def __init__(self, n_total, gamma, beta, out4, running=None, eps=BN_EPS, momentum=BN_MOMENTUM):
        rm, rv = (None, None) if running is None else running
        self.n_total, self.C, self.eps, self.momentum = float(n_total), gamma.numel(), eps, momentum
        self.ins = (gamma, beta, None)
        self.outs = (out4[0], out4[1], out4[2], out4[3], rm, rv)


class BnBwd:
    """``bn=`` of a call that produces the BatchNorm-backward reductions (bn_bwd_reduce / spmm_bnred / gemm_nn_bnred): its
    second stage also writes what bn_bwd_prepare would (dgamma, dbeta, c10 rows = c1, c0).  DDMP_OPT_BN_BWD."""
    flag = OPT_BN_BWD

    def __init__(self, n_total, bn4, dgamma, dbeta, c10):
        self.n_total, self.C, self.eps, self.momentum = float(n_total), dgamma.numel(), 0.0, 0.0
        self.ins = (bn4[0], bn4[2], bn4[3])
        self.outs = (dgamma, dbeta, c10[0], c10[1], None, None)


def _mk_opts(bn=None, scales=None, prepared=False, want_bn=False, want_scales=False):
    """-> (address | None, keep-alive) of the ddmp_opts block of ONE call.  scales = (slot_a, slot_b | None, prime).
    (want_bn / want_scales: which families of options the call accepts -- documentation at the call sites.)"""
    if bn is None and scales is None and not prepared:
        return None, None
    o = _Opts()
    o.struct_size = ctypes.sizeof(_Opts)
    flags = 0
    if bn is not None:
        flags |= bn.flag
        o.bn_n_total, o.bn_C, o.bn_eps, o.bn_momentum = bn.n_total, bn.C, bn.eps, bn.momentum
        for i, t in enumerate(bn.ins):
            o.bn_in[i] = None if t is None else t.data_ptr()
        for i, t in enumerate(bn.outs):
            o.bn_out[i] = None if t is None else t.data_ptr()
    if scales is not None:
        a, b, prime = scales
        flags |= OPT_SCALES
        o.slot_a = None if a is None else a.data_ptr()
        o.slot_b = None if b is None else b.data_ptr()
        o.prime = int(bool(prime))
    if prepared:
        flags |= OPT_PREPARED
    o.flags = flags
    return ctypes.c_void_p(ctypes.addressof(o)), (o, bn, scales)


def gemm_scales_roll(slots):
    """Once per iteration: the maxima recorded by this iteration's GEMM kernels become the next iteration's scales."""
    assert slots.dtype == torch.float32 and slots.is_contiguous() and slots.shape[-1] == 4
    check(_lib.lib().ddmp_gemm_scales_roll(_p(slots), slots.numel() // 4, _stream()), "ddmp_gemm_scales_roll")


def _chk(t, dtype=torch.float32, name="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise DdmpError("%s must be a CUDA (ROCm) tensor: the HIP path has no CPU fallback" % name)
    if t.device.index != torch.cuda.current_device():
        # the library launches on the CURRENT device's stream and allocates graphs there: a tensor of another device
        # would be addressed from the wrong GPU.  The nets / trainers / losses enter `torch.cuda.device(their device)`
        # themselves; a bare ops call has to be made under the tensor's device.
        raise DdmpError("%s lives on cuda:%d but the current device is cuda:%d: wrap the call in "
                        "`with torch.cuda.device(t.device):`" % (name, t.device.index, torch.cuda.current_device()))
    if t.dtype != dtype:
        raise DdmpError("%s must be %s, got %s" % (name, dtype, t.dtype))
    return t


F32, BF16 = 0, 1            # DDMP_F32 / DDMP_BF16 of include/ddmp_hip.h (feature dtype of the dtype-tagged entry points)


def _dt(t) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise DdmpError("feature tensors are float32 or bfloat16, got %s" % t.dtype)


def _mat(t, name="matrix", like=None):
    """2-D float32 / bfloat16 CUDA tensor with unit inner stride -> (tensor, leading dimension).  ``like``: a tensor
    whose dtype it has to share (all feature operands of one call)."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16:
        _chk(t, torch.bfloat16, name)
    else:
        _chk(t, torch.float32, name)
    if like is not None and like.dtype != t.dtype:
        raise DdmpError("%s is %s but the call's other feature operand is %s" % (name, t.dtype, like.dtype))
    if t.dim() != 2 or t.stride(1) != 1:
        raise DdmpError("%s must be 2-D with contiguous rows" % name)
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)))


class Workspace:
    """Grow-only scratch buffer for split-K partials, pre-split weights and column reductions: one per
    (device, stream, host thread) -- logical ranks emulated as threads on one stream must not share it."""

    _bufs = {}

    @classmethod
    def get(cls, nbytes: int, device) -> torch.Tensor:
        key = (torch.device(device).index, torch.cuda.current_stream().cuda_stream, threading.get_ident())
        buf = cls._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
            cls._bufs[key] = buf
        return buf


# ---------------------------------------------------------------------------------------- graph
class Graph:
    """CSR of A + I with D^-1/2 on the device (``ddmp_graph``).  Built once per edge_index
    (the reference's GCNConv re-normalises on every call, cached=False).  ``norm="sym"``: CSR of A, no self loops (ChebConv)."""

    def __init__(self, handle, n_rows, n_cols, nnz):
        self._h = handle
        self.n_rows, self.n_cols, self.nnz = n_rows, n_cols, nnz
        self.valued = 0                                         # GV_* flags of a valued graph (from_edge_index(valued=...))
        self.nnz_in = 0                                         # its input edges
        self.values_key = None                                  # token of the weight version its values were last set from
        self.values_src = None                                  # that version's weight tensor (None: all ones) -- what a backward
        #                                                         pass saves to restore the values it ran on
        self.n_set_values = self.n_status_reads = 0             # diagnostics: refreshes / reads of the validation word
        self._fin = weakref.finalize(self, _lib.lib().ddmp_graph_destroy, handle)
        a, b, c, d = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        check(_lib.lib().ddmp_graph_info(handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)), "ddmp_graph_info")
        self.max_row_nnz = int(d.value)                         # entries of the longest row (self loop included)

    @property
    def handle(self):
        return self._h

    @classmethod
    def from_edge_index(cls, edge_index: torch.Tensor, num_nodes: int, norm: str = "gcn", valued=None) -> "Graph":
        """``norm``: "gcn" = D^-1/2 (A + I) D^-1/2 (GCNConv) | "sym" = D^-1/2 A D^-1/2 without self loops (ChebConv's S:
        explicit self loops dropped, none added, dinv = 0 and an empty row for a node without edges).

        ``valued`` = GV_* flags (``norm`` is then ignored): a VALUED graph -- coalesced structure built once, values set on the
        device per weight version by ``set_values`` (all-ones weights until then).  The edge structure must be symmetric."""
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise DdmpError("edge_index must be a [2, nnz] int64 tensor")
        if valued is not None:
            ei = edge_index.contiguous()
            h = ctypes.c_void_p()
            st = _lib.lib().ddmp_graph_create_valued(int(num_nodes), int(ei.shape[1]), _p(ei), 1 if ei.is_cuda else 0, int(valued),
                                                     ctypes.byref(h))
            if st == -1:
                raise ValueError("a valued graph needs a symmetric edge STRUCTURE (both directions of every edge present in "
                                 "edge_index) and valid flags: ddmp_graph_create_valued refused the edge list")
            check(st, "ddmp_graph_create_valued")
            g = cls(h, int(num_nodes), int(num_nodes), 0)
            nnz = ctypes.c_int64()
            check(_lib.lib().ddmp_graph_info(h, None, None, ctypes.byref(nnz), None), "ddmp_graph_info")
            g.nnz, g.valued, g.nnz_in = int(nnz.value), int(valued) | GV_VALUED, int(ei.shape[1])
            return g
        if norm not in ("gcn", "sym"):
            raise DdmpError("graph normalisation must be 'gcn' or 'sym', got %r" % (norm,))
        ei = edge_index.contiguous()
        h = ctypes.c_void_p()
        create = _lib.lib().ddmp_graph_create if norm == "gcn" else _lib.lib().ddmp_graph_create_sym
        st = create(int(num_nodes), int(ei.shape[1]), _p(ei), 1 if ei.is_cuda else 0, ctypes.byref(h))
        check(st, "ddmp_graph_create" if norm == "gcn" else "ddmp_graph_create_sym")
        g = cls(h, int(num_nodes), int(num_nodes), int(ei.shape[1]) + int(num_nodes))
        if norm == "sym":                                       # entries = the edges that are not self loops
            nnz = ctypes.c_int64()
            check(_lib.lib().ddmp_graph_info(h, None, None, ctypes.byref(nnz), None), "ddmp_graph_info")
            g.nnz = int(nnz.value)
        return g

    def set_values(self, w=None, key=None, validate=True, checked=False):
        """Values of one weight version (``ddmp_graph_set_values``: device kernels, no host round trip of the values).  ``w``: CUDA
        float32 / float64 [nnz_in] (float64 is rounded to float32 once) or None = all ones.  ``validate``: read the device's
        validation word ONCE and raise ValueError for non-finite weights, a negative weighted degree, or (GV_REQUIRE_SYM)
        values that are not symmetric.  ``key``: the caller's token of this weight version (``values_key`` afterwards).
        ``checked``: the caller has run ``check_edge_weight`` on ``w``."""
        if not self.valued:
            raise DdmpError("set_values needs a valued graph (Graph.from_edge_index(..., valued=flags))")
        src = None if w is None else w.detach()                 # (shares storage and version counter with the caller's tensor)
        if w is not None:
            if not checked:
                check_edge_weight(w, self.nnz_in)
            w = _chk(w.detach().to(torch.float32).contiguous(), torch.float32, "edge_weight")
        self.n_set_values += 1
        with _timed("set_values", (int(round(self.nnz / max(self.n_rows, 1))),), 4.0 * self.nnz_in + 24.0 * self.nnz + 12.0 * self.n_rows):
            check(_lib.lib().ddmp_graph_set_values(self.handle, _p(w), _stream()), "ddmp_graph_set_values")
        self.values_key, self.values_src = key, src
        if validate:
            self.n_status_reads += 1
            st = ctypes.c_int()
            check(_lib.lib().ddmp_graph_values_status(self.handle, ctypes.byref(st), _stream()), "ddmp_graph_values_status")
            if st.value:
                self.values_key = self.values_src = None
                what = [m for b, m in ((GV_ENONFINITE, "edge_weight has non-finite values"),
                                       (GV_ENEGDEG, "a node's weighted degree is negative (PyG's gcn_norm would give NaN)"),
                                       (GV_ENOTSYM, "edge_weight is not symmetric (w_ij != w_ji after coalescing): ChebConv takes "
                                                    "symmetric weights only -- symmetrise them, e.g. (w + w[reverse]) / 2")) if st.value & b]
                raise ValueError("; ".join(what))
        return self

    def values(self):
        """-> (ew, ew_t, a [entries], s [n]) device copies of a valued graph's arrays (tests, diagnostics)."""
        dev = torch.device("cuda", torch.cuda.current_device())
        ew, ew_t, a = (torch.empty(self.nnz, dtype=torch.float32, device=dev) for _ in range(3))
        s_ = torch.empty(self.n_rows, dtype=torch.float32, device=dev)
        check(_lib.lib().ddmp_graph_export_values(self.handle, _p(ew), _p(ew_t), _p(a), _p(s_), _stream()), "ddmp_graph_export_values")
        return ew, ew_t, a, s_

    @classmethod
    def from_csr_host(cls, rowptr: np.ndarray, col: np.ndarray, dinv: np.ndarray, n_cols: int, rows=None) -> "Graph":
        """``rows`` = (row0, row1): only these rows of the tables, as a graph of their own -- output row i is node row0 + i, the
        columns keep the numbering of the whole local graph (same X, the output tensor starts at row row0): the interior /
        boundary halves of a partitioned graph (dist.py)."""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        dinv = np.ascontiguousarray(dinv, dtype=np.float32)
        n_rows = len(rowptr) - 1
        h = ctypes.c_void_p()
        if rows is not None:
            r0, r1 = int(rows[0]), int(rows[1])
            st = _lib.lib().ddmp_graph_create_csr_rows_host(n_rows, int(n_cols), rowptr.ctypes.data, col.ctypes.data,
                                                            dinv.ctypes.data, r0, r1, ctypes.byref(h))
            check(st, "ddmp_graph_create_csr_rows_host")
            return cls(h, r1 - r0, int(n_cols), int(rowptr[r1] - rowptr[r0]))
        st = _lib.lib().ddmp_graph_create_csr_host(n_rows, int(n_cols), rowptr.ctypes.data, col.ctypes.data,
                                                   dinv.ctypes.data, ctypes.byref(h))
        check(st, "ddmp_graph_create_csr_host")
        return cls(h, n_rows, int(n_cols), int(rowptr[-1]))


_graph_cache = {}
_values_token = [0]

# flags of a valued graph (DDMP_GV_* of include/ddmp_hip.h) and the validation bits of set_values
GV_LOOPS, GV_IMPROVED, GV_NORMALIZE, GV_DROP_LOOPS, GV_REQUIRE_SYM, GV_VALUED = 1, 2, 4, 8, 16, 256
GV_ENONFINITE, GV_ENEGDEG, GV_ENOTSYM = 1, 2, 4


def check_edge_weight(w, nnz, need_cuda=True):
    """The refusals that depend on shape, dtype and device only -- ValueError before any launch."""
    if not isinstance(w, torch.Tensor):
        raise ValueError("edge_weight must be a tensor, got %s" % type(w).__name__)
    if w.dim() != 1 or w.shape[0] != int(nnz):
        raise ValueError("edge_weight must have one value per edge: expected shape [%d], got %s" % (int(nnz), tuple(w.shape)))
    if w.dtype not in (torch.float32, torch.float64):
        raise ValueError("edge_weight must be float32 or float64, got %s" % w.dtype)
    if need_cuda and not w.is_cuda:
        raise ValueError("edge_weight must be a CUDA (ROCm) tensor: the HIP path has no CPU fallback")
    return w


def valued_flags(norm="gcn", improved=False, add_self_loops=True, normalize=True):
    """GV_* flags of PyG's options.  "gcn": gcn_norm(improved, add_self_loops) when normalising, the raw weights otherwise
    (no loops added, whatever add_self_loops says); "sym": ChebConv's S -- loops dropped, symmetric values required."""
    if norm == "sym":
        return GV_DROP_LOOPS | GV_NORMALIZE | GV_REQUIRE_SYM
    if not normalize:
        return 0
    return GV_NORMALIZE | ((GV_LOOPS | (GV_IMPROVED if improved else 0)) if add_self_loops else 0)


def graph_for(edge_index: torch.Tensor, num_nodes: int, norm: str = "gcn", edge_weight=None, improved=False,
              add_self_loops=True, normalize=True) -> Graph:
    """Graph of a static mesh, cached on the IDENTITY of the edge_index tensor (weak reference + in-place
    version counter) and the normalisation.  A data_ptr key would be wrong: a freed tensor's address is reused by other meshes.
    A caller that builds a fresh edge_index tensor on every call (as ``data.edge_index.to(device)`` does when
    the dataset lives on the host) gets a correct but rebuilt graph each time -- keep the tensor.

    ``norm``: "gcn" (GCNConv: self loops added) | "sym" (ChebConv: S = D^-1/2 A D^-1/2, no self loops) | "gat" (GATConv: the
    coalesced structure with multiplicities, ``_gat_graph_for``).  A GCNConv and a
    ChebConv on the same edge_index tensor each get their own graph.  "sym" supports SYMMETRIC edge lists only (both
    directions of every edge present, as every graph of this project is): S is then symmetric, the degree is the in-degree,
    and the same graph serves the backward pass.

    ``edge_weight`` (CUDA float32 / float64 [nnz]) or a non-default ``improved`` / ``add_self_loops`` / ``normalize``: a VALUED
    graph.  Its structure is cached like any graph's (identity + version of edge_index, and the options); its values are
    refreshed by ONE ``set_values`` when the identity or ``_version`` of ``edge_weight`` differs from the one last set -- a learned
    weight changes every step and costs that, not a rebuild.  With ``edge_weight=None`` and default options this is today's
    unvalued graph, handle and kernels.

    One handle serves every weight version on a structure, so its values are those of the LAST version set: an autograd function
    that gathers in its backward records ``values_key`` / ``values_src`` in forward and restores them (``restore_values``)."""
    if norm == "gat":
        return _gat_graph_for(edge_index, num_nodes, edge_weight, improved, add_self_loops, normalize)
    if norm not in ("gcn", "sym"):
        raise DdmpError("graph normalisation must be 'gcn' or 'sym', got %r" % (norm,))
    flags = None
    if edge_weight is not None or improved or not add_self_loops or not normalize:
        if edge_weight is not None:
            check_edge_weight(edge_weight, edge_index.shape[1])
        flags = valued_flags(norm, improved, add_self_loops, normalize)
    key = (id(edge_index), norm) if flags is None else (id(edge_index), norm, flags)
    hit = _graph_cache.get(key)
    g = None
    if hit is not None:
        ref, version, n, g_ = hit
        if ref() is edge_index and version == edge_index._version and n == int(num_nodes):
            g = g_
    if g is None:
        for k in [k for k, v in _graph_cache.items() if v[0]() is None]:
            del _graph_cache[k]
        g = Graph.from_edge_index(edge_index, num_nodes, norm, valued=flags)
        _graph_cache[key] = (weakref.ref(edge_index), edge_index._version, int(num_nodes), g)
        if flags is not None:
            g._wref, g.values_key = None, ("ones",)
    if flags is not None:
        if edge_weight is None:
            if g.values_key != ("ones",):
                g.set_values(None, key=("ones",), validate=False)
                g._wref = None
        else:
            cur = getattr(g, "_wref", None)
            if not (cur is not None and cur[0]() is edge_weight and cur[1] == edge_weight._version
                    and g.values_key == cur[2]):
                _values_token[0] += 1
                tok = ("w", _values_token[0])
                g._wref = None
                g.set_values(edge_weight, key=tok, checked=True)
                g._wref = (weakref.ref(edge_weight), edge_weight._version, tok)
    return g


def _gat_graph_for(edge_index, num_nodes, edge_weight, improved, add_self_loops, normalize) -> Graph:
    """``graph_for(..., norm="gat")``: the structure GATConv attends over -- a valued graph with flags GV_LOOPS alone (0 for
    ``add_self_loops=False``: explicit loops stay ordinary entries) that KEEPS its all-ones values: ``a`` is then the multiplicity
    of each coalesced entry, which the edge softmax weighs its terms by.  Cached on the identity + version of ``edge_index``
    under a key of its own: a GCNConv on the same tensor never gets this handle, and ``set_values`` never runs on it."""
    if edge_weight is not None or improved or not normalize:
        raise ValueError("graph_for(norm='gat') takes add_self_loops only: the attention graph has no edge weights")
    flags = GV_LOOPS if add_self_loops else 0
    key = (id(edge_index), "gat", flags)
    hit = _graph_cache.get(key)
    if hit is not None:
        ref, version, n, g = hit
        if ref() is edge_index and version == edge_index._version and n == int(num_nodes):
            return g
    for k in [k for k, v in _graph_cache.items() if v[0]() is None]:
        del _graph_cache[k]
    g = Graph.from_edge_index(edge_index, num_nodes, valued=flags)
    g._wref, g.values_key = None, ("ones",)
    _graph_cache[key] = (weakref.ref(edge_index), edge_index._version, int(num_nodes), g)
    return g


def restore_values(g: Graph, key, w):
    """Backward-pass guard of the valued operators: if another weight version was set on ``g`` since the forward that recorded
    ``key``, set that forward's values again (``w``: its saved weights, None = all ones).  Validated then; no status read."""
    if g is not None and g.valued and g.values_key != key:
        g.set_values(w, key=key, validate=False, checked=True)
        g._wref = None


def csr_build_host(edge_index: np.ndarray, num_nodes: int, norm: str = "gcn"):
    """Host CSR (no GPU needed): -> rowptr int32[n+1], col int32[nnz'], dinv f32[n].  ``norm`` as in ``graph_for``."""
    if norm not in ("gcn", "sym"):
        raise DdmpError("graph normalisation must be 'gcn' or 'sym', got %r" % (norm,))
    ei = np.ascontiguousarray(edge_index, dtype=np.int64)
    nnz = ei.shape[1]
    rowptr = np.zeros(num_nodes + 1, np.int32)
    col = np.zeros(nnz + num_nodes, np.int32)
    dinv = np.zeros(num_nodes, np.float32)
    cap = ctypes.c_int64(nnz + num_nodes)
    build = _lib.lib().ddmp_csr_build_host if norm == "gcn" else _lib.lib().ddmp_csr_build_sym_host
    st = build(num_nodes, nnz, ei.ctypes.data, rowptr.ctypes.data, col.ctypes.data, dinv.ctypes.data, ctypes.byref(cap))
    check(st, "ddmp_csr_build_host" if norm == "gcn" else "ddmp_csr_build_sym_host")
    return rowptr, col[:cap.value].copy(), dinv


def csr_build_valued_host(edge_index: np.ndarray, num_nodes: int, flags: int):
    """Host structure of a valued graph (no GPU needed; ``ddmp_csr_build_valued_host``): -> dict of rowptr [n+1], col, mirror
    [entries], ee_ptr [entries+1], ee_idx, eid [nnz] (int32).  ValueError when the edge structure is not symmetric."""
    ei = np.ascontiguousarray(edge_index, dtype=np.int64)
    nnz, n = ei.shape[1], int(num_nodes)
    cap = nnz + n
    rowptr, col, mirror = np.zeros(n + 1, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    ee_ptr, ee_idx, eid = np.zeros(cap + 1, np.int32), np.zeros(max(nnz, 1), np.int32), np.zeros(max(nnz, 1), np.int32)
    used = ctypes.c_int64(cap)
    st = _lib.lib().ddmp_csr_build_valued_host(n, nnz, ei.ctypes.data, int(flags), rowptr.ctypes.data, col.ctypes.data,
                                               ee_ptr.ctypes.data, ee_idx.ctypes.data, eid.ctypes.data, mirror.ctypes.data,
                                               ctypes.byref(used))
    if st == -1:
        raise ValueError("ddmp_csr_build_valued_host: the edge structure is not symmetric (or the flags are invalid)")
    check(st, "ddmp_csr_build_valued_host")
    ne = used.value
    return dict(rowptr=rowptr, col=col[:ne].copy(), mirror=mirror[:ne].copy(), ee_ptr=ee_ptr[:ne + 1].copy(),
                ee_idx=ee_idx[:int(ee_ptr[ne])].copy(), eid=eid[:nnz].copy())


def valued_values_host(tables, w, flags: int):
    """Host restatement of ``ddmp_graph_set_values`` in float32, the device's summation orders: -> a, s, ew, ew_t (numpy
    float32).  An entry's edges are summed in input order, a row's entries in CSR order, s = float32(1 / sqrt(float64(deg)))."""
    rowptr, col, mirror, ee_ptr, ee_idx = (tables[k] for k in ("rowptr", "col", "mirror", "ee_ptr", "ee_idx"))
    ne, n = len(col), len(rowptr) - 1
    w = None if w is None else np.asarray(w, dtype=np.float32)
    fill = np.float32(2.0 if flags & GV_IMPROVED else 1.0)
    a = np.zeros(ne, np.float32)
    for e in range(ne):
        t0, t1 = int(ee_ptr[e]), int(ee_ptr[e + 1])
        v = fill if t0 == t1 else np.float32(0.0)
        for t in range(t0, t1):
            v = np.float32(v + (np.float32(1.0) if w is None else w[ee_idx[t]]))
        a[e] = v
    s = np.ones(n, np.float32)
    if flags & GV_NORMALIZE:
        for i in range(n):
            deg = np.float32(0.0)
            for e in range(int(rowptr[i]), int(rowptr[i + 1])):
                deg = np.float32(deg + a[e])
            s[i] = np.float32(1.0 / np.sqrt(np.float64(deg))) if deg > 0 else np.float32(0.0)
        ew = (a * s[col]).astype(np.float32)
        ew_t = (a[mirror] * s[col]).astype(np.float32)
    else:
        ew, ew_t = a.copy(), a[mirror].copy()
    return a, s, ew, ew_t


def bfs_order_host(rowptr: np.ndarray, col: np.ndarray) -> np.ndarray:
    n = len(rowptr) - 1
    order = np.zeros(n, np.int32)
    st = _lib.lib().ddmp_csr_bfs_order_host(n, rowptr.ctypes.data, col.ctypes.data, order.ctypes.data)
    check(st, "ddmp_csr_bfs_order_host")
    return order


def rcb_order_host(points: np.ndarray, leaf: int = 64) -> np.ndarray:
    """Recursive-coordinate-bisection node order (new id -> old id) of ``points`` [n,3]: leaves of ``leaf`` consecutive
    ids are compact patches of the surface (ddmp_rcb_order_host; host code, no GPU needed)."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise DdmpError("rcb_order_host: points must be [n,3]")
    order = np.zeros(len(p), np.int32)
    check(_lib.lib().ddmp_rcb_order_host(len(p), p.ctypes.data, int(leaf), order.ctypes.data), "ddmp_rcb_order_host")
    return order


# ---------------------------------------------------------------------------------------- kernels
def spmm(g: Graph, x, out=None, bias=None, pro=None, slope=SLOPE, transpose=False):
    """out[i] = dinv_i * sum_j dinv_j f(x[j]) (+bias); x has g.n_cols rows, out g.n_rows rows.  A valued graph: out = A x (+bias)
    with its current values, float32 features, no prologue; ``transpose=True``: out = A^T x (same structure, mirrored values)."""
    x, ldx = _mat(x, "x")
    if g.valued and (x.dtype != torch.float32 or pro is not None):
        raise ValueError("a valued graph gathers float32 features without a prologue (bf16 features with edge_weight are not supported)")
    if transpose and not g.valued:
        raise DdmpError("transpose=True needs a valued graph (an unvalued graph's operator is symmetric)")
    if x.shape[0] < g.n_cols:
        raise DdmpError("x has %d rows, graph references %d nodes" % (x.shape[0], g.n_cols))
    C = x.shape[1]
    if out is None:
        out = torch.empty((g.n_rows, C), dtype=x.dtype, device=x.device)
    out, ldy = _mat(out, "out", x)
    ps, psh = (None, None) if pro is None else pro
    es = x.element_size()
    # algorithmic bytes: every feature row read once + written once, int32 col ids, rowptr, dinv
    alg = 2.0 * g.n_rows * C * es + 4.0 * g.nnz + 4.0 * (g.n_rows + 1) + 4.0 * g.n_rows
    with _timed("spmm", (C, int(round(g.nnz / max(g.n_rows, 1)))), alg, 2.0 * g.nnz * C):      # key: width, CSR entries per row
        if transpose:
            st = _lib.lib().ddmp_spmm_t_f32(g.handle, _p(x), ldx, _p(out), ldy, C, _p(bias), _stream())
        else:
            st = _lib.lib().ddmp_spmm(g.handle, _p(x), ldx, _p(out), ldy, C, _dt(x), _p(bias), _p(ps), _p(psh), slope,
                                      _stream())
    check(st, "ddmp_spmm")
    return out


def sddmm(g: Graph, dy, h, out=None):
    """out[e] = sum_c dy[row e, c] * h[col e, c] for every CSR entry of ``g`` (``ddmp_sddmm_f32``): dL/dA per entry of Y = A H.
    float32, fixed summation order (bitwise reproducible).  dy: [>= n_rows, C], h: [>= n_cols, C]; out: float32 [g.nnz]."""
    dy, lddy = _mat(_chk(dy, torch.float32, "dy"), "dy")
    h, ldh = _mat(_chk(h, torch.float32, "h"), "h")
    C = dy.shape[1]
    if h.shape[1] != C or dy.shape[0] < g.n_rows or h.shape[0] < g.n_cols:
        raise DdmpError("sddmm: dy must be [>= %d, C] and h [>= %d, C], got %s and %s" % (g.n_rows, g.n_cols, tuple(dy.shape), tuple(h.shape)))
    if out is None:
        out = torch.empty(g.nnz, dtype=torch.float32, device=dy.device)
    _chk(out, torch.float32, "out")
    if out.numel() < g.nnz or not out.is_contiguous():
        raise DdmpError("sddmm: out must be a contiguous float32 [%d]" % g.nnz)
    # algorithmic bytes: the gathered rows and the rows' own dy once each, one float per entry out, int32 col ids, rowptr
    alg = 4.0 * (g.n_cols + g.n_rows) * C + 8.0 * g.nnz + 4.0 * (g.n_rows + 1)
    with _timed("sddmm", (C, int(round(g.nnz / max(g.n_rows, 1)))), alg, 2.0 * g.nnz * C):
        st = _lib.lib().ddmp_sddmm_f32(g.handle, _p(dy), lddy, _p(h), ldh, C, _p(out), _stream())
    check(st, "ddmp_sddmm_f32")
    return out


def graph_weight_grad(g: Graph, G, out=None):
    """dL/d(edge_weight) [nnz_in] of a valued graph from G = dL/dA per entry (``sddmm``), through its normalisation
    (``ddmp_graph_weight_grad``; formulas in include/ddmp_hip.h and DESIGN.md 4.7)."""
    if not g.valued:
        raise DdmpError("graph_weight_grad needs a valued graph")
    _chk(G, torch.float32, "G")
    if G.numel() < g.nnz or not G.is_contiguous():
        raise DdmpError("graph_weight_grad: G must be a contiguous float32 [%d]" % g.nnz)
    if out is None:
        out = torch.empty(g.nnz_in, dtype=torch.float32, device=G.device)
    _chk(out, torch.float32, "out")
    if g.nnz_in == 0:                                           # (only added self loops: no input edge, nothing to write -- and an
        return out                                              #  empty tensor's null pointer is a missing argument to the library)
    with _timed("graph_weight_grad", (int(round(g.nnz / max(g.n_rows, 1))),), 28.0 * g.nnz + 8.0 * g.nnz_in + 8.0 * g.n_rows):
        check(_lib.lib().ddmp_graph_weight_grad(g.handle, _p(G), _p(out), _stream()), "ddmp_graph_weight_grad")
    return out


# ---------------------------------------------------------------------------------------- graph attention
def _gat_graph(g: Graph):
    if not g.valued or g.values_key != ("ones",):
        raise DdmpError("the attention kernels need the graph of graph_for(edge_index, n, norm='gat'): a valued graph left at its "
                        "all-ones values (its entries' multiplicities)")
    if g.nnz == 0:
        # the per-entry arrays (alpha, dz, w ...) would be empty tensors with a null pointer, which the library takes for a
        # missing argument: refused here, before any launch, not with a status from inside it
        raise ValueError("the graph has no entry at all (no edge and no added self loop): the graph-operator kernels are not "
                         "defined on it")
    return g


def _rows(t, name, rows, width=None):
    """float32 [>= rows, width] row block (a column block of a wider row buffer is fine; ``width=None``: any width) -> (tensor, ld)."""
    t, ld = _mat(_chk(t, torch.float32, name), name)
    if t.shape[0] < rows or t.shape[1] < 1 or (width is not None and t.shape[1] != width):
        raise DdmpError("%s must be [>= %d, %s], got %s" % (name, rows, "C" if width is None else width, tuple(t.shape)))
    return t, ld


def _gat_hf(t, heads, name, rows=0):
    """float32 [>= rows, heads * C] row block -> (tensor, ld, C)."""
    t, ld = _rows(t, name, rows)
    if heads < 1 or t.shape[1] % heads:
        raise DdmpError("%s: width %d is not heads (%d) x C" % (name, t.shape[1], heads))
    return t, ld, t.shape[1] // heads


def _head_mats(g, heads, who, **mats):
    """The [n, heads * C] operands of a call by name -> (n, C, {name: (tensor, ld)}); all of one width."""
    _gat_graph(g)
    n, C, out = g.n_rows, None, {}
    for name, t in mats.items():
        t, ld, c = _gat_hf(t, heads, name, n)
        if C is not None and c != C:
            raise DdmpError("%s: %s differs in width from the other operands" % (who, name))
        C = c
        out[name] = (t, ld)
    return n, C, out


def _out(out, name, rows, width, device):
    """An output row block: ``out`` checked as float32 [>= rows, width], or (None) a new [rows, width] -> (tensor, ld)."""
    if out is None:
        out = torch.empty((rows, width), dtype=torch.float32, device=device)
    return _rows(out, name, rows, width)


def _out_with_root(out, who, n, hc, C, root, device):
    """The [dhf | droot] row buffer of a node-side backward: ``out`` checked as float32 [n, >= hc (+ C with ``root``)], or (None) a
    new one of exactly that width -> ((dhf, ld), (droot, ld) | (None, 0)), views of its leading columns."""
    wt = hc + (C if root else 0)
    if out is None:
        out = torch.empty((n, wt), dtype=torch.float32, device=device)
    out, _ = _mat(_chk(out, torch.float32, "out"), "out")
    if out.shape[0] != n or out.shape[1] < wt:
        raise DdmpError("%s: out must be [%d, >= %d], got %s" % (who, n, wt, tuple(out.shape)))
    return _mat(out[:, :hc], "dhf"), (_mat(out[:, hc:wt], "droot") if root else (None, 0))


def _gat_arr(t, shape, name):
    """contiguous float32 array of exactly ``shape``."""
    _chk(t, torch.float32, name)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise DdmpError("%s must be a contiguous float32 %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def _gat_key(g, heads, C):
    return (heads, C, int(round(g.nnz / max(g.n_rows, 1))))


def gat_scores(hf, att_src, att_dst, heads):
    """-> (s_src, s_dst) [n, heads]: s[i, h] = sum_c hf[i, h * C + c] * att[h, c] (``ddmp_gat_scores_f32``; att: [heads, C])."""
    hf, ldh, C = _gat_hf(hf, heads, "hf")
    n = hf.shape[0]
    att_src, att_dst = _gat_arr(att_src, (heads, C), "att_src"), _gat_arr(att_dst, (heads, C), "att_dst")
    s_src, s_dst = (torch.empty((n, heads), dtype=torch.float32, device=hf.device) for _ in range(2))
    # algorithmic bytes: hf read once, the two score arrays written, the attention vectors
    with _timed("gat_scores", (heads, C), 4.0 * n * heads * C + 8.0 * n * heads + 8.0 * heads * C, 4.0 * n * heads * C):
        st = _lib.lib().ddmp_gat_scores_f32(_p(hf), ldh, n, heads, C, _p(att_src), _p(att_dst), _p(s_src), _p(s_dst), _stream())
    check(st, "ddmp_gat_scores_f32")
    return s_src, s_dst


def gat_fwd(g: Graph, hf, s_src, s_dst, heads, slope, bias=None, out=None):
    """Edge softmax + gather in one launch (``ddmp_gat_fwd_f32``) -> (y [n, heads * C], alpha [g.nnz, heads]).
    ``bias``: float32 [heads * C] added in the epilogue, or None."""
    _gat_graph(g)
    hf, ldh, C = _gat_hf(hf, heads, "hf", g.n_rows)
    n = g.n_rows
    s_src, s_dst = _gat_arr(s_src, (hf.shape[0], heads), "s_src"), _gat_arr(s_dst, (hf.shape[0], heads), "s_dst")
    if bias is not None:
        bias = _gat_arr(bias, (heads * C,), "bias")
    out, ldy = _out(out, "out", n, heads * C, hf.device)
    alpha = torch.empty((g.nnz, heads), dtype=torch.float32, device=hf.device)
    # algorithmic bytes: every feature row read once + written once, alpha written, both scores read, col + multiplicity, rowptr
    alg = 8.0 * n * heads * C + 4.0 * g.nnz * heads + 8.0 * n * heads + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("gat_fwd", _gat_key(g, heads, C), alg, 2.0 * g.nnz * heads * C, survey=8.0 * n * heads * C + 4.0 * g.nnz + 4.0 * (n + 1)):
        st = _lib.lib().ddmp_gat_fwd_f32(g.handle, _p(hf), ldh, heads, C, _p(s_src), _p(s_dst), float(slope), _p(bias), _p(alpha),
                                         _p(out), ldy, _stream())
    check(st, "ddmp_gat_fwd_f32")
    return out, alpha


def gat_bwd_edge(g: Graph, dout, hf, s_src, s_dst, alpha, heads, slope):
    """Edge side of the backward (``ddmp_gat_bwd_edge_f32``) -> (ds [g.nnz, heads], ds_dst [n, heads])."""
    n, C, m = _head_mats(g, heads, "gat_bwd_edge", dout=dout, hf=hf)
    (dout, lddo), (hf, ldh) = m["dout"], m["hf"]
    s_src, s_dst = _gat_arr(s_src, (hf.shape[0], heads), "s_src"), _gat_arr(s_dst, (hf.shape[0], heads), "s_dst")
    alpha = _gat_arr(alpha, (g.nnz, heads), "alpha")
    ds = torch.empty((g.nnz, heads), dtype=torch.float32, device=hf.device)
    ds_dst = torch.empty((n, heads), dtype=torch.float32, device=hf.device)
    # algorithmic bytes: dout and hf read once each, alpha read, ds written, the scores read, ds_dst written, col, rowptr
    alg = 8.0 * n * heads * C + 8.0 * g.nnz * heads + 12.0 * n * heads + 4.0 * g.nnz + 4.0 * (n + 1)
    with _timed("gat_bwd_edge", _gat_key(g, heads, C), alg, 2.0 * g.nnz * heads * C):
        st = _lib.lib().ddmp_gat_bwd_edge_f32(g.handle, _p(dout), lddo, _p(hf), ldh, heads, C, _p(s_src), _p(s_dst), float(slope),
                                              _p(alpha), _p(ds), _p(ds_dst), _stream())
    check(st, "ddmp_gat_bwd_edge_f32")
    return ds, ds_dst


def gat_bwd_node(g: Graph, dout, alpha, ds, ds_dst, att_src, att_dst, heads):
    """Node side of the backward (``ddmp_gat_bwd_node_f32``) -> (dhf [n, heads * C] written completely, ds_src [n, heads])."""
    _gat_graph(g)
    n = g.n_rows
    dout, lddo, C = _gat_hf(dout, heads, "dout", n)
    alpha, ds = _gat_arr(alpha, (g.nnz, heads), "alpha"), _gat_arr(ds, (g.nnz, heads), "ds")
    ds_dst = _gat_arr(ds_dst, (n, heads), "ds_dst")
    att_src, att_dst = _gat_arr(att_src, (heads, C), "att_src"), _gat_arr(att_dst, (heads, C), "att_dst")
    dhf = torch.empty((n, heads * C), dtype=torch.float32, device=dout.device)
    ds_src = torch.empty((n, heads), dtype=torch.float32, device=dout.device)
    # algorithmic bytes: dout read once, dhf written, alpha and ds read through the mirror map, col + mirror, ds_dst / ds_src, rowptr
    alg = 8.0 * n * heads * C + 8.0 * g.nnz * heads + 8.0 * n * heads + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("gat_bwd_node", _gat_key(g, heads, C), alg, 2.0 * g.nnz * heads * C):
        st = _lib.lib().ddmp_gat_bwd_node_f32(g.handle, _p(dout), lddo, heads, C, _p(alpha), _p(ds), _p(ds_dst), _p(att_src),
                                              _p(att_dst), _p(dhf), dhf.stride(0), _p(ds_src), _stream())
    check(st, "ddmp_gat_bwd_node_f32")
    return dhf, ds_src


def gat_datt(hf, ds_src, ds_dst, heads):
    """-> (datt_src, datt_dst) [heads, C]: datt[h, c] = sum_i ds[i, h] * hf[i, h * C + c] (``ddmp_gat_datt_f32``: two-stage
    column reduction, per-chunk partials in the workspace, fixed order)."""
    hf, ldh, C = _gat_hf(hf, heads, "hf")
    n = hf.shape[0]
    ds_src, ds_dst = _gat_arr(ds_src, (n, heads), "ds_src"), _gat_arr(ds_dst, (n, heads), "ds_dst")
    L = _lib.lib()
    need = L.ddmp_gat_datt_workspace_bytes(n, heads, C)
    ws = Workspace.get(need, hf.device)
    datt_src, datt_dst = (torch.empty((heads, C), dtype=torch.float32, device=hf.device) for _ in range(2))
    with _timed("gat_datt", (heads, C), 4.0 * n * heads * C + 8.0 * n * heads + 2.0 * need, 4.0 * n * heads * C):
        st = L.ddmp_gat_datt_f32(_p(hf), ldh, n, heads, C, _p(ds_src), _p(ds_dst), _p(datt_src), _p(datt_dst), _p(ws), ws.numel(),
                                 _stream())
    check(st, "ddmp_gat_datt_f32")
    return datt_src, datt_dst


# ---------------------------------------------------------------------------------------- dynamic graph attention
def gatv2_fwd(g: Graph, xl, xr, att, heads, slope, bias=None, out=None):
    """Per-edge scores + edge softmax + gather in one launch (``ddmp_gatv2_fwd_f32``) -> (y [n, heads * C], alpha [g.nnz, heads]).
    ``xl`` / ``xr``: [n, heads * C] (column blocks of one row buffer, or the same tensor twice); ``att``: [heads, C]; ``bias``:
    float32 [heads * C] added in the epilogue, or None."""
    n, C, m = _head_mats(g, heads, "gatv2_fwd", xl=xl, xr=xr)
    (xl, ldl), (xr, ldr) = m["xl"], m["xr"]
    att = _gat_arr(att, (heads, C), "att")
    if bias is not None:
        bias = _gat_arr(bias, (heads * C,), "bias")
    out, ldy = _out(out, "out", n, heads * C, xl.device)
    alpha = torch.empty((g.nnz, heads), dtype=torch.float32, device=xl.device)
    # algorithmic bytes: xl and xr read once each, y written, alpha written, col + multiplicity, rowptr, att
    alg = 12.0 * n * heads * C + 4.0 * g.nnz * heads + 8.0 * g.nnz + 4.0 * (n + 1) + 4.0 * heads * C
    with _timed("gatv2_fwd", _gat_key(g, heads, C), alg, 6.0 * g.nnz * heads * C):
        st = _lib.lib().ddmp_gatv2_fwd_f32(g.handle, _p(xl), ldl, _p(xr), ldr, heads, C, _p(att), float(slope), _p(bias), _p(alpha),
                                           _p(out), ldy, _stream())
    check(st, "ddmp_gatv2_fwd_f32")
    return out, alpha


def gatv2_bwd_edge(g: Graph, dout, xl, xr, att, alpha, heads, slope, out=None, want_datt=True):
    """Row i's side of the backward (``ddmp_gatv2_bwd_edge_f32``) -> (dz [g.nnz, heads], dxr [n, heads * C] written completely,
    part [n, heads * C] | None: the rows' shares of datt, for ``gatv2_datt``).  ``out``: where dxr goes (a column block of a row
    buffer is fine)."""
    n, C, m = _head_mats(g, heads, "gatv2_bwd_edge", xl=xl, xr=xr, dout=dout)
    (xl, ldl), (xr, ldr), (dout, lddo) = m["xl"], m["xr"], m["dout"]
    att, alpha = _gat_arr(att, (heads, C), "att"), _gat_arr(alpha, (g.nnz, heads), "alpha")
    out, lddr = _out(out, "out", n, heads * C, xl.device)
    dz = torch.empty((g.nnz, heads), dtype=torch.float32, device=xl.device)
    part = torch.empty((n, heads * C), dtype=torch.float32, device=xl.device) if want_datt else None
    # algorithmic bytes: dout, xl and xr read once each, dxr (and part) written, alpha read, dz written, col, rowptr, att
    alg = (20.0 if want_datt else 16.0) * n * heads * C + 8.0 * g.nnz * heads + 4.0 * g.nnz + 4.0 * (n + 1) + 4.0 * heads * C
    with _timed("gatv2_bwd_edge", _gat_key(g, heads, C), alg, 8.0 * g.nnz * heads * C):
        st = _lib.lib().ddmp_gatv2_bwd_edge_f32(g.handle, _p(dout), lddo, _p(xl), ldl, _p(xr), ldr, heads, C, _p(att), float(slope),
                                                _p(alpha), _p(dz), _p(out), lddr, _p(part), heads * C, _stream())
    check(st, "ddmp_gatv2_bwd_edge_f32")
    return dz, out, part


def gatv2_bwd_node(g: Graph, dout, xl, xr, att, alpha, dz, heads, slope, out=None):
    """Node j's side of the backward (``ddmp_gatv2_bwd_node_f32``) -> dxl [n, heads * C] written completely.  ``out``: where it
    goes (a column block of a row buffer is fine)."""
    n, C, m = _head_mats(g, heads, "gatv2_bwd_node", xl=xl, xr=xr, dout=dout)
    (xl, ldl), (xr, ldr), (dout, lddo) = m["xl"], m["xr"], m["dout"]
    att = _gat_arr(att, (heads, C), "att")
    alpha, dz = _gat_arr(alpha, (g.nnz, heads), "alpha"), _gat_arr(dz, (g.nnz, heads), "dz")
    out, lddl = _out(out, "out", n, heads * C, xl.device)
    # algorithmic bytes: dout, xr and xl read once each, dxl written, alpha and dz read through the mirror map, col + mirror, rowptr
    alg = 16.0 * n * heads * C + 8.0 * g.nnz * heads + 8.0 * g.nnz + 4.0 * (n + 1) + 4.0 * heads * C
    with _timed("gatv2_bwd_node", _gat_key(g, heads, C), alg, 6.0 * g.nnz * heads * C):
        st = _lib.lib().ddmp_gatv2_bwd_node_f32(g.handle, _p(dout), lddo, _p(xl), ldl, _p(xr), ldr, heads, C, _p(att), float(slope),
                                                _p(alpha), _p(dz), _p(out), lddl, _stream())
    check(st, "ddmp_gatv2_bwd_node_f32")
    return out


def gatv2_datt(part, heads):
    """-> datt [heads, C]: the column sum of the rows' shares ``part`` [n, heads * C] (``ddmp_gatv2_datt_f32``: two-stage column
    reduction, per-chunk partials in the workspace, fixed order)."""
    part, ldp, C = _gat_hf(part, heads, "part")
    n = part.shape[0]
    L = _lib.lib()
    need = L.ddmp_gatv2_datt_workspace_bytes(n, heads, C)
    ws = Workspace.get(need, part.device)
    datt = torch.empty((heads, C), dtype=torch.float32, device=part.device)
    with _timed("gatv2_datt", (heads, C), 4.0 * n * heads * C + 2.0 * need, 1.0 * n * heads * C):
        st = L.ddmp_gatv2_datt_f32(_p(part), ldp, n, heads, C, _p(datt), _p(ws), ws.numel(), _stream())
    check(st, "ddmp_gatv2_datt_f32")
    return datt


# ---------------------------------------------------------------------------------------- graph transformer
def tconv_fwd(g: Graph, q, k, v, heads, scale=None, skip=None, out=None):
    """Dot-product scores + edge softmax + gather in one launch (``ddmp_tconv_fwd_f32``) -> (y [n, heads * C], alpha [g.nnz,
    heads]).  ``q`` / ``k`` / ``v``: [n, heads * C] (column blocks of one row buffer are fine; ``k`` and ``v`` may be the same
    tensor); ``scale``: the factor on q . k, default 1 / sqrt(C); ``skip``: [n, heads * C] added in the epilogue, or None."""
    mats = dict(q=q, k=k, v=v) if skip is None else dict(q=q, k=k, v=v, skip=skip)
    n, C, m = _head_mats(g, heads, "tconv_fwd", **mats)
    (q, ldq), (k, ldk), (v, ldv) = m["q"], m["k"], m["v"]
    skip, lds = m.get("skip", (None, 0))
    scale = 1.0 / math.sqrt(C) if scale is None else float(scale)
    out, ldy = _out(out, "out", n, heads * C, q.device)
    alpha = torch.empty((g.nnz, heads), dtype=torch.float32, device=q.device)
    # algorithmic bytes: q, k and v (and the skip) read once each, y written, alpha written, col + multiplicity, rowptr
    alg = (16.0 if skip is None else 20.0) * n * heads * C + 4.0 * g.nnz * heads + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("tconv_fwd", _gat_key(g, heads, C), alg, 4.0 * g.nnz * heads * C):
        st = _lib.lib().ddmp_tconv_fwd_f32(g.handle, _p(q), ldq, _p(k), ldk, _p(v), ldv, heads, C, scale, _p(skip), lds, _p(alpha),
                                           _p(out), ldy, _stream())
    check(st, "ddmp_tconv_fwd_f32")
    return out, alpha


def tconv_bwd_edge(g: Graph, dout, k, v, alpha, heads, scale=None, out=None):
    """Row i's side of the backward (``ddmp_tconv_bwd_edge_f32``) -> (dz [g.nnz, heads], dq [n, heads * C] written completely).
    ``out``: where dq goes (a column block of a row buffer is fine)."""
    n, C, m = _head_mats(g, heads, "tconv_bwd_edge", dout=dout, k=k, v=v)
    (dout, lddo), (k, ldk), (v, ldv) = m["dout"], m["k"], m["v"]
    scale = 1.0 / math.sqrt(C) if scale is None else float(scale)
    alpha = _gat_arr(alpha, (g.nnz, heads), "alpha")
    out, lddq = _out(out, "out", n, heads * C, k.device)
    dz = torch.empty((g.nnz, heads), dtype=torch.float32, device=k.device)
    # algorithmic bytes: dout, k and v read once each, dq written, alpha read, dz written, col, rowptr
    alg = 16.0 * n * heads * C + 8.0 * g.nnz * heads + 4.0 * g.nnz + 4.0 * (n + 1)
    with _timed("tconv_bwd_edge", _gat_key(g, heads, C), alg, 4.0 * g.nnz * heads * C):
        st = _lib.lib().ddmp_tconv_bwd_edge_f32(g.handle, _p(dout), lddo, _p(k), ldk, _p(v), ldv, heads, C, scale, _p(alpha), _p(dz),
                                                _p(out), lddq, _stream())
    check(st, "ddmp_tconv_bwd_edge_f32")
    return dz, out


def tconv_bwd_node(g: Graph, dout, q, alpha, dz, heads, scale=None, out_k=None, out_v=None, out_s=None):
    """Node j's side of the backward (``ddmp_tconv_bwd_node_f32``) -> (dk, dv) [n, heads * C] each, written completely.
    ``out_k`` / ``out_v``: where they go; ``out_s``: a [n, heads * C] block that also receives a copy of ``dout`` (the skip
    term's gradient), or None.  Column blocks of one row buffer are fine."""
    n, C, m = _head_mats(g, heads, "tconv_bwd_node", dout=dout, q=q)
    (dout, lddo), (q, ldq) = m["dout"], m["q"]
    scale = 1.0 / math.sqrt(C) if scale is None else float(scale)
    alpha, dz = _gat_arr(alpha, (g.nnz, heads), "alpha"), _gat_arr(dz, (g.nnz, heads), "dz")
    out_k, lddk = _out(out_k, "out_k", n, heads * C, q.device)
    out_v, lddv = _out(out_v, "out_v", n, heads * C, q.device)
    ldds = 0
    if out_s is not None:
        out_s, ldds = _out(out_s, "out_s", n, heads * C, q.device)
    # algorithmic bytes: dout and q read once each, dk and dv (and ds) written, alpha and dz read through the mirror map,
    # col + mirror, rowptr
    alg = (16.0 if out_s is None else 20.0) * n * heads * C + 8.0 * g.nnz * heads + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("tconv_bwd_node", _gat_key(g, heads, C), alg, 4.0 * g.nnz * heads * C):
        st = _lib.lib().ddmp_tconv_bwd_node_f32(g.handle, _p(dout), lddo, _p(q), ldq, heads, C, scale, _p(alpha), _p(dz), _p(out_k),
                                                lddk, _p(out_v), lddv, _p(out_s), ldds, _stream())
    check(st, "ddmp_tconv_bwd_node_f32")
    return out_k, out_v


# ---------------------------------------------------------------------------------------- residual gated graph conv
def _rgate_key(g, C):
    return (C, int(round(g.nnz / max(g.n_rows, 1))))


def rgate_fwd(g: Graph, k, q, v, skip=None, bias=None, out=None):
    """Per-channel sigmoid gate + gather in one launch (``ddmp_rgate_fwd_f32``) -> y [n, C]:
    ``y[i] = skip[i] + bias + sum_{e in row i} a_e sigmoid(k[i] + q[col e]) * v[col e]``.  ``k`` / ``q`` / ``v``: [n, C] (column
    blocks of one row buffer are fine); ``skip``: [n, C] and ``bias``: float32 [C], each added in the epilogue, or None.  Nothing
    is kept per entry."""
    mats = dict(k=k, q=q, v=v) if skip is None else dict(k=k, q=q, v=v, skip=skip)
    n, C, m = _head_mats(g, 1, "rgate_fwd", **mats)
    (k, ldk), (q, ldq), (v, ldv) = m["k"], m["q"], m["v"]
    skip, lds = m.get("skip", (None, 0))
    if bias is not None:
        bias = _gat_arr(bias, (C,), "bias")
    out, ldy = _out(out, "out", n, C, k.device)
    # algorithmic bytes: k, q and v (and the skip) read once each, y written, col + multiplicity, rowptr, bias
    alg = (16.0 if skip is None else 20.0) * n * C + 8.0 * g.nnz + 4.0 * (n + 1) + (0.0 if bias is None else 4.0 * C)
    with _timed("rgate_fwd", _rgate_key(g, C), alg, 6.0 * g.nnz * C):
        st = _lib.lib().ddmp_rgate_fwd_f32(g.handle, _p(k), ldk, _p(q), ldq, _p(v), ldv, C, _p(skip), lds, _p(bias), _p(out), ldy,
                                           _stream())
    check(st, "ddmp_rgate_fwd_f32")
    return out


def rgate_bwd_row(g: Graph, dout, k, q, v, out=None):
    """Row i's side of the backward (``ddmp_rgate_bwd_row_f32``) -> dk [n, C] written completely; the gate is recomputed.
    ``out``: where dk goes (a column block of a row buffer is fine)."""
    n, C, m = _head_mats(g, 1, "rgate_bwd_row", dout=dout, k=k, q=q, v=v)
    (dout, lddo), (k, ldk), (q, ldq), (v, ldv) = m["dout"], m["k"], m["q"], m["v"]
    out, lddk = _out(out, "out", n, C, k.device)
    # algorithmic bytes: dout, k, q and v read once each, dk written, col + multiplicity, rowptr
    alg = 20.0 * n * C + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("rgate_bwd_row", _rgate_key(g, C), alg, 9.0 * g.nnz * C):
        st = _lib.lib().ddmp_rgate_bwd_row_f32(g.handle, _p(dout), lddo, _p(k), ldk, _p(q), ldq, _p(v), ldv, C, _p(out), lddk,
                                               _stream())
    check(st, "ddmp_rgate_bwd_row_f32")
    return out


def rgate_bwd_node(g: Graph, dout, k, q, v, out_q=None, out_v=None, out_s=None):
    """Node j's side of the backward (``ddmp_rgate_bwd_node_f32``) -> (dq, dv) [n, C] each, written completely; the gate is
    recomputed and the multiplicities are read through the mirror map.  ``out_q`` / ``out_v``: where they go; ``out_s``: a [n, C]
    block that also receives a copy of ``dout`` (the skip term's gradient), or None.  Column blocks of one row buffer are fine."""
    n, C, m = _head_mats(g, 1, "rgate_bwd_node", dout=dout, k=k, q=q, v=v)
    (dout, lddo), (k, ldk), (q, ldq), (v, ldv) = m["dout"], m["k"], m["q"], m["v"]
    out_q, lddq = _out(out_q, "out_q", n, C, q.device)
    out_v, lddv = _out(out_v, "out_v", n, C, q.device)
    ldds = 0
    if out_s is not None:
        out_s, ldds = _out(out_s, "out_s", n, C, q.device)
    # algorithmic bytes: dout, k, q and v read once each, dq and dv (and ds) written, col + mirror + multiplicity, rowptr
    alg = (24.0 if out_s is None else 28.0) * n * C + 12.0 * g.nnz + 4.0 * (n + 1)
    with _timed("rgate_bwd_node", _rgate_key(g, C), alg, 10.0 * g.nnz * C):
        st = _lib.lib().ddmp_rgate_bwd_node_f32(g.handle, _p(dout), lddo, _p(k), ldk, _p(q), ldq, _p(v), ldv, C, _p(out_q), lddq,
                                                _p(out_v), lddv, _p(out_s), ldds, _stream())
    check(st, "ddmp_rgate_bwd_node_f32")
    return out_q, out_v


# ---------------------------------------------------------------------------------------- feature-steered convolution
def feast_fwd(g: Graph, hf, p, c, heads, bias=None, out=None):
    """Head softmax + gather in one launch (``ddmp_feast_fwd_f32``) -> (y [n, C], beta [g.nnz, heads]).  ``hf``: [n, heads * C],
    ``p``: [n, heads] (both may be column blocks of one row buffer), ``c``: [heads], ``bias``: float32 [C] or None."""
    _gat_graph(g)
    n = g.n_rows
    hf, ldh, C = _gat_hf(hf, heads, "hf", n)
    p, ldp = _rows(p, "p", n, heads)
    c = _gat_arr(c, (heads,), "c")
    if bias is not None:
        bias = _gat_arr(bias, (C,), "bias")
    out, ldy = _out(out, "out", n, C, hf.device)
    beta = torch.empty((g.nnz, heads), dtype=torch.float32, device=hf.device)
    # algorithmic bytes: every gathered row (heads * C wide) read once, the output row (C wide) written once, beta written, p read
    # once, col + multiplicity, rowptr
    alg = 4.0 * n * (heads + 1) * C + 4.0 * g.nnz * heads + 4.0 * n * heads + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("feast_fwd", _gat_key(g, heads, C), alg, 2.0 * g.nnz * heads * C,
                survey=4.0 * n * (heads + 1) * C + 4.0 * g.nnz + 4.0 * (n + 1)):
        st = _lib.lib().ddmp_feast_fwd_f32(g.handle, _p(hf), ldh, _p(p), ldp, heads, C, _p(c), _p(bias), _p(beta), _p(out), ldy,
                                           _stream())
    check(st, "ddmp_feast_fwd_f32")
    return out, beta


def feast_bwd_edge(g: Graph, dout, hf, beta, heads):
    """Edge side of the backward (``ddmp_feast_bwd_edge_f32``) -> (dz [g.nnz, heads], rs [n, heads]).  ``dout``: [n, C]."""
    _gat_graph(g)
    n = g.n_rows
    hf, ldh, C = _gat_hf(hf, heads, "hf", n)
    dout, lddo = _rows(dout, "dout", n, C)
    beta = _gat_arr(beta, (g.nnz, heads), "beta")
    dz = torch.empty((g.nnz, heads), dtype=torch.float32, device=hf.device)
    rs = torch.empty((n, heads), dtype=torch.float32, device=hf.device)
    # algorithmic bytes: hf and dout read once each, beta read, dz written, rs written, col, rowptr
    alg = 4.0 * n * (heads + 1) * C + 8.0 * g.nnz * heads + 4.0 * n * heads + 4.0 * g.nnz + 4.0 * (n + 1)
    with _timed("feast_bwd_edge", _gat_key(g, heads, C), alg, 2.0 * g.nnz * heads * C):
        st = _lib.lib().ddmp_feast_bwd_edge_f32(g.handle, _p(dout), lddo, _p(hf), ldh, heads, C, _p(beta), _p(dz), _p(rs), _stream())
    check(st, "ddmp_feast_bwd_edge_f32")
    return dz, rs


def feast_bwd_node(g: Graph, dout, beta, dz, rs, heads, out=None):
    """Node side of the backward (``ddmp_feast_bwd_node_f32``) -> (dhf [n, heads * C] written completely, dp [n, heads]).
    ``out``: a float32 [n, >= heads * C + heads] row buffer that receives [dhf | dp] in its leading columns (the two results are
    then views of it); None: two tensors of their own."""
    _gat_graph(g)
    n = g.n_rows
    dout, lddo = _rows(dout, "dout", n)
    C = dout.shape[1]
    beta, dz = _gat_arr(beta, (g.nnz, heads), "beta"), _gat_arr(dz, (g.nnz, heads), "dz")
    rs = _gat_arr(rs, (n, heads), "rs")
    hc = heads * C
    if out is None:
        dhf = torch.empty((n, hc), dtype=torch.float32, device=dout.device)
        dp = torch.empty((n, heads), dtype=torch.float32, device=dout.device)
    else:
        out, _ = _mat(_chk(out, torch.float32, "out"), "out")
        if out.shape[0] != n or out.shape[1] < hc + heads:
            raise DdmpError("feast_bwd_node: out must be [%d, >= %d], got %s" % (n, hc + heads, tuple(out.shape)))
        dhf, dp = out[:, :hc], out[:, hc:hc + heads]
    (dhf, lddh), (dp, lddp) = _mat(dhf, "dhf"), _mat(dp, "dp")
    # algorithmic bytes: dout read once, dhf written, beta and dz read through the mirror map, col + mirror, rs read, dp written, rowptr
    alg = 4.0 * n * (heads + 1) * C + 8.0 * g.nnz * heads + 8.0 * n * heads + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("feast_bwd_node", _gat_key(g, heads, C), alg, 2.0 * g.nnz * heads * C):
        st = _lib.lib().ddmp_feast_bwd_node_f32(g.handle, _p(dout), lddo, heads, C, _p(beta), _p(dz), _p(rs), _p(dhf), lddh, _p(dp),
                                                lddp, _stream())
    check(st, "ddmp_feast_bwd_node_f32")
    return dhf, dp


def feast_dc(rs, heads):
    """-> dc [heads]: dc[h] = sum_i rs[i, h] (``ddmp_feast_dc_f32``: two-stage column reduction, per-chunk partials in the
    workspace, fixed order).  ``colsum`` takes power-of-two widths from 8 on a 4-aligned leading dimension; the head counts in use
    (1, 2, 3, 4, 8) almost never qualify, so every head count takes this one path."""
    _chk(rs, torch.float32, "rs")
    if rs.dim() != 2 or rs.shape[1] != heads or not rs.is_contiguous() or rs.shape[0] < 1:
        raise DdmpError("rs must be a contiguous float32 [n >= 1, %d], got %s" % (heads, tuple(rs.shape)))
    n = rs.shape[0]
    L = _lib.lib()
    need = L.ddmp_feast_dc_workspace_bytes(n, heads)
    ws = Workspace.get(need, rs.device)
    dc = torch.empty(heads, dtype=torch.float32, device=rs.device)
    with _timed("feast_dc", (heads,), 4.0 * n * heads + 2.0 * need, 1.0 * n * heads):
        st = L.ddmp_feast_dc_f32(_p(rs), n, heads, _p(dc), _p(ws), ws.numel(), _stream())
    check(st, "ddmp_feast_dc_f32")
    return dc


# ---------------------------------------------------------------------------------------- Gaussian-mixture convolution
GMM_MAX_KD = 128            # K * dim: the [n, 2 K dim] partials of the edge-side backward go through feast_dc (<= 256 columns)


def _gmm_graph(g: Graph):
    _gat_graph(g)
    if g.valued != GV_VALUED:
        raise DdmpError("the Gaussian-mixture kernels need the graph of graph_for(edge_index, n, norm='gat', add_self_loops=False): "
                        "every input edge must belong to exactly one entry")
    return g


def _gmm_params(g, attr, mu, sigma, K):
    """-> (attr, mu, sigma, dim) checked: attr contiguous float32 [g.nnz_in, dim], mu / sigma contiguous float32 [K, dim]."""
    _chk(attr, torch.float32, "attr")
    if attr.dim() != 2 or attr.shape[0] != g.nnz_in or attr.shape[1] < 1 or not attr.is_contiguous():
        raise DdmpError("attr must be a contiguous float32 [%d, dim] (one row per input edge), got %s" % (g.nnz_in, tuple(attr.shape)))
    dim = attr.shape[1]
    if K < 1 or K * dim > GMM_MAX_KD:
        raise DdmpError("K (%d) x dim (%d) must be in [1, %d]" % (K, dim, GMM_MAX_KD))
    return attr, _gat_arr(mu, (K, dim), "mu"), _gat_arr(sigma, (K, dim), "sigma"), dim


def gmm_fwd(g: Graph, hf, attr, mu, sigma, K, root=None, bias=None, out=None):
    """Per-edge Gaussians + gather in one launch (``ddmp_gmm_fwd_f32``) -> (y [n, C], w [g.nnz, K]).  ``hf``: [n, K * C], ``root``:
    [n, C] added per row or None (both may be column blocks of one row buffer), ``attr``: [g.nnz_in, dim] pseudo-coordinates of
    the input edges, ``mu`` / ``sigma``: [K, dim], ``bias``: float32 [C] or None."""
    _gmm_graph(g)
    n = g.n_rows
    hf, ldh, C = _gat_hf(hf, K, "hf", n)
    attr, mu, sigma, dim = _gmm_params(g, attr, mu, sigma, K)
    ldr = 0
    if root is not None:
        root, ldr = _rows(root, "root", n, C)
    if bias is not None:
        bias = _gat_arr(bias, (C,), "bias")
    out, ldy = _out(out, "out", n, C, hf.device)
    w = torch.empty((g.nnz, K), dtype=torch.float32, device=hf.device)
    # algorithmic bytes: every gathered row (K * C wide) read once, the output row (C wide) written once, the root block read, w
    # written, the attribute rows read once, col + multiplicity + ee_ptr, ee_idx, rowptr
    alg = (4.0 * n * (K + 1 + (root is not None)) * C + 4.0 * g.nnz * K + 4.0 * g.nnz_in * (dim + 1) + 12.0 * g.nnz + 4.0 * (n + 1))
    with _timed("gmm_fwd", _gat_key(g, K, C) + (dim,), alg, 2.0 * g.nnz * K * C,
                survey=4.0 * n * (K + 1) * C + 4.0 * g.nnz + 4.0 * (n + 1)):
        st = _lib.lib().ddmp_gmm_fwd_f32(g.handle, _p(hf), ldh, _p(attr), dim, _p(mu), _p(sigma), K, C, _p(root), ldr, _p(bias),
                                         _p(w), _p(out), ldy, _stream())
    check(st, "ddmp_gmm_fwd_f32")
    return out, w


def gmm_bwd_edge(g: Graph, dout, hf, attr, mu, sigma, K, want_dattr=False):
    """Edge side of the backward (``ddmp_gmm_bwd_edge_f32``) -> (parts [n, 2 * K * dim], dattr [g.nnz_in, dim] | None).  The column
    sums of ``parts`` (``feast_dc(parts, 2 * K * dim)``) are [dmu | dsigma], each [K, dim] flattened.  ``dout``: [n, C]."""
    _gmm_graph(g)
    n = g.n_rows
    hf, ldh, C = _gat_hf(hf, K, "hf", n)
    dout, lddo = _rows(dout, "dout", n, C)
    attr, mu, sigma, dim = _gmm_params(g, attr, mu, sigma, K)
    ge = torch.empty((g.nnz, K), dtype=torch.float32, device=hf.device)
    parts = torch.empty((n, 2 * K * dim), dtype=torch.float32, device=hf.device)
    dattr = torch.empty((g.nnz_in, dim), dtype=torch.float32, device=hf.device) if want_dattr else None
    # algorithmic bytes: hf and dout read once each, the dot products written and read back, the attribute rows read (and their
    # gradient written), the partials written, col + multiplicity + ee_ptr, ee_idx, rowptr
    alg = (4.0 * n * (K + 1) * C + 8.0 * g.nnz * K + 4.0 * g.nnz_in * (dim * (2 if want_dattr else 1) + 1) + 8.0 * n * K * dim
           + 12.0 * g.nnz + 4.0 * (n + 1))
    with _timed("gmm_bwd_edge", _gat_key(g, K, C) + (dim,), alg, 2.0 * g.nnz * K * C):
        st = _lib.lib().ddmp_gmm_bwd_edge_f32(g.handle, _p(dout), lddo, _p(hf), ldh, _p(attr), dim, _p(mu), _p(sigma), K, C, _p(ge),
                                              _p(parts), _p(dattr), _stream())
    check(st, "ddmp_gmm_bwd_edge_f32")
    return parts, dattr


def gmm_bwd_node(g: Graph, dout, w, K, out=None, root=False):
    """Node side of the backward (``ddmp_gmm_bwd_node_f32``) -> (dhf [n, K * C] written completely, droot [n, C] | None): with
    ``root`` the launch also copies ``dout`` into the root block's columns.  ``out``: a float32 [n, >= K * C (+ C)] row buffer that
    receives [dhf | droot] in its leading columns (the results are then views of it; further columns are left untouched); None: a
    buffer of its own."""
    _gmm_graph(g)
    n = g.n_rows
    dout, lddo = _rows(dout, "dout", n)
    C = dout.shape[1]
    w = _gat_arr(w, (g.nnz, K), "w")
    (dhf, lddh), (dr, lddr) = _out_with_root(out, "gmm_bwd_node", n, K * C, C, root, dout.device)
    # algorithmic bytes: dout read once, dhf (and the root block) written, w read through the mirror map, col + mirror, rowptr
    alg = 4.0 * n * (K + 1 + bool(root)) * C + 4.0 * g.nnz * K + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("gmm_bwd_node", _gat_key(g, K, C), alg, 2.0 * g.nnz * K * C):
        st = _lib.lib().ddmp_gmm_bwd_node_f32(g.handle, _p(dout), lddo, K, C, _p(w), _p(dhf), lddh, _p(dr), lddr, _stream())
    check(st, "ddmp_gmm_bwd_node_f32")
    return dhf, dr


# ---------------------------------------------------------------------------------------- B-spline convolution
SPLINE_MAX_DIM = 5          # S = 2^dim <= 32 selected blocks per edge


def _spline_params(g, attr, kernel_size, is_open, C):
    """-> (attr, ks, op, dim, K, S) checked: attr contiguous float32 [g.nnz_in, dim], ``kernel_size`` / ``is_open`` sequences of
    dim ints >= 1 / bools as ctypes int32 arrays (host), K = prod(kernel_size), S = 2^dim."""
    _chk(attr, torch.float32, "attr")
    if attr.dim() != 2 or attr.shape[0] != g.nnz_in or attr.shape[1] < 1 or not attr.is_contiguous():
        raise DdmpError("attr must be a contiguous float32 [%d, dim] (one row per input edge), got %s" % (g.nnz_in, tuple(attr.shape)))
    dim = attr.shape[1]
    kernel_size, is_open = [int(k) for k in kernel_size], [int(bool(o)) for o in is_open]
    if not 1 <= dim <= SPLINE_MAX_DIM or len(kernel_size) != dim or len(is_open) != dim or min(kernel_size) < 1:
        raise DdmpError("kernel_size and is_open must have dim (%d, in [1, %d]) entries, every kernel_size >= 1; got %r, %r"
                        % (dim, SPLINE_MAX_DIM, kernel_size, is_open))
    K = math.prod(kernel_size)
    if K * C >= 1 << 24:
        raise DdmpError("prod(kernel_size) (%d) x C (%d) must be below 2^24" % (K, C))
    i32 = ctypes.c_int32 * dim
    return attr, i32(*kernel_size), i32(*is_open), dim, K, 1 << dim


def spline_fwd(g: Graph, hf, attr, kernel_size, is_open, root=None, bias=None, mean=True, out=None):
    """B-spline basis + block gather in one launch (``ddmp_spline_fwd_f32``) -> y [n, C].  ``hf``: [n, K * C] with
    K = prod(kernel_size) blocks (the first coordinate varies fastest), ``root``: [n, C] added per row or None (both may be column
    blocks of one row buffer), ``attr``: [g.nnz_in, dim] pseudo-coordinates of the input edges, ``kernel_size`` / ``is_open``:
    dim ints / bools, ``bias``: float32 [C] or None, ``mean``: divide a row's sum by its number of input edges."""
    _gmm_graph(g)
    n = g.n_rows
    K = math.prod(int(k) for k in kernel_size)
    hf, ldh, C = _gat_hf(hf, K, "hf", n)
    attr, ks, op, dim, K, S = _spline_params(g, attr, kernel_size, is_open, C)
    ldr = 0
    if root is not None:
        root, ldr = _rows(root, "root", n, C)
    if bias is not None:
        bias = _gat_arr(bias, (C,), "bias")
    out, ldy = _out(out, "out", n, C, hf.device)
    # algorithmic bytes: the S selected blocks (C wide) of the neighbour's row per input edge -- not its K blocks --, the output row
    # written once, the root block read, the attribute rows read once, col + ee_ptr, ee_idx, rowptr
    alg = (4.0 * g.nnz_in * S * C + 4.0 * n * (1 + (root is not None)) * C + 4.0 * g.nnz_in * (dim + 1) + 8.0 * g.nnz
           + 4.0 * (n + 1))
    with _timed("spline_fwd", _gat_key(g, K, C) + (dim,), alg, 2.0 * g.nnz_in * S * C):
        st = _lib.lib().ddmp_spline_fwd_f32(g.handle, _p(hf), ldh, _p(attr), dim, ks, op, C, _p(root), ldr, _p(bias), int(bool(mean)),
                                            _p(out), ldy, _stream())
    check(st, "ddmp_spline_fwd_f32")
    return out


def spline_bwd_node(g: Graph, dout, attr, kernel_size, is_open, C, mean=True, out=None, root=False):
    """The backward of the graph part in one launch (``ddmp_spline_bwd_node_f32``) -> (dhf [n, K * C] written completely -- blocks
    no edge selects are zero --, droot [n, C] | None): with ``root`` the launch also copies ``dout`` into the root block's columns.
    ``dout``: [n, C]; ``out``: a float32 [n, >= K * C (+ C)] row buffer that receives [dhf | droot] in its leading columns (the
    results are then views of it; further columns are left untouched); None: a buffer of its own."""
    _gmm_graph(g)
    n = g.n_rows
    dout, lddo = _rows(dout, "dout", n, C)
    attr, ks, op, dim, K, S = _spline_params(g, attr, kernel_size, is_open, C)
    (dhf, lddh), (dr, lddr) = _out_with_root(out, "spline_bwd_node", n, K * C, C, root, dout.device)
    # algorithmic bytes: dhf (and the root block) written once, dout read once (and once more for the root block), the attribute
    # rows read once, col + mirror + ee_ptr, ee_idx, rowptr; the S read-modify-writes per edge stay in the row's own cache lines
    alg = 4.0 * n * (K + 1 + 2 * bool(root)) * C + 4.0 * g.nnz_in * (dim + 1) + 12.0 * g.nnz + 4.0 * (n + 1)
    with _timed("spline_bwd_node", _gat_key(g, K, C) + (dim,), alg, 2.0 * g.nnz_in * S * C):
        st = _lib.lib().ddmp_spline_bwd_node_f32(g.handle, _p(dout), lddo, _p(attr), dim, ks, op, C, int(bool(mean)), _p(dhf), lddh,
                                                 _p(dr), lddr, _stream())
    check(st, "ddmp_spline_bwd_node_f32")
    return dhf, dr


# ---------------------------------------------------------------------------------------- crystal graph convolution
CG_MAX_DIM = 8              # attribute coordinates per edge: the 2 dim float4 of Ef / Es of a column slab stay in registers


def _cgate_operands(g, who, attr, ef, es, **mats):
    """The operands every crystal-gate call shares -> (n, C, {name: (tensor, ld)}, attr, ef, es, dim): the [n, C] row blocks by
    name (column blocks of one row buffer are fine), ``attr`` contiguous float32 [g.nnz_in, dim] and ``ef`` / ``es`` contiguous
    float32 [dim, C] (the edge weights TRANSPOSED) -- or all three None: dim = 0, the entries count with their multiplicities."""
    n, C, m = _head_mats(g, 1, who, **mats)
    if attr is None:
        if ef is not None or es is not None:
            raise DdmpError("%s: ef / es without attr (dim == 0 takes neither)" % who)
        return n, C, m, None, None, None, 0
    _gmm_graph(g)
    _chk(attr, torch.float32, "attr")
    if attr.dim() != 2 or attr.shape[0] != g.nnz_in or not attr.is_contiguous() or not 1 <= attr.shape[1] <= CG_MAX_DIM:
        raise DdmpError("attr must be a contiguous float32 [%d, dim] (one row per input edge) with dim in [1, %d], got %s"
                        % (g.nnz_in, CG_MAX_DIM, tuple(attr.shape)))
    dim = attr.shape[1]
    return n, C, m, attr, _gat_arr(ef, (dim, C), "ef"), _gat_arr(es, (dim, C), "es"), dim


def _cgate_key(g, C, dim):
    return (C, dim, int(round(g.nnz / max(g.n_rows, 1))))


def _cgate_graph_bytes(g, n, C, dim, mirror=False):
    """col (+ mirror), rowptr and: the multiplicities (dim == 0) | ee_ptr, ee_idx, the attribute rows and Ef / Es (dim > 0)."""
    b = (8.0 if mirror else 4.0) * g.nnz + 4.0 * (n + 1)
    return b + (4.0 * g.nnz if dim == 0 else 4.0 * g.nnz + 4.0 * g.nnz_in * (dim + 1) + 8.0 * dim * C)


def cgate_fwd(g: Graph, af, as_, bf, bs, attr=None, ef=None, es=None, root=None, mean=False, out=None):
    """Two per-channel gates + gather in one launch (``ddmp_cgate_fwd_f32``) -> y [n, C]:
    ``y[i] = root[i] + w_i sum_{t: j -> i} sigmoid(af[i] + bf[j] + ef^T a_t) * softplus(as_[i] + bs[j] + es^T a_t)``, ``w_i`` = 1 or
    (``mean``) 1 / the number of input edges into i.  ``af`` / ``as_`` / ``bf`` / ``bs``: [n, C] (column blocks of one row buffer
    are fine); ``attr``: contiguous float32 [g.nnz_in, dim] with ``ef`` / ``es`` [dim, C], or all None (dim = 0); ``root``: [n, C]
    added per row, or None.  Nothing is kept per edge."""
    mats = dict(af=af, as_=as_, bf=bf, bs=bs) if root is None else dict(af=af, as_=as_, bf=bf, bs=bs, root=root)
    n, C, m, attr, ef, es, dim = _cgate_operands(g, "cgate_fwd", attr, ef, es, **mats)
    (af, ldaf), (as_, ldas), (bf, ldbf), (bs, ldbs) = m["af"], m["as_"], m["bf"], m["bs"]
    root, ldr = m.get("root", (None, 0))
    out, ldy = _out(out, "out", n, C, af.device)
    # algorithmic bytes: the four blocks (and the root) read once each, y written, the graph and the attributes
    alg = (20.0 if root is None else 24.0) * n * C + _cgate_graph_bytes(g, n, C, dim)
    with _timed("cgate_fwd", _cgate_key(g, C, dim), alg, (4.0 * dim + 30.0) * max(g.nnz, g.nnz_in) * C):
        st = _lib.lib().ddmp_cgate_fwd_f32(g.handle, _p(af), ldaf, _p(as_), ldas, _p(bf), ldbf, _p(bs), ldbs, C, _p(attr), dim,
                                           _p(ef), _p(es), _p(root), ldr, int(bool(mean)), _p(out), ldy, _stream())
    check(st, "ddmp_cgate_fwd_f32")
    return out


def cgate_bwd_row(g: Graph, dout, af, as_, bf, bs, attr=None, ef=None, es=None, mean=False, out_f=None, out_s=None, want_parts=True):
    """Row i's side of the backward (``ddmp_cgate_bwd_row_f32``) -> (daf, das [n, C] each, written completely, parts | None);
    both gates are recomputed.  ``parts`` (dim > 0 and ``want_parts``): the rows' shares of the edge weights' gradient,
    [n, 2 * dim * C]; their column sum (``gatv2_datt(parts, 2 * dim)``) is [def ; des], [dim, C] each.  ``out_f`` / ``out_s``: where
    daf / das go (column blocks of a row buffer are fine)."""
    n, C, m, attr, ef, es, dim = _cgate_operands(g, "cgate_bwd_row", attr, ef, es, dout=dout, af=af, as_=as_, bf=bf, bs=bs)
    (dout, lddo), (af, ldaf), (as_, ldas), (bf, ldbf), (bs, ldbs) = m["dout"], m["af"], m["as_"], m["bf"], m["bs"]
    out_f, lddaf = _out(out_f, "out_f", n, C, af.device)
    out_s, lddas = _out(out_s, "out_s", n, C, af.device)
    parts = torch.empty((n, 2 * dim * C), dtype=torch.float32, device=af.device) if dim > 0 and want_parts else None
    # algorithmic bytes: dout and the four blocks read once each, daf and das (and the partials) written, the graph and the attributes
    alg = 28.0 * n * C + (0.0 if parts is None else 8.0 * n * dim * C) + _cgate_graph_bytes(g, n, C, dim)
    with _timed("cgate_bwd_row", _cgate_key(g, C, dim), alg, (8.0 * dim + 40.0) * max(g.nnz, g.nnz_in) * C):
        st = _lib.lib().ddmp_cgate_bwd_row_f32(g.handle, _p(dout), lddo, _p(af), ldaf, _p(as_), ldas, _p(bf), ldbf, _p(bs), ldbs, C,
                                               _p(attr), dim, _p(ef), _p(es), int(bool(mean)), _p(out_f), lddaf, _p(out_s), lddas,
                                               _p(parts), _stream())
    check(st, "ddmp_cgate_bwd_row_f32")
    return out_f, out_s, parts


def cgate_bwd_node(g: Graph, dout, af, as_, bf, bs, attr=None, ef=None, es=None, mean=False, out_f=None, out_s=None, out_r=None):
    """Node j's side of the backward (``ddmp_cgate_bwd_node_f32``) -> (dbf, dbs) [n, C] each, written completely; both gates are
    recomputed and the edges j -> i (or their count) are read through the mirror map.  ``out_f`` / ``out_s``: where they go;
    ``out_r``: a [n, C] block that also receives a copy of ``dout`` (the root term's gradient), or None.  Column blocks of one row
    buffer are fine."""
    n, C, m, attr, ef, es, dim = _cgate_operands(g, "cgate_bwd_node", attr, ef, es, dout=dout, af=af, as_=as_, bf=bf, bs=bs)
    (dout, lddo), (af, ldaf), (as_, ldas), (bf, ldbf), (bs, ldbs) = m["dout"], m["af"], m["as_"], m["bf"], m["bs"]
    out_f, lddbf = _out(out_f, "out_f", n, C, af.device)
    out_s, lddbs = _out(out_s, "out_s", n, C, af.device)
    ldds = 0
    if out_r is not None:
        out_r, ldds = _out(out_r, "out_r", n, C, af.device)
    # algorithmic bytes: dout and the four blocks read once each, dbf and dbs (and the root block) written, the graph (col + mirror)
    # and the attributes
    alg = (28.0 if out_r is None else 32.0) * n * C + _cgate_graph_bytes(g, n, C, dim, mirror=True)
    with _timed("cgate_bwd_node", _cgate_key(g, C, dim), alg, (4.0 * dim + 40.0) * max(g.nnz, g.nnz_in) * C):
        st = _lib.lib().ddmp_cgate_bwd_node_f32(g.handle, _p(dout), lddo, _p(af), ldaf, _p(as_), ldas, _p(bf), ldbf, _p(bs), ldbs, C,
                                                _p(attr), dim, _p(ef), _p(es), int(bool(mean)), _p(out_f), lddbf, _p(out_s), lddbs,
                                                _p(out_r), ldds, _stream())
    check(st, "ddmp_cgate_bwd_node_f32")
    return out_f, out_s


# ---------------------------------------------------------------------------------------- max aggregation
def _gmax_arg(arg, n, C):
    _chk(arg, torch.int32, "arg")
    if arg.dim() != 2 or arg.stride(1) != 1 or arg.shape[0] < n or arg.shape[1] != C:
        raise DdmpError("arg must be an int32 [>= %d, %d] with contiguous rows, got %s" % (n, C, tuple(arg.shape)))
    return arg, (arg.stride(0) if arg.shape[0] > 1 else max(C, arg.stride(0)))


def gather_max(g: Graph, b, a=None, out=None, want_arg=True):
    """Arg-max gather in one launch (``ddmp_gather_max_f32``) -> (y [n, C], arg int32 [n, C] | None):
    ``y[i, c] = a[i, c] + max_{e in row i} b[col e, c]``, ``arg[i, c]`` the source node id of the winning entry (ties: the smallest
    id).  A row without entries gets y = 0 (not ``a``) and arg = -1.  ``b``, ``a``: [n, C] (they may be column blocks of one row
    buffer; ``a=None`` means 0); ``want_arg=False`` skips the store of ``arg`` (a forward without a backward)."""
    _gat_graph(g)
    n = g.n_rows
    b, ldb = _rows(b, "b", n)
    C = b.shape[1]
    lda = 0
    if a is not None:
        a, lda = _rows(a, "a", n, C)
    out, ldy = _out(out, "out", n, C, b.device)
    arg, ldg = None, 0
    if want_arg:
        arg, ldg = _gmax_arg(torch.empty((n, C), dtype=torch.int32, device=b.device), n, C)
    # algorithmic bytes: every gathered row read once, the rows' own a read, y written, arg written, col, rowptr
    na = (1 if a is not None else 0) + (1 if want_arg else 0)
    alg = 4.0 * n * C * (2 + na) + 4.0 * g.nnz + 4.0 * (n + 1)
    with _timed("gather_max", (C, int(round(g.nnz / max(n, 1)))), alg, 1.0 * g.nnz * C, survey=8.0 * n * C + 4.0 * g.nnz + 4.0 * (n + 1)):
        st = _lib.lib().ddmp_gather_max_f32(g.handle, _p(b), ldb, _p(a), lda, C, _p(out), ldy, _p(arg), ldg, _stream())
    check(st, "ddmp_gather_max_f32")
    return out, arg


def gather_max_bwd(g: Graph, dg, arg, out=None):
    """Backward of ``gather_max`` in one launch (``ddmp_gather_max_bwd_f32``) -> (dA, dB), both [n, C]: ``dA[j] = dg[j]`` (0 for
    a row without entries), ``dB[j, c] = sum_{e' in row j} (arg[col e', c] == j ? dg[col e', c] : 0)``.  The results are views
    into ``out``, a float32 [n, 2 * Cp] row buffer with Cp = C rounded up to 4: dA in columns [0, C), dB in [Cp, Cp + C); the
    padding columns are left untouched.  ``out=None``: a buffer of its own."""
    _gat_graph(g)
    n = g.n_rows
    dg, lddg = _rows(dg, "dg", n)
    C = dg.shape[1]
    arg, ldg = _gmax_arg(arg, n, C)
    cp = (C + 3) // 4 * 4
    if out is None:
        out = torch.empty((n, 2 * cp), dtype=torch.float32, device=dg.device)
    out, _ = _mat(_chk(out, torch.float32, "out"), "out")
    if out.shape[0] != n or out.shape[1] != 2 * cp:
        raise DdmpError("gather_max_bwd: out must be [%d, %d], got %s" % (n, 2 * cp, tuple(out.shape)))
    (da, ldda), (db, lddb) = _mat(out[:, :C], "dA"), _mat(out[:, cp:cp + C], "dB")
    # algorithmic bytes: dg and arg read once each, dA and dB written, col, rowptr
    alg = 16.0 * n * C + 4.0 * g.nnz + 4.0 * (n + 1)
    with _timed("gather_max_bwd", (C, int(round(g.nnz / max(n, 1)))), alg, 1.0 * g.nnz * C):
        st = _lib.lib().ddmp_gather_max_bwd_f32(g.handle, _p(dg), lddg, _p(arg), ldg, C, _p(da), ldda, _p(db), lddb, _stream())
    check(st, "ddmp_gather_max_bwd_f32")
    return da, db


# ---------------------------------------------------------------------------------------- max aggregation of an edge-conditioned
# message over point-pair features
def ppf_entries(g: Graph, pos, normal):
    """Point-pair features of the COALESCED entries in one launch (``ddmp_ppf_entries_f32``) -> F float32 [g.nnz, 4]:
    ``F[e] = [|d|, angle(n_i, d), angle(n_j, d), angle(n_i, n_j)]`` for the entry e = (i, j = col e), ``d = pos[j] - pos[i]``,
    ``angle(a, b) = atan2(|a x b|, a . b)``; a loop entry is exactly 0.  ``pos``, ``normal``: float32 [n, 3] (column blocks of a
    wider row buffer are fine).  The result is cached on ``g`` by the identity and ``_version`` of the two tensors (weak
    references, like ``graph_for``): every layer of a net and every training step share one evaluation -- keep the tensors."""
    _gat_graph(g)
    hit = getattr(g, "_ppf", None)
    if (hit is not None and hit[0]() is pos and hit[1]() is normal and isinstance(pos, torch.Tensor) and isinstance(normal, torch.Tensor)
            and hit[2] == (pos._version, normal._version)):
        return hit[3]
    n = g.n_rows
    pos, ldp = _rows(pos, "pos", n, 3)
    normal, ldn = _rows(normal, "normal", n, 3)
    if pos.shape[0] != n or normal.shape[0] != n:
        raise DdmpError("pos and normal must be [%d, 3], got %s and %s" % (n, tuple(pos.shape), tuple(normal.shape)))
    f = torch.empty((g.nnz, 4), dtype=torch.float32, device=pos.device)
    # algorithmic bytes: pos and normal read once, F written, col + mirror
    with _timed("ppf_entries", (int(round(g.nnz / max(n, 1))),), 24.0 * n + 24.0 * g.nnz, 90.0 * g.nnz):
        st = _lib.lib().ddmp_ppf_entries_f32(g.handle, _p(pos), ldp, _p(normal), ldn, _p(f), _stream())
    check(st, "ddmp_ppf_entries_f32")
    g._ppf = (weakref.ref(pos), weakref.ref(normal), (pos._version, normal._version), f)
    return f


def _ppf_f(g, f):
    _chk(f, torch.float32, "f")
    if f.dim() != 2 or tuple(f.shape) != (g.nnz, 4) or not f.is_contiguous():
        raise DdmpError("f must be a contiguous float32 [%d, 4] (one row per coalesced entry: ops.ppf_entries), got %s"
                        % (g.nnz, tuple(f.shape)))
    return f


def gather_max_attr(g: Graph, b, f, e, out=None, want_arg=True):
    """Arg-max gather of an edge-conditioned message in one launch (``ddmp_gather_max_attr_f32``) -> (y [n, C], arg int32 [n, C]
    | None): ``y[i, c] = max_{entry t in row i} (b[col t, c] + sum_d f[t, d] e[d, c])``, ``arg[i, c]`` the source node id of the
    winning entry (ties: the smallest id).  A row without entries gets y = 0 and arg = -1.  ``b``: [n, C] (a column block of a
    row buffer is fine) or None = 0; ``f``: contiguous [g.nnz, 4] (``ppf_entries``); ``e``: contiguous [4, C] (the edge weights
    TRANSPOSED); ``want_arg=False`` skips the store of ``arg`` (a forward without a backward)."""
    _gat_graph(g)
    n = g.n_rows
    f = _ppf_f(g, f)
    _chk(e, torch.float32, "e")
    if e.dim() != 2 or e.shape[0] != 4 or e.shape[1] < 1 or not e.is_contiguous():
        raise DdmpError("e must be a contiguous float32 [4, C], got %s" % (tuple(e.shape),))
    C = e.shape[1]
    ldb = 0
    if b is not None:
        b, ldb = _rows(b, "b", n, C)
    out, ldy = _out(out, "out", n, C, f.device)
    arg, ldg = None, 0
    if want_arg:
        arg, ldg = _gmax_arg(torch.empty((n, C), dtype=torch.int32, device=f.device), n, C)
    # algorithmic bytes: every gathered row read once, y (and arg) written, F, E, col, rowptr
    nb = (1 if b is not None else 0) + 1 + (1 if want_arg else 0)
    alg = 4.0 * n * C * nb + 20.0 * g.nnz + 16.0 * C + 4.0 * (n + 1)
    with _timed("gather_max_attr", (C, int(round(g.nnz / max(n, 1)))), alg, 9.0 * g.nnz * C):
        st = _lib.lib().ddmp_gather_max_attr_f32(g.handle, _p(b), ldb, _p(f), _p(e), C, _p(out), ldy, _p(arg), ldg, _stream())
    check(st, "ddmp_gather_max_attr_f32")
    return out, arg


def gather_max_attr_bwd(g: Graph, dg, arg, f, out=None, want_parts=True):
    """Backward of ``gather_max_attr`` in ONE launch (``ddmp_gather_max_attr_bwd_f32``) -> (dB [n, C], parts | None):
    ``dB[j, c] = sum_{e' in row j} (arg[col e', c] == j ? dg[col e', c] : 0)``; ``parts`` (``want_parts``): float32
    [ceil(n / 8), 4 * C], the shares of ``dE[d, c] = sum_i dg[i, c] f[entry(i, arg[i, c]), d]`` of every 8 consecutive rows -- their
    column sum ``gatv2_datt(parts, 4)`` is dE [4, C].  ``out``: where dB goes (a column block of a row buffer is fine)."""
    _gat_graph(g)
    n = g.n_rows
    dg, lddg = _rows(dg, "dg", n)
    C = dg.shape[1]
    arg, ldg = _gmax_arg(arg, n, C)
    f = _ppf_f(g, f)
    out, lddb = _out(out, "out", n, C, dg.device)
    parts = torch.empty(((n + 7) // 8, 4 * C), dtype=torch.float32, device=dg.device) if want_parts else None
    # algorithmic bytes: dg and arg read once each, dB (and the partials) written, F, col, rowptr
    alg = 12.0 * n * C + (2.0 * n * C if want_parts else 0.0) + (20.0 if want_parts else 4.0) * g.nnz + 4.0 * (n + 1)
    with _timed("gather_max_attr_bwd", (C, int(round(g.nnz / max(n, 1)))), alg, (5.0 if want_parts else 1.0) * g.nnz * C):
        st = _lib.lib().ddmp_gather_max_attr_bwd_f32(g.handle, _p(dg), lddg, _p(arg), ldg, _p(f), C, _p(out), lddb, _p(parts),
                                                     _stream())
    check(st, "ddmp_gather_max_attr_bwd_f32")
    return out, parts


# ---------------------------------------------------------------------------------------- neighbour statistics and moments
#   Written once for both operators: the ``want`` validation, the (pointer, leading dimension) table of
# the forward's blocks and args, and the backward's operand table with its refusals.
STATS = ("mean", "add", "max", "min")
MOMENTS = ("mean", "sum", "max", "min", "std", "var")
_NBR_BLOCK = {"mean": "sum", "add": "sum", "sum": "sum", "max": "max", "min": "min", "std": "var", "var": "var"}


def _nbr_want(want, names, pairs):
    want = (want,) if isinstance(want, str) else tuple(want)
    if (not want or any(w not in names for w in want) or len(set(want)) != len(want)
            or any(u in want and v in want for u, v in pairs)):
        raise DdmpError("want must be a non-empty sequence of distinct names out of %r with %s, got %r"
                        % (names, " and ".join("at most one of %r / %r" % uv for uv in pairs), want))
    return want


def _nbr_out(who, out, n, width, device):
    if out is None:
        out = torch.empty((n, width), dtype=torch.float32, device=device)
    out, ldo = _mat(_chk(out, torch.float32, "out"), "out")
    if out.shape[0] != n or out.shape[1] < width:
        raise DdmpError("%s: out must be [%d, >= %d], got %s" % (who, n, width, tuple(out.shape)))
    return out, ldo


def _nbr_table(want, firsts, want_arg, n, C, device):
    """-> (ptr, args, flat): ``ptr[block]`` = (tensor, leading dimension) of the sum / max / min / var block from ``firsts`` (parallel
    to ``want``) and of the args ``amax`` / ``amin`` allocated here (``want_arg``), (None, 0) where absent; ``args`` parallel to
    ``want``; ``flat``: S, lds, Mx, ldmx, argmx, ldamx, Mn, ldmn, argmn, ldamn as both entry points take them."""
    ptr = {k: (None, 0) for k in ("sum", "max", "amax", "min", "amin", "var")}
    args = [None] * len(want)
    for k, w in enumerate(want):
        ptr[_NBR_BLOCK[w]] = firsts[k]
        if w in ("max", "min") and want_arg:
            args[k] = torch.empty((n, C), dtype=torch.int32, device=device)
            ptr["a" + w] = _gmax_arg(args[k], n, C)
    flat = [v for k in ("sum", "max", "amax", "min", "amin") for v in (_p(ptr[k][0]), ptr[k][1])]
    return ptr, args, flat


def _nbr_bwd_operands(who, n, rows, argmx, argmn, invdeg, bad, rule):
    """The backward's operands.  ``rows``: name -> float32 [n, C] tensor or None, with ds, dmx and dmn among them; ``bad``: the
    operator's own refusal, ``rule`` its wording.  -> (first, C, op, invdeg): the first gradient present, ``op[name]`` = the
    (pointer, leading dimension) arguments of every row operand and arg ((None, 0) where absent), invdeg checked."""
    ds, dmx, dmn = rows["ds"], rows["dmx"], rows["dmn"]
    first = next((t for t in (ds, dmx, dmn) if t is not None), None)
    if (first is None or (dmx is None) != (argmx is None) or (dmn is None) != (argmn is None) or (ds is None and invdeg is not None)
            or bad):
        raise DdmpError("%s: at least one of ds, dmx, dmn; dmx comes with argmx, dmn with argmn; %s" % (who, rule))
    C = first.shape[1] if isinstance(first, torch.Tensor) and first.dim() == 2 else 0
    op = {name: (None, 0) if t is None else _rows(t, name, n, C) for name, t in rows.items()}
    for name, t in (("argmx", argmx), ("argmn", argmn)):
        op[name] = (None, 0) if t is None else _gmax_arg(t, n, C)
    if invdeg is not None:
        invdeg = _gat_arr(invdeg, (n,), "invdeg")
    return first, C, {name: (_p(t), ld) for name, (t, ld) in op.items()}, invdeg


def _stats_want(want):
    """``want`` as a tuple of distinct names out of ``STATS`` with at most one of mean / add, or ``DdmpError``."""
    return _nbr_want(want, STATS, (("mean", "add"),))


def gather_stats(g: Graph, x, want=("mean",), root=None, bias=None, copy_x=False, want_arg=True, out=None):
    """Mean-or-sum / max / min of the neighbours' rows in ONE launch (``ddmp_gather_stats_f32``): every neighbour row is read once
    and feeds every statistic in ``want`` (names out of ``STATS``, at most one of mean / add).  -> (blocks, args, invdeg):

    * ``blocks``: one [n, C] result per entry of ``want``, in that order, then (``copy_x``) a copy of ``x[:n]``.  They are the
      consecutive column blocks [k * C, (k + 1) * C) of ``out``, a float32 [n, >= len(blocks) * C] row buffer (further columns are
      left untouched); ``out=None``: a buffer of its own, exactly that wide.
    * ``args``: parallel to ``want``: int32 [n, C], the source node id of the winning entry, for max / min (ties: the smallest id;
      -1 for a row without entries; ``want_arg=False``: not stored, None -- a forward without a backward), None for mean / add.
    * ``invdeg``: [n], 1 / the number of input edges into the row (0 for a row without entries) when ``want`` has mean, else None.

    mean / add: ``w_i sum_e a_e x[col e] + root[i] + bias`` with ``root`` [n, C] (it may be a column block of the buffer ``x`` is
    a block of) and ``bias`` [C] both optional and only allowed with mean / add; a row without entries gets ``root + bias`` (or
    0), and 0 in max / min."""
    _gmm_graph(g)
    want = _stats_want(want)
    n = g.n_rows
    x, ldx = _rows(x, "x", n)
    C = x.shape[1]
    summed = "mean" in want or "add" in want
    if (root is not None or bias is not None) and not summed:
        raise DdmpError("gather_stats: root and bias belong to the mean / add block, which was not requested")
    ldr = 0
    if root is not None:
        root, ldr = _rows(root, "root", n, C)
    if bias is not None:
        bias = _gat_arr(bias, (C,), "bias")
    nb = len(want) + bool(copy_x)
    out, _ = _nbr_out("gather_stats", out, n, nb * C, x.device)
    blocks = [out[:, k * C:(k + 1) * C] for k in range(nb)]
    _, args, flat = _nbr_table(want, [_mat(blk, w) for blk, w in zip(blocks, want)], want_arg, n, C, x.device)
    xc, ldxc = _mat(blocks[-1], "copy") if copy_x else (None, 0)
    invdeg = torch.empty(n, dtype=torch.float32, device=x.device) if "mean" in want else None
    # algorithmic bytes: every gathered row read ONCE whatever the number of statistics, one row written per block and per arg, the
    # root block and the row's own features (copy_x) read, invdeg written, col + multiplicity, rowptr
    n_arg = sum(a is not None for a in args)
    alg = 4.0 * n * C * (1 + nb + n_arg + (root is not None) + bool(copy_x)) + 4.0 * n * (invdeg is not None) + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("gather_stats", (C, "+".join(want), int(round(g.nnz / max(n, 1)))), alg, 1.0 * g.nnz * C * len(want),
                survey=8.0 * n * C + 4.0 * g.nnz + 4.0 * (n + 1)):
        st = _lib.lib().ddmp_gather_stats_f32(g.handle, _p(x), ldx, C, int("mean" in want), _p(root), ldr, _p(bias), *flat,
                                              _p(invdeg), _p(xc), ldxc, _stream())
    check(st, "ddmp_gather_stats_f32")
    return tuple(blocks), tuple(args), invdeg


def gather_stats_bwd(g: Graph, ds=None, invdeg=None, dmx=None, argmx=None, dmn=None, argmn=None, dx0=None, root=False, out=None):
    """Backward of ``gather_stats`` in one launch (``ddmp_gather_stats_bwd_f32``) -> (dx [n, C] written completely, droot [n, C] |
    None): ``dx[j] = dx0[j] + sum_{e' in row j} (a_{mirror e'} w_i ds[i] + (argmx[i] == j ? dmx[i] : 0) + (argmn[i] == j ?
    dmn[i] : 0))`` with ``i = col e'`` and ``w_i = invdeg[i]`` (the mean) or 1 (``invdeg=None``: the sum).  ``ds``, ``dmx`` (with
    ``argmx``) and ``dmn`` (with ``argmn``): the gradients of the requested blocks, [n, C] each, at least one; ``dx0``: the
    gradient that arrived through the ``copy_x`` block, or None.  ``root``: the launch also copies ``ds`` into the root block's
    columns.  ``out``: a float32 [n, >= C (+ C)] row buffer that receives [dx | droot] in its leading columns (the results are then
    views of it; further columns are left untouched); None: a buffer of its own."""
    _gmm_graph(g)
    n = g.n_rows
    first, C, op, invdeg = _nbr_bwd_operands("gather_stats_bwd", n, dict(ds=ds, dmx=dmx, dmn=dmn, dx0=dx0), argmx, argmn, invdeg,
                                             ds is None and root, "invdeg and root need ds")
    (dx, lddx), (dr, lddr) = _out_with_root(out, "gather_stats_bwd", n, C, C, root, first.device)
    ns = sum(t is not None for t in (ds, dmx, dmn, dx0))
    # algorithmic bytes: every requested gradient stream (and each arg) read once, dx (and the root block, with ds once more)
    # written, invdeg, col + mirror + multiplicity, rowptr
    alg = (4.0 * n * C * (ns + (argmx is not None) + (argmn is not None) + 1 + 2 * bool(root)) + 4.0 * n * (invdeg is not None)
           + 12.0 * g.nnz + 4.0 * (n + 1))
    with _timed("gather_stats_bwd", (C, ns, int(round(g.nnz / max(n, 1)))), alg, 1.0 * g.nnz * C * ns):
        st = _lib.lib().ddmp_gather_stats_bwd_f32(g.handle, C, *op["ds"], _p(invdeg), *op["dmx"], *op["argmx"], *op["dmn"],
                                                  *op["argmn"], *op["dx0"], _p(dx), lddx, _p(dr), lddr, _stream())
    check(st, "ddmp_gather_stats_bwd_f32")
    return dx, dr


def _moments_want(want):
    """``want`` as a tuple of distinct names out of ``MOMENTS`` with at most one of mean / sum and at most one of std / var, or
    ``DdmpError``."""
    return _nbr_want(want, MOMENTS, (("mean", "sum"), ("std", "var")))


def gather_moments(g: Graph, b, want=("mean",), root=None, tower_width=None, want_arg=True, out=None):
    """Mean-or-sum / max / min / std-or-var of the neighbours' rows in ONE launch (``ddmp_gather_moments_f32``): every neighbour row
    of ``b`` [n, C] is read once and feeds every statistic in ``want`` (names out of ``MOMENTS``, at most one of mean / sum and of
    std / var).  -> (blocks, args, invdeg, mu):

    * ``blocks``: one result per entry of ``want``, in that order, views into ``out``, a float32 [n, >= len(want) * C] row buffer
      (further columns are left untouched; ``out=None``: a buffer of its own, exactly that wide).  Plain layout
      (``tower_width`` None or C): block k is the columns [k * C, (k + 1) * C), an [n, C] view.  Tower-major (``tower_width`` = tw,
      a divisor of C; T = C / tw towers): the buffer is ``[tower][statistic][tw]``, column c of block k lands at
      ``(c // tw) * len(want) * tw + k * tw + c % tw``, and block k is the [n, T, tw] view of it -- the columns
      ``[t * len(want) * tw, (t + 1) * len(want) * tw)`` hold every statistic of tower t.
    * ``args``: parallel to ``want``: int32 [n, C] (plain), the source node id of the winning entry, for max / min (ties: the smallest
      id; -1 for a row without entries; ``want_arg=False``: not stored, None), None for the others.
    * ``invdeg``: [n], 1 / the number of input edges into the row (0 for a row without entries), always.
    * ``mu``: [n, C], the neighbour mean WITHOUT the root, when ``want`` has std or var (the backward needs it), else None.

    std / var: the second central moment from sums shifted by the row's first entry, ``std = var > 1e-5 ? sqrt(var) : 0`` (PyG
    2.2.0's ``StdAggregation``).  ``root`` [n, C] (it may be a column block of the buffer ``b`` is a block of): on a row with
    entries it is added to mean / max / min and ``deg * root`` to sum, never to std / var; a row without entries gets 0 in every
    block whatever ``root`` is."""
    _gmm_graph(g)
    want = _moments_want(want)
    n = g.n_rows
    b, ldb = _rows(b, "b", n)
    C = b.shape[1]
    tw = C if tower_width is None else tower_width
    if not isinstance(tw, int) or isinstance(tw, bool) or tw < 1 or C % tw:
        raise DdmpError("gather_moments: tower_width must be a divisor of C = %d, got %r" % (C, tower_width))
    ldr = 0
    if root is not None:
        root, ldr = _rows(root, "root", n, C)
    nb, T = len(want), C // tw
    out, ldo = _nbr_out("gather_moments", out, n, nb * C, b.device)
    if T == 1:
        blocks = [out[:, k * C:(k + 1) * C] for k in range(nb)]
    else:
        towers = out[:, :nb * C].unflatten(1, (T, nb, tw))
        blocks = [towers[:, :, k] for k in range(nb)]
    # (a block's first column; the kernel places the towers)
    ptr, args, flat = _nbr_table(want, [(out[:, k * tw:], ldo) for k in range(nb)], want_arg, n, C, b.device)
    has_var = ptr["var"][0] is not None
    mu = torch.empty((n, C), dtype=torch.float32, device=b.device) if has_var else None
    invdeg = torch.empty(n, dtype=torch.float32, device=b.device)
    # algorithmic bytes: every gathered row read ONCE whatever the number of statistics, one row written per block, per arg and for mu,
    # the root block read, invdeg written, col + multiplicity, rowptr
    n_arg = sum(a is not None for a in args)
    alg = 4.0 * n * C * (1 + nb + n_arg + (root is not None) + has_var) + 4.0 * n + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("gather_moments", (C, "+".join(want), tw, int(round(g.nnz / max(n, 1)))), alg, 1.0 * g.nnz * C * (nb + has_var),
                survey=8.0 * n * C + 4.0 * g.nnz + 4.0 * (n + 1)):
        st = _lib.lib().ddmp_gather_moments_f32(g.handle, _p(b), ldb, C, int("mean" in want), int("std" in want), _p(root), ldr, tw,
                                                nb * tw, *flat, _p(ptr["var"][0]), ptr["var"][1], _p(mu), C, _p(invdeg), _stream())
    check(st, "ddmp_gather_moments_f32")
    return tuple(blocks), tuple(args), invdeg, mu


def gather_moments_bwd(g: Graph, ds=None, dq=None, b=None, invdeg=None, dmx=None, argmx=None, dmn=None, argmn=None,
                       out=None):
    """Backward of ``gather_moments`` in one launch (``ddmp_gather_moments_bwd_f32``) -> db [n, C], written completely:
    ``db[j] = sum_{e' in row j} (a w_i ds[i] + (argmx[i] == j ? dmx[i] : 0) + (argmn[i] == j ? dmn[i] : 0)) + b[j] *
    sum_{e' in row j} a w_i dq[i]`` with ``i = col e'``, ``a`` the mirrored multiplicity and ``w_i = invdeg[i]`` (None: 1).  All
    operands [n, C], plain layout.  ``dq`` (with ``b``, and needing ``ds``) is the second stream of the std / var chain rule: with
    ``G = dstd / std`` where ``std > 0`` (else 0), or ``2 dvar``, pass ``dq = G`` and add ``-G * mu`` to ``ds``.
    ``out``: a float32 [n, C] row block (it may be a column block
    of a wider buffer) that receives db; None: a tensor of its own."""
    _gmm_graph(g)
    n = g.n_rows
    first, C, op, invdeg = _nbr_bwd_operands("gather_moments_bwd", n, dict(ds=ds, dq=dq, b=b, dmx=dmx, dmn=dmn), argmx, argmn, invdeg,
                                             (ds is None and dq is not None) or (dq is None) != (b is None),
                                             "dq comes with b and needs ds; invdeg needs ds")
    db, lddb = _out(out, "out", n, C, first.device)
    if db.shape[0] != n:
        raise DdmpError("gather_moments_bwd: out must be [%d, %d], got %s" % (n, C, tuple(db.shape)))
    ns = sum(t is not None for t in (ds, dq, dmx, dmn))
    # algorithmic bytes: every requested gradient stream (and each arg) read once, the row's own b read, db written, invdeg, col +
    # mirror + multiplicity, rowptr
    alg = (4.0 * n * C * (ns + (argmx is not None) + (argmn is not None) + (b is not None) + 1) + 4.0 * n * (invdeg is not None)
           + 12.0 * g.nnz + 4.0 * (n + 1))
    with _timed("gather_moments_bwd", (C, ns, int(round(g.nnz / max(n, 1)))), alg, 1.0 * g.nnz * C * ns):
        st = _lib.lib().ddmp_gather_moments_bwd_f32(g.handle, C, *op["ds"], *op["dq"], *op["b"], _p(invdeg), *op["dmx"], *op["argmx"],
                                                    *op["dmn"], *op["argmn"], _p(db), lddb, _stream())
    check(st, "ddmp_gather_moments_bwd_f32")
    return db


# ---------------------------------------------------------------------------------------- softmax aggregation
def _smax_scalars(who, t, msg_eps):
    """-> (t, has_eps, eps) as Python numbers: ``t`` any finite float, ``msg_eps`` None or a finite float >= 0."""
    t = float(t)
    if not math.isfinite(t):
        raise DdmpError("%s: the temperature t must be finite, got %r" % (who, t))
    if msg_eps is None:
        return t, 0, 0.0
    eps = float(msg_eps)
    if not math.isfinite(eps) or eps < 0.0:
        raise DdmpError("%s: msg_eps must be None or a finite float >= 0, got %r" % (who, msg_eps))
    return t, 1, eps


def gather_softmax(g: Graph, h, t, msg_eps=None, root=None, out=None, want_lse=True):
    """Per-channel softmax aggregation of the neighbours' rows in ONE launch (``ddmp_gather_softmax_f32``) -> (y [n, C], lse [n, C] |
    None): with the message ``m_j = relu(h[j]) + msg_eps`` (``msg_eps=None``: ``m_j = h[j]``, a plain ``SoftmaxAggregation``) and the
    temperature ``t`` (any finite float), per row i and channel c ``y = root[i] + sum_e p_e m_e`` with ``p_e = a_e exp(t m_e) /
    sum_e a_e exp(t m_e)`` over the row's entries (``a_e``: the entry's multiplicity) and ``lse = log sum_e a_e exp(t m_e)``, both
    evaluated against the running maximum.  ``h`` [n, C]; ``root`` [n, C] optional (it may be a column block of the buffer ``h`` is a
    block of); a row without entries gets its root row bit for bit (0 without root) and lse = 0.  ``out``: a float32 [n, C] row block
    (it may be a column block of a wider buffer) that receives y; None: a tensor of its own.  ``want_lse=False`` skips the store of
    ``lse`` (a forward without a backward)."""
    _gmm_graph(g)
    t, has_eps, eps = _smax_scalars("gather_softmax", t, msg_eps)
    n = g.n_rows
    h, ldh = _rows(h, "h", n)
    C = h.shape[1]
    ldr = 0
    if root is not None:
        root, ldr = _rows(root, "root", n, C)
    y, ldy = _out(out, "out", n, C, h.device)
    if y.shape[0] != n:
        raise DdmpError("gather_softmax: out must be [%d, %d], got %s" % (n, C, tuple(y.shape)))
    lse = torch.empty((n, C), dtype=torch.float32, device=h.device) if want_lse else None
    # algorithmic bytes: every gathered row read ONCE, y (and lse) written, the root block read, col + multiplicity, rowptr
    alg = 4.0 * n * C * (2 + bool(want_lse) + (root is not None)) + 8.0 * g.nnz + 4.0 * (n + 1)
    with _timed("gather_softmax", (C, has_eps, int(round(g.nnz / max(n, 1)))), alg, 8.0 * g.nnz * C,
                survey=8.0 * n * C + 4.0 * g.nnz + 4.0 * (n + 1)):
        st = _lib.lib().ddmp_gather_softmax_f32(g.handle, _p(h), ldh, C, t, has_eps, eps, _p(root), ldr, _p(y), ldy, _p(lse), C,
                                                _stream())
    check(st, "ddmp_gather_softmax_f32")
    return y, lse


def gather_softmax_bwd(g: Graph, dout, h, y, lse, t, msg_eps=None, root=False, want_dt=False, out=None):
    """Backward of ``gather_softmax`` in one launch (``ddmp_gather_softmax_bwd_f32``) -> (dh [n, C] written completely, droot [n, C] |
    None, dt_rows [n] | None).  ``y`` is the forward's aggregate WITHOUT the root term (a caller whose forward fused a root passes
    ``y - root``), ``lse`` the forward's.  With ``i = col e'``, ``w`` the mirrored multiplicity and ``p = exp(t m_j - lse[i])``:
    ``s[j] = sum_{e' in row j} w p dout[i]``, ``r[j] = sum_{e' in row j} w p dout[i] (m_j - y[i])``, ``dh[j] = (s + t r)`` times
    ``[h[j] > 0]`` when ``msg_eps`` is given, ``droot[j] = dout[j]`` (``root=True``), ``dt_rows[j] = sum_c m_j[c] r[j, c]``
    (``want_dt``; the temperature's gradient is ``dt_rows.sum()``).  ``root="add"``: the forward's root WAS ``h``, so ``dout[j]`` is
    added to ``dh[j]`` (after the mask) and there is no droot block.  ``out``: a float32 [n, >= C (+ C)] row buffer that receives
    [dh | droot] in its leading columns (the results are then views of it; further columns are left untouched); None: a buffer of its
    own."""
    _gmm_graph(g)
    t, has_eps, eps = _smax_scalars("gather_softmax_bwd", t, msg_eps)
    n = g.n_rows
    dout, lddo = _rows(dout, "dout", n)
    C = dout.shape[1]
    h, ldh = _rows(h, "h", n, C)
    y, ldy = _rows(y, "y", n, C)
    lse, ldl = _rows(lse, "lse", n, C)
    if root not in (False, True, "add"):
        raise DdmpError("gather_softmax_bwd: root must be False, True or 'add', got %r" % (root,))
    add, root = int(root == "add"), root is True
    (dh, lddh), (dr, lddr) = _out_with_root(out, "gather_softmax_bwd", n, C, C, root, dout.device)
    dt = torch.empty(n, dtype=torch.float32, device=dout.device) if want_dt else None
    # algorithmic bytes: the three neighbour streams (dout, y, lse) read once each, the row's own h read, dh written (and the root
    # block, with dout once more), dt_rows, col + mirror + multiplicity, rowptr
    alg = 4.0 * n * C * (5 + 2 * root + add) + 4.0 * n * bool(want_dt) + 12.0 * g.nnz + 4.0 * (n + 1)
    with _timed("gather_softmax_bwd", (C, has_eps, int(round(g.nnz / max(n, 1)))), alg, 9.0 * g.nnz * C):
        st = _lib.lib().ddmp_gather_softmax_bwd_f32(g.handle, C, _p(dout), lddo, _p(h), ldh, _p(y), ldy, _p(lse), ldl, t, has_eps, eps,
                                                    add, _p(dh), lddh, _p(dr), lddr, _p(dt), _stream())
    check(st, "ddmp_gather_softmax_bwd_f32")
    return dh, dr, dt


def spmm_axpby(g: Graph, x, out=None, z=None, z2=None, a=1.0, b=0.0, c=0.0, d=0.0):
    """out[i] = a * (dinv_i * sum_j dinv_j x[j]) + b * x[i] + c * z[i] + d * z2[i], float32 (ddmp_spmm_axpby_f32): one step of a
    three-term recurrence per launch.  ``z`` / ``z2`` optional (their coefficient is then ignored); ``out`` may be ``z`` or ``z2``,
    never ``x``.  Column blocks of wider buffers are fine (any row stride)."""
    x, ldx = _mat(_chk(x, torch.float32, "x"), "x")
    if x.shape[0] < g.n_cols:
        raise DdmpError("x has %d rows, graph references %d nodes" % (x.shape[0], g.n_cols))
    C = x.shape[1]
    if out is None:
        out = torch.empty((g.n_rows, C), dtype=x.dtype, device=x.device)
    out, ldy = _mat(_chk(out, torch.float32, "out"), "out")
    ldz = ldz2 = 0
    if z is not None:
        z, ldz = _mat(_chk(z, torch.float32, "z"), "z")
    if z2 is not None:
        z2, ldz2 = _mat(_chk(z2, torch.float32, "z2"), "z2")
    for t, nm in ((out, "out"), (z, "z"), (z2, "z2")):
        if t is not None and (t.shape[0] < g.n_rows or t.shape[1] != C):
            raise DdmpError("%s must be [>= %d, %d], got %s" % (nm, g.n_rows, C, tuple(t.shape)))
    # algorithmic bytes: N x C x 4 per stream actually touched (the gathered rows, the output, x's own rows when b != 0, z, z2)
    # + int32 col ids, rowptr, dinv
    streams = 2 + (1 if b != 0 else 0) + (z is not None) + (z2 is not None)
    tables = 4.0 * g.nnz + 4.0 * (g.n_rows + 1) + 4.0 * g.n_rows
    with _timed("spmm_axpby", (C, int(round(g.nnz / max(g.n_rows, 1)))), 4.0 * streams * g.n_rows * C + tables, 2.0 * g.nnz * C,
                survey=8.0 * g.n_rows * C + tables):
        st = _lib.lib().ddmp_spmm_axpby_f32(g.handle, _p(x), ldx, _p(out), ldy, _p(z), ldz, _p(z2), ldz2, C, float(a), float(b),
                                            float(c), float(d), _stream())
    check(st, "ddmp_spmm_axpby_f32")
    return out


def spmm_stats_supported(C, dtype=torch.float32):
    """Does spmm_stats take its fused form for C channels?"""
    if dtype == torch.bfloat16:
        return C % 16 == 0 and C <= 1024
    return dtype == torch.float32 and bool(_lib.lib().ddmp_spmm_stats_supported(int(C)))


def spmm_stats(g: Graph, x, out, ref, sums, bias=None, pro=None, slope=SLOPE, bn=None):
    """out = spmm(g, x) (+bias, prologue) and sums (float64 [2C]) = bn_stats(out) from the same kernel: the statistics are
    summed around ``ref`` (float32 [C], close to the column means -- the previous iteration's batch means; zeros are valid)
    in float32 over 16 rows at a time, in float64 from there on (ddmp_spmm_stats)."""
    x, ldx = _mat(x, "x")
    out, ldy = _mat(out, "out", x)
    C = x.shape[1]
    ps, psh = (None, None) if pro is None else pro
    L = _lib.lib()
    ws = Workspace.get(max(L.ddmp_spmm_bnred_ws_bytes(g.n_rows, C, _dt(x)), L.ddmp_colreduce_workspace_bytes(g.n_rows, C)), x.device)
    es = x.element_size()
    alg = float(es) * (g.n_cols + g.n_rows) * C + 4.0 * g.nnz + 8.0 * g.n_rows
    with _timed("spmm", (C, int(round(g.nnz / max(g.n_rows, 1)))), alg, 2.0 * g.nnz * C, survey=2.0 * g.n_rows * C * es + 4.0 * g.nnz + 4.0 * (g.n_rows + 1) + 4.0 * g.n_rows):
        o, keep = _mk_opts(bn, want_bn=True)
        st = L.ddmp_spmm_stats_o(g.handle, _p(x), ldx, _p(out), ldy, C, _dt(x), _p(bias), _p(ps), _p(psh), slope,
                                 _p(_chk(ref, torch.float32, "ref")), _p(sums), _p(ws), ws.numel(), _stream(), o)
    check(st, "ddmp_spmm_stats")
    return out


def spmm_bnred(g: Graph, x, out, yp, bn4, sums2, slope=SLOPE, bn=None):
    """out = spmm(g, x) (a gradient dZ) and sums2 = bn_bwd_reduce(out, yp, bn4) from the same kernel."""
    x, ldx = _mat(x, "x")
    out, ldy = _mat(out, "out", x)
    yp, ldyp = _mat(yp, "yp", x)
    C = x.shape[1]
    L = _lib.lib()
    ws = Workspace.get(L.ddmp_spmm_bnred_ws_bytes(g.n_rows, C, _dt(x)), x.device)
    alg = 3.0 * g.n_rows * C * x.element_size() + 4.0 * g.nnz + 4.0 * (g.n_rows + 1) + 4.0 * g.n_rows
    with _timed("spmm", (C, int(round(g.nnz / max(g.n_rows, 1)))), alg, 2.0 * g.nnz * C, survey=2.0 * g.n_rows * C * x.element_size() + 4.0 * g.nnz + 4.0 * (g.n_rows + 1) + 4.0 * g.n_rows):
        o, keep = _mk_opts(bn, want_bn=True)
        st = L.ddmp_spmm_bnred_o(g.handle, _p(x), ldx, _p(out), ldy, C, _dt(x), _p(yp), ldyp, _p(bn4[0]), _p(bn4[1]),
                                 _p(bn4[2]), _p(bn4[3]), slope, _p(sums2), _p(ws), ws.numel(), _stream(), o)
    check(st, "ddmp_spmm_bnred")
    return out


def spmm_bnbwd_supported(C):
    return bool(_lib.lib().ddmp_spmm_bnbwd_supported(int(C)))


def spmm_bnbwd(g: Graph, dz, yb, bn4, c10, out, slope=SLOPE):
    """out[:n_rows] = A_hat @ dY with dY = BatchNorm+LeakyReLU backward of (dz, yb) rebuilt on the gather (what
    bn_bwd_apply would have written: a*dz*lrelu'(a*yb+b) + c1*yb + c0)."""
    dz, lddz = _mat(dz, "dz")
    yb, ldyb = _mat(yb, "yb", dz)
    out, ldo = _mat(out, "out", dz)
    C = dz.shape[1]
    assert dz.shape[0] >= g.n_cols and yb.shape[0] >= g.n_cols and out.shape[0] >= g.n_rows and yb.shape[1] == C
    es = dz.element_size()
    with _timed("spmm", (C, int(round(g.nnz / max(g.n_rows, 1)))), es * (2.0 * g.n_cols + g.n_rows) * C + 4.0 * g.nnz + 8.0 * g.n_rows,
                2.0 * g.nnz * C, survey=2.0 * g.n_rows * C * es + 4.0 * g.nnz + 4.0 * (g.n_rows + 1) + 4.0 * g.n_rows):
        st = _lib.lib().ddmp_spmm_bnbwd(g.handle, _p(dz), lddz, _p(yb), ldyb, _p(out), ldo, C, _dt(dz), _p(bn4[0]),
                                        _p(bn4[1]), _p(c10[0]), _p(c10[1]), slope, _stream())
    check(st, "ddmp_spmm_bnbwd")
    return out


class WeightPlan:
    """The argument arrays of one ddmp_gemm_prepare_weights call, built once (the weight matrices are views of a parameter
    arena whose address does not change between iterations); ``run()`` re-splits the current weights."""

    def __init__(self, items, n_rows, scratch):
        n = len(items)
        assert scratch.dtype == torch.float32 and scratch.numel() >= 8 * n
        self._keep = (items, scratch)
        self.n, self.n_rows, self.scratch = n, int(n_rows), scratch
        arrs = ((ctypes.c_void_p * n)(*[w.data_ptr() for w, _, _, _ in items]),
                (ctypes.c_int64 * n)(*[w.stride(0) for w, _, _, _ in items]),
                (ctypes.c_int * n)(*[w.shape[0] for w, _, _, _ in items]),
                (ctypes.c_int * n)(*[w.shape[1] for w, _, _, _ in items]),
                (ctypes.c_int * n)(*[int(f) for _, f, _, _ in items]),
                (ctypes.c_int * n)(*[int(bool(h)) for _, _, h, _ in items]),
                (ctypes.c_void_p * n)(*[p.data_ptr() for _, _, _, p in items]),
                (ctypes.c_size_t * n)(*[p.numel() for _, _, _, p in items]))
        self._arrs = arrs
        self._args = [ctypes.cast(a, ctypes.c_void_p) for a in arrs]

    def run(self):
        check(_lib.lib().ddmp_gemm_prepare_weights(self.n, *self._args, self.n_rows, _p(self.scratch), _stream()),
              "ddmp_gemm_prepare_weights")


def gemm_prepare_weights(items, n_rows, scratch):
    """items: [(w [M,K] float32, form 0 forward | 1 dgrad, has_pro, planes uint8 buffer)]: split all these weight matrices
    into the planes their products over ``n_rows`` rows want, in two launches (ddmp_gemm_prepare_weights).  The GEMM calls
    then take ``wplanes=planes``.  ``scratch``: float32 [>= 8 len(items)]."""
    WeightPlan(items, n_rows, scratch).run()


def gemm_rows_workspace_bytes(K, M):
    return int(_lib.lib().ddmp_gemm_rows_workspace_bytes(int(K), int(M)))


def _wws(wplanes, nbytes, device):
    """The weight-plane workspace of a GEMM call -> (buffer, prepared): the caller's prepared buffer (the call is then given
    DDMP_OPT_PREPARED) or scratch."""
    if wplanes is not None:
        if wplanes.numel() < nbytes:
            raise DdmpError("wplanes: %d bytes, the product needs %d" % (wplanes.numel(), nbytes))
        return wplanes, True
    return Workspace.get(nbytes, device), False


def gemm_nt(a, w, out=None, bias=None, pro=None, slope=SLOPE, n_rows=None, wplanes=None, scales=None):
    """out[n,M] = f(a[n,K]) @ w[M,K]^T (+bias)."""
    a, lda = _mat(a, "a")
    w, ldw = _mat(_chk(w, torch.float32, "w"), "w")
    n = a.shape[0] if n_rows is None else n_rows
    K, M = a.shape[1], w.shape[0]
    if w.shape[1] != K:
        raise DdmpError("gemm_nt: inner dimensions differ (%d vs %d)" % (K, w.shape[1]))
    if out is None:
        out = torch.empty((n, M), dtype=a.dtype, device=a.device)
    out, ldy = _mat(out, "out", a)
    ps, psh = (None, None) if pro is None else pro
    L = _lib.lib()
    ws, prep = _wws(wplanes if a.dtype == torch.float32 else None, L.ddmp_gemm_rows_ws_bytes(K, M, _dt(a)), a.device)
    es = a.element_size()
    with _timed("gemm_nt", (K, M), es * n * (K + M) + 4.0 * K * M, 2.0 * n * K * M, survey=es * n * (K + M)):
        o, keep = _mk_opts(None, scales, prep, want_scales=True)
        st = L.ddmp_gemm_nt_o(_p(a), lda, _p(w), ldw, _p(out), ldy, n, K, M, _dt(a), _p(bias), _p(ps), _p(psh),
                              slope, _p(ws), ws.numel(), _stream(), o)
    check(st, "ddmp_gemm_nt")
    return out


def gemm_nt_stats(a, w, sums, out=None, bias=None, pro=None, slope=SLOPE, n_rows=None, wplanes=None, scales=None, bn=None):
    """gemm_nt that also fills ``sums`` (float64 [2M]) with the column sums of out and out^2 (= bn_stats(out)):
    produced in the row-panel kernel's epilogue where that kernel runs, by a separate pass otherwise."""
    if a.dtype == torch.bfloat16:
        # bf16 features: statistics from the row-register kernel's epilogue where that kernel runs (round 3), else the
        # GEMM followed by the streaming statistics pass
        n = a.shape[0] if n_rows is None else n_rows
        K, M = a.shape[1], w.shape[0]
        L = _lib.lib()
        if L.ddmp_gemm_fused_bf16_supported(int(M), int(K), int(n)) & 1:
            a, lda = _mat(a, "a")
            w, ldw = _mat(_chk(w, torch.float32, "w"), "w")
            if out is None:
                out = torch.empty((n, M), dtype=a.dtype, device=a.device)
            out, ldy = _mat(out, "out", a)
            ps, psh = (None, None) if pro is None else pro
            nb = (L.ddmp_gemm_rows_ws_bytes(K, M, _dt(a)) + 255) // 256 * 256
            sb = L.ddmp_gemm_nt_stats_bf16_workspace_bytes(n, M)
            ws = Workspace.get(nb + sb, a.device)
            with _timed("gemm_nt", (K, M), 2.0 * n * (K + M) + 4.0 * K * M, 2.0 * n * K * M, survey=2.0 * n * (K + M)):
                o, keep = _mk_opts(bn, want_bn=True)
                st = L.ddmp_gemm_nt_stats_bf16_o(_p(a), lda, _p(w), ldw, _p(out), ldy, n, K, M, _p(bias), _p(ps), _p(psh), slope,
                                                 _p(sums), _p(ws), nb, ws.data_ptr() + nb, ws.numel() - nb, _stream(), o)
            check(st, "ddmp_gemm_nt_stats_bf16")
            return out
        out = gemm_nt(a, w, out=out, bias=bias, pro=pro, slope=slope, n_rows=n_rows)
        bn_stats(out, sums=sums, n_rows=n_rows, bn=bn)
        return out
    a, lda = _mat(a, "a")
    w, ldw = _mat(w, "w")
    n = a.shape[0] if n_rows is None else n_rows
    K, M = a.shape[1], w.shape[0]
    if w.shape[1] != K:
        raise DdmpError("gemm_nt: inner dimensions differ (%d vs %d)" % (K, w.shape[1]))
    if out is None:
        out = torch.empty((n, M), dtype=torch.float32, device=a.device)
    out, ldy = _mat(out, "out")
    ps, psh = (None, None) if pro is None else pro
    L = _lib.lib()
    nb = (L.ddmp_gemm_rows_workspace_bytes(K, M) + 255) // 256 * 256
    sb = L.ddmp_gemm_nt_stats_workspace_bytes(n, M)
    ws = Workspace.get(nb + sb, a.device)
    wp = ws if wplanes is None else _wws(wplanes, L.ddmp_gemm_rows_workspace_bytes(K, M), a.device)[0]
    with _timed("gemm_nt", (K, M), 4.0 * n * (K + M) + 4.0 * K * M, 2.0 * n * K * M, survey=4.0 * n * (K + M)):
        o, keep = _mk_opts(bn, scales, wplanes is not None, want_bn=True, want_scales=True)
        st = L.ddmp_gemm_nt_stats_f32_o(_p(a), lda, _p(w), ldw, _p(out), ldy, n, K, M, _p(bias), _p(ps), _p(psh), slope,
                                        _p(sums), _p(wp), nb if wplanes is None else wp.numel(), ws.data_ptr() + nb,
                                        ws.numel() - nb, _stream(), o)
    check(st, "ddmp_gemm_nt_stats_f32")
    return out


def gemm_nn(a, w, out=None, n_rows=None, wplanes=None, scales=None):
    """out[n,K] = a[n,M] @ w[M,K]."""
    a, lda = _mat(a, "a")
    w, ldw = _mat(_chk(w, torch.float32, "w"), "w")
    n = a.shape[0] if n_rows is None else n_rows
    M, K = w.shape
    if a.shape[1] != M:
        raise DdmpError("gemm_nn: inner dimensions differ")
    if out is None:
        out = torch.empty((n, K), dtype=a.dtype, device=a.device)
    out, ldy = _mat(out, "out", a)
    L = _lib.lib()
    ws, prep = _wws(wplanes if a.dtype == torch.float32 else None, L.ddmp_gemm_rows_ws_bytes(K, M, _dt(a)), a.device)
    es = a.element_size()
    with _timed("gemm_nn", (M, K), es * n * (K + M) + 4.0 * K * M, 2.0 * n * K * M, survey=es * n * (K + M)):
        o, keep = _mk_opts(None, scales, prep, want_scales=True)
        st = L.ddmp_gemm_nn_o(_p(a), lda, _p(w), ldw, _p(out), ldy, n, M, K, _dt(a), _p(ws), ws.numel(), _stream(), o)
    check(st, "ddmp_gemm_nn")
    return out


def gemm_nn_bnred_supported(M, K, n_rows, dtype=torch.float32):
    """Does gemm_nn_bnred exist for a dgrad M -> K over n_rows rows (row-register kernel, float32 features; the bfloat16 twin
    of round 5 measured no gain inside the step and left the library in round 6: experiments/r05/)?"""
    return dtype == torch.float32 and bool(_lib.lib().ddmp_gemm_nn_bnred_supported(int(M), int(K), int(n_rows)))


def gemm_nn_bnred(a, w, yp, bn4, sums, out=None, slope=SLOPE, n_rows=None, wplanes=None, scales=None, bn=None):
    """out[n,K] = a[n,M] @ w[M,K] AND sums (float64 [2K]) = bn_bwd_reduce(out, yp, bn4): the BatchNorm-backward column
    reductions of `out` as the gradient behind the previous layer's BatchNorm+LeakyReLU (yp: that layer's conv output),
    from the GEMM epilogue -- one read of yp instead of a pass over out and yp."""
    a, lda = _mat(a, "a")
    w, ldw = _mat(_chk(w, torch.float32, "w"), "w")
    yp, ldyp = _mat(yp, "yp", a)
    n = a.shape[0] if n_rows is None else n_rows
    M, K = w.shape
    if out is None:
        out = torch.empty((n, K), dtype=a.dtype, device=a.device)
    out, ldo = _mat(out, "out", a)
    L = _lib.lib()
    if a.dtype != torch.float32:
        raise DdmpError("gemm_nn_bnred: float32 features only")
    nb = (L.ddmp_gemm_rows_workspace_bytes(K, M) + 255) // 256 * 256
    sb = L.ddmp_gemm_nt_stats_workspace_bytes(n, K)
    ws = Workspace.get(nb + sb, a.device)
    wp = ws if wplanes is None else _wws(wplanes, L.ddmp_gemm_rows_workspace_bytes(K, M), a.device)[0]
    with _timed("gemm_nn", (M, K), 4.0 * n * (2 * K + M) + 4.0 * K * M, 2.0 * n * K * M, survey=4.0 * n * (K + M)):
        o, keep = _mk_opts(bn, scales, wplanes is not None, want_bn=True, want_scales=True)
        st = L.ddmp_gemm_nn_bnred_f32_o(_p(a), lda, _p(w), ldw, _p(out), ldo, n, M, K, _p(yp), ldyp, _p(bn4[0]), _p(bn4[1]),
                                        _p(bn4[2]), _p(bn4[3]), slope, _p(sums), _p(wp), nb if wplanes is None else wp.numel(),
                                        ws.data_ptr() + nb, ws.numel() - nb, _stream(), o)
    check(st, "ddmp_gemm_nn_bnred_f32")
    return out


def gemm_tn(g, z, out=None, pro=None, slope=SLOPE, n_rows=None, scales=None):
    """out[M,K] = g[n,M]^T @ f(z[n,K])  (weight gradient)."""
    g, ldg = _mat(g, "g")
    z, ldz = _mat(z, "z", g)
    n = g.shape[0] if n_rows is None else n_rows
    M, K = g.shape[1], z.shape[1]
    if out is None:
        out = torch.empty((M, K), dtype=torch.float32, device=g.device)
    out, ldo = _mat(_chk(out, torch.float32, "out"), "out")
    L = _lib.lib()
    need = L.ddmp_gemm_tn_ws_bytes(n, M, K, _dt(g))
    ws = Workspace.get(need, g.device)
    ps, psh = (None, None) if pro is None else pro
    es = g.element_size()
    with _timed("gemm_tn", (M, K), es * n * (K + M) + 4.0 * K * M, 2.0 * n * K * M, survey=es * n * (K + M)):
        o, keep = _mk_opts(None, scales, want_scales=True)
        st = L.ddmp_gemm_tn_o(_p(g), ldg, _p(z), ldz, _p(out), ldo, n, M, K, _dt(g), _p(ps), _p(psh), slope, _p(ws),
                              ws.numel(), _stream(), o)
    check(st, "ddmp_gemm_tn")
    return out


def gemm_bnbwd_supported(cout, cin, n_rows, dtype=torch.float32):
    """Do the fused BatchNorm-backward GEMMs exist for a layer cin -> cout over n_rows rows in the current GEMM mode?
    (bf16 features: on the row-register kernel, round 3.)"""
    if dtype == torch.bfloat16:
        return bool(_lib.lib().ddmp_gemm_fused_bf16_supported(int(cout), int(cin), int(n_rows)) & 2)
    if dtype != torch.float32:
        return False
    return bool(_lib.lib().ddmp_gemm_bnbwd_supported(int(cout), int(cin), int(n_rows)))


def gemm_tn_bnbwd_supported(cout, cin, n_rows, dtype=torch.float32):
    """Does gemm_tn_bnbwd exist for cin -> cout over n_rows rows (float32 features; the wgrad alone)?"""
    return dtype == torch.float32 and bool(_lib.lib().ddmp_gemm_tn_bnbwd_supported(int(cout), int(cin), int(n_rows)))


ROW_FAMILIES = {1: "f16x3-panel", 2: "bf16-panel", 3: "tiled", 4: "presplit", 5: "plain"}
TN_KERNELS = {1: "f16x3-rowmajor", 2: "bf16-panel", 3: "bf16-tiled", 4: "f32-tiled"}


def gemm_row_route(n_rows, KD, MD, has_pro=False, lda=None, lda2=0, ldy=None, y_misaligned=False):
    """-> (family name, row-register kernel?) of a row product out[n, MD] = f(a[n, KD]) . B in the current GEMM mode
    (ddmp_gemm_row_route; host only).  lda2 > 0: the (dz, yb) operand pair of gemm_nn_bnbwd."""
    r = int(_lib.lib().ddmp_gemm_row_route(int(n_rows), int(KD), int(MD), int(bool(has_pro)), int(KD if lda is None else lda),
                                           int(lda2), int(MD if ldy is None else ldy), int(bool(y_misaligned))))
    check(min(r, 0), "ddmp_gemm_row_route")
    return ROW_FAMILIES[r & 255], bool(r & 256)


def gemm_tn_route(n_rows, M, K, dual=False, ld_ok=True):
    """-> (kernel name, T, tm, tk, n_splits) of a weight gradient out[M, K] over n_rows rows in the current GEMM mode
    (ddmp_gemm_tn_route; host only).  dual: the gemm_tn_bnbwd form; ld_ok: leading dimensions % 4 == 0 and bases on 16 bytes."""
    plan = (ctypes.c_int * 4)()
    r = int(_lib.lib().ddmp_gemm_tn_route(int(n_rows), int(M), int(K), int(bool(dual)), int(bool(ld_ok)),
                                          ctypes.cast(plan, ctypes.c_void_p)))
    check(min(r, 0), "ddmp_gemm_tn_route")
    return (TN_KERNELS[r],) + tuple(plan)


def rows_gather(src, idx, out=None, n_rows=None):
    """out[r] = src[idx[r]] (halo packing on the library's kernel; float32 / bfloat16 rows of 16-byte multiples)."""
    src, lds = _mat(src, "src")
    n = idx.numel() if n_rows is None else n_rows
    if out is None:
        out = torch.empty((n, src.shape[1]), dtype=src.dtype, device=src.device)
    out, ldo = _mat(out, "out", src)
    check(_lib.lib().ddmp_rows_gather(_p(src), lds, _p(_chk(idx, torch.int64, "idx")), n, src.shape[1], _dt(src), _p(out), ldo, 0,
                                      _stream()), "ddmp_rows_gather")
    return out


def to_bf16(src, dst=None):
    """float32 -> bfloat16 (round to nearest even) on the library's kernel."""
    src = _chk(src.contiguous(), torch.float32, "src")
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    check(_lib.lib().ddmp_f32_to_bf16(_p(src), _p(dst), src.numel(), _stream()), "ddmp_f32_to_bf16")
    return dst


def gemm_nn_bnbwd(dz, yb, w, bn4, c10, out=None, slope=SLOPE, n_rows=None, wplanes=None, scales=None):
    """out[n,K] = dY[n,M] @ w[M,K] with dY = BatchNorm+LeakyReLU backward of (dz, yb) computed on the operand load
    (what bn_bwd_apply would have written: a*dz*lrelu'(a*yb+b) + c1*yb + c0)."""
    if dz.dtype == torch.bfloat16:
        dz, lddz = _mat(dz, "dz")
        yb, ldyb = _mat(yb, "yb", dz)
        w, ldw = _mat(_chk(w, torch.float32, "w"), "w")
        n = dz.shape[0] if n_rows is None else n_rows
        M, K = w.shape
        if out is None:
            out = torch.empty((n, K), dtype=dz.dtype, device=dz.device)
        out, ldo = _mat(out, "out", dz)
        L = _lib.lib()
        ws = Workspace.get(L.ddmp_gemm_rows_ws_bytes(K, M, _dt(dz)), dz.device)
        with _timed("gemm_nn", (M, K), 2.0 * n * (K + 2 * M) + 4.0 * K * M, 2.0 * n * K * M, survey=2.0 * n * (K + M)):
            st = L.ddmp_gemm_nn_bnbwd_bf16(_p(dz), lddz, _p(yb), ldyb, _p(w), ldw, _p(out), ldo, n, M, K, _p(bn4[0]), _p(bn4[1]),
                                           _p(c10[0]), _p(c10[1]), slope, _p(ws), ws.numel(), _stream())
        check(st, "ddmp_gemm_nn_bnbwd_bf16")
        return out
    dz, lddz = _mat(dz, "dz")
    yb, ldyb = _mat(yb, "yb")
    w, ldw = _mat(w, "w")
    n = dz.shape[0] if n_rows is None else n_rows
    M, K = w.shape
    if out is None:
        out = torch.empty((n, K), dtype=torch.float32, device=dz.device)
    out, ldo = _mat(out, "out")
    L = _lib.lib()
    ws, prep = _wws(wplanes, L.ddmp_gemm_rows_workspace_bytes(K, M), dz.device)
    with _timed("gemm_nn", (M, K), 4.0 * n * (K + 2 * M) + 4.0 * K * M, 2.0 * n * K * M, survey=4.0 * n * (K + M)):
        o, keep = _mk_opts(None, scales, prep, want_scales=True)
        st = L.ddmp_gemm_nn_bnbwd_f32_o(_p(dz), lddz, _p(yb), ldyb, _p(w), ldw, _p(out), ldo, n, M, K, _p(bn4[0]), _p(bn4[1]),
                                        _p(c10[0]), _p(c10[1]), slope, _p(ws), ws.numel(), _stream(), o)
    check(st, "ddmp_gemm_nn_bnbwd_f32")
    return out


def gemm_tn_bnbwd(dz, yb, z, bn4, c10, out=None, pro=None, slope=SLOPE, n_rows=None, scales=None):
    """out[M,K] = dY^T @ f(z) with dY as in gemm_nn_bnbwd."""
    if dz.dtype == torch.bfloat16:
        dz, lddz = _mat(dz, "dz")
        yb, ldyb = _mat(yb, "yb", dz)
        z, ldz = _mat(z, "z", dz)
        n = dz.shape[0] if n_rows is None else n_rows
        M, K = yb.shape[1], z.shape[1]
        if out is None:
            out = torch.empty((M, K), dtype=torch.float32, device=dz.device)
        out, ldo = _mat(_chk(out, torch.float32, "out"), "out")
        L = _lib.lib()
        ws = Workspace.get(L.ddmp_gemm_tn_ws_bytes(n, M, K, _dt(dz)), dz.device)
        ps, psh = (None, None) if pro is None else pro
        with _timed("gemm_tn", (M, K), 2.0 * n * (K + 2 * M) + 4.0 * K * M, 2.0 * n * K * M, survey=2.0 * n * (K + M)):
            st = L.ddmp_gemm_tn_bnbwd_bf16(_p(dz), lddz, _p(yb), ldyb, _p(z), ldz, _p(out), ldo, n, M, K, _p(bn4[0]), _p(bn4[1]),
                                           _p(c10[0]), _p(c10[1]), _p(ps), _p(psh), slope, _p(ws), ws.numel(), _stream())
        check(st, "ddmp_gemm_tn_bnbwd_bf16")
        return out
    dz, lddz = _mat(dz, "dz")
    yb, ldyb = _mat(yb, "yb")
    z, ldz = _mat(z, "z")
    n = dz.shape[0] if n_rows is None else n_rows
    M, K = yb.shape[1], z.shape[1]
    if out is None:
        out = torch.empty((M, K), dtype=torch.float32, device=dz.device)
    out, ldo = _mat(out, "out")
    L = _lib.lib()
    ws = Workspace.get(L.ddmp_gemm_tn_workspace_bytes(n, M, K), dz.device)
    ps, psh = (None, None) if pro is None else pro
    with _timed("gemm_tn", (M, K), 4.0 * n * (K + 2 * M) + 4.0 * K * M, 2.0 * n * K * M, survey=4.0 * n * (K + M)):
        o, keep = _mk_opts(None, scales, want_scales=True)
        st = L.ddmp_gemm_tn_bnbwd_f32_o(_p(dz), lddz, _p(yb), ldyb, _p(z), ldz, _p(out), ldo, n, M, K, _p(bn4[0]), _p(bn4[1]),
                                        _p(c10[0]), _p(c10[1]), _p(ps), _p(psh), slope, _p(ws), ws.numel(), _stream(), o)
    check(st, "ddmp_gemm_tn_bnbwd_f32")
    return out


def _colws(n, C, device):
    need = _lib.lib().ddmp_colreduce_workspace_bytes(n, C)
    if need == 0:
        raise DdmpError("column reduction: unsupported width %d (power of two in [8,1024])" % C)
    return Workspace.get(need, device)


def bn_stats(y, sums=None, n_rows=None, bn=None):
    """-> float64 [2C] = (column sums, column sums of squares) of y[:n_rows]."""
    y, ldy = _mat(y, "y")
    n = y.shape[0] if n_rows is None else n_rows
    C = y.shape[1]
    if sums is None:
        sums = torch.empty(2 * C, dtype=torch.float64, device=y.device)
    ws = _colws(n, C, y.device)
    with _timed("bn_stats", C, float(y.element_size()) * n * C):
        o, keep = _mk_opts(bn, want_bn=True)
        st = _lib.lib().ddmp_bn_stats_o(_p(y), ldy, n, C, _dt(y), _p(sums), _p(ws), ws.numel(), _stream(), o)
    check(st, "ddmp_bn_stats")
    return sums


def bn_prepare(sums, n_total, gamma, beta, out4, running=None, eps=BN_EPS, momentum=BN_MOMENTUM):
    """out4: float32 [4,C] rows = scale, shift, mean, rstd (written)."""
    C = gamma.numel()
    rm, rv = (None, None) if running is None else running
    st = _lib.lib().ddmp_bn_prepare_f32(_p(sums), float(n_total), C, _p(gamma), _p(beta), eps, momentum,
                                        _p(out4[0]), _p(out4[1]), _p(out4[2]), _p(out4[3]), _p(rm), _p(rv), _stream())
    check(st, "ddmp_bn_prepare_f32")
    return out4


def bn_lrelu_apply(y, scale, shift, out=None, slope=SLOPE):
    y, ldy = _mat(y, "y")
    if out is None:
        out = torch.empty_like(y)
    out, ldz = _mat(out, "out", y)
    fn = _lib.lib().ddmp_bn_lrelu_apply_bf16 if y.dtype == torch.bfloat16 else _lib.lib().ddmp_bn_lrelu_apply_f32
    st = fn(_p(y), ldy, _p(out), ldz, y.shape[0], y.shape[1], _p(scale), _p(shift), slope, _stream())
    check(st, "ddmp_bn_lrelu_apply")
    return out


def bn_bwd_reduce(dz, y, bn4, sums2=None, slope=SLOPE, n_rows=None, bn=None):
    dz, lddz = _mat(dz, "dz")
    y, ldy = _mat(y, "y", dz)
    n = y.shape[0] if n_rows is None else n_rows
    C = y.shape[1]
    if sums2 is None:
        sums2 = torch.empty(2 * C, dtype=torch.float64, device=y.device)
    ws = _colws(n, C, y.device)
    with _timed("bn_bwd_reduce", C, 2.0 * y.element_size() * n * C):
        o, keep = _mk_opts(bn, want_bn=True)
        st = _lib.lib().ddmp_bn_bwd_reduce_o(_p(dz), lddz, _p(y), ldy, n, C, _dt(y), _p(bn4[0]), _p(bn4[1]), _p(bn4[2]),
                                             _p(bn4[3]), slope, _p(sums2), _p(ws), ws.numel(), _stream(), o)
    check(st, "ddmp_bn_bwd_reduce")
    return sums2


def bn_bwd_prepare(sums2, n_total, bn4, dgamma, dbeta, c10):
    """c10: float32 [2,C] rows = c1, c0 (written)."""
    C = dgamma.numel()
    st = _lib.lib().ddmp_bn_bwd_prepare_f32(_p(sums2), float(n_total), C, _p(bn4[0]), _p(bn4[2]), _p(bn4[3]),
                                            _p(dgamma), _p(dbeta), _p(c10[0]), _p(c10[1]), _stream())
    check(st, "ddmp_bn_bwd_prepare_f32")


def bn_bwd_apply(dz, y, bn4, c10, dy, dbias_sums, slope=SLOPE, n_rows=None):
    """dy = BatchNorm+LeakyReLU backward of (dz, y); dbias_sums (float64 [C]): its column sums, None: not computed."""
    dz, lddz = _mat(dz, "dz")
    y, ldy = _mat(y, "y", dz)
    dy, lddy = _mat(dy, "dy", dz)
    n = y.shape[0] if n_rows is None else n_rows
    C = y.shape[1]
    ws = _colws(n, C, y.device)
    with _timed("bn_bwd_apply", C, 3.0 * y.element_size() * n * C):
        st = _lib.lib().ddmp_bn_bwd_apply(_p(dz), lddz, _p(y), ldy, _p(dy), lddy, n, C, _dt(y), _p(bn4[0]), _p(bn4[1]),
                                          _p(c10[0]), _p(c10[1]), slope, _p(dbias_sums), _p(ws), ws.numel(),
                                          _stream())
    check(st, "ddmp_bn_bwd_apply")
    return dy


def colsum(x, sums=None, n_rows=None):
    x, ldx = _mat(x, "x")
    n = x.shape[0] if n_rows is None else n_rows
    C = x.shape[1]
    if sums is None:
        sums = torch.empty(C, dtype=torch.float64, device=x.device)
    ws = _colws(n, C, x.device)
    st = _lib.lib().ddmp_colsum_f32(_p(x), ldx, n, C, _p(sums), _p(ws), ws.numel(), _stream())
    check(st, "ddmp_colsum_f32")
    return sums


def f64_to_f32(src, dst):
    st = _lib.lib().ddmp_f64_to_f32(_p(src), _p(dst), src.numel(), _stream())
    check(st, "ddmp_f64_to_f32")
    return dst


def head_fwd(y, bn4, W1, b1, W2, b2, kind, x_pos, out, slope=SLOPE, n_rows=None):
    y, ldy = _mat(y, "y")
    n = y.shape[0] if n_rows is None else n_rows
    with _timed("head_fwd", kind, n * (32.0 * y.element_size() + 12 + (12 if kind == 0 else 0))):
        st = _lib.lib().ddmp_head_fwd(_p(y), ldy, n, _dt(y), _p(bn4[0]), _p(bn4[1]), slope, _p(W1), _p(b1), _p(W2),
                                      _p(b2), kind, _p(x_pos), _p(out), _stream())
    check(st, "ddmp_head_fwd")
    return out


def head_bwd(y, bn4, W1, b1, W2, b2, kind, dout, dz, dW1, db1, dW2, db2, slope=SLOPE, n_rows=None):
    y, ldy = _mat(y, "y")
    dz, lddz = _mat(dz, "dz", y)
    n = y.shape[0] if n_rows is None else n_rows
    L = _lib.lib()
    ws = Workspace.get(L.ddmp_head_bwd_workspace_bytes(n), y.device)
    with _timed("head_bwd", kind, n * (64.0 * y.element_size() + 12)):
        st = L.ddmp_head_bwd(_p(y), ldy, n, _dt(y), _p(bn4[0]), _p(bn4[1]), slope, _p(W1), _p(b1), _p(W2), _p(b2), kind,
                             _p(dout), _p(dz), lddz, _p(dW1), _p(db1), _p(dW2), _p(db2), _p(ws), ws.numel(),
                             _stream())
    check(st, "ddmp_head_bwd")


def grad_sumsq(g, out=None):
    L = _lib.lib()
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=g.device)
    ws = Workspace.get(L.ddmp_sumsq_workspace_bytes(), g.device)
    with _timed("optimizer", "sumsq", 4.0 * g.numel()):
        st = L.ddmp_grad_sumsq_f32(_p(g), g.numel(), _p(out), _p(ws), ws.numel(), _stream())
    check(st, "ddmp_grad_sumsq_f32")
    return out


def grad_clip_(g, sumsq, max_norm):
    st = _lib.lib().ddmp_grad_clip_f32(_p(g), g.numel(), _p(sumsq), float(max_norm), _stream())
    check(st, "ddmp_grad_clip_f32")


def adam_step_(p, g, m, v, lr, step, betas=(0.9, 0.999), eps=1e-8, clip_sumsq=None, max_norm=0.0):
    with _timed("optimizer", "adam", 28.0 * p.numel()):
        st = _lib.lib().ddmp_adam_step_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), betas[0], betas[1], eps,
                                           int(step), _p(clip_sumsq), float(max_norm), _stream())
    check(st, "ddmp_adam_step_f32")


def adam_prepare(counter, lr, coef, betas=(0.9, 0.999)):
    """device-side: counter += 1; coef = (lr / (1 - b1^t), sqrt(1 - b2^t))  (int32 [1], float32 [2])."""
    check(_lib.lib().ddmp_adam_prepare(_p(counter), float(lr), betas[0], betas[1], _p(coef), _stream()), "ddmp_adam_prepare")


def adam_step_dev_(p, g, m, v, coef, betas=(0.9, 0.999), eps=1e-8, clip_sumsq=None, max_norm=0.0):
    with _timed("optimizer", "adam", 28.0 * p.numel()):
        st = _lib.lib().ddmp_adam_step_dev_f32(_p(p), _p(g), _p(m), _p(v), p.numel(), betas[0], betas[1], eps, _p(coef),
                                               _p(clip_sumsq), float(max_norm), _stream())
    check(st, "ddmp_adam_step_dev_f32")

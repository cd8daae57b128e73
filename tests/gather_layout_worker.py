"""Runner of tests/test_gpu_gather_layouts.py, and its worker process: every entry point of the gather on operands that are column
blocks of wider buffers (tests/gather_layout_cases.py), under the environment the process was started with -- the library reads
DDMP_SPMM_LEAN / DDMP_SPMM_PATCH once per process, hence a process per setting.

For each (entry point, graph, width, dtype): the contiguous call against float64 at the project's bounds; then every layout --
the route from the library's own selection queries (asked with the call's actual leading dimensions) must be what
gather_layout_cases.expected_route says; where it is the contiguous call's route the output block and the float64 sums are BITWISE
the contiguous call's, else they meet the float64 bound; everything outside the output block keeps the sentinel's bits, every
input buffer (NaN outside its block) is bit-identical to its copy; a refusal raises DdmpError and leaves every buffer untouched.
One line per layout is printed.

As a program: ``python gather_layout_worker.py OUT.npz`` runs the table restricted to "ico", "hub", "rcbhub" and widths 32, 96,
128, asserts the route the environment names and writes the contiguous calls' outputs to OUT.npz."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gather_layout_cases as K   # noqa: E402

NAN = float("nan")
DEFAULT_CONFIG = not any(k.startswith("DDMP_") and k != "DDMP_LIB" for k in os.environ)
RESTRICTED_WIDTHS = (32, 96, 128)
ALIGNED_LAYOUTS = ("contig", "block", "mixed", "mixed-rot", "mixed-same-in")


def relerr(a, b):
    a, b = a.double(), b.double().to(a.device)
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Gr:
    """A graph under test: the device handle, its float64 operator (``mm``; valued graphs: ``mm_t`` too) and, for sddmm, its CSR."""

    def __init__(self, name, handle, n, n_cols, mm, mm_t=None, csr=None, keep=None):
        self.name, self.g, self.n, self.n_cols, self.mm, self.mm_t, self.csr, self._keep = name, handle, n, n_cols, mm, mm_t, csr, keep
        self.valued = mm_t is not None


def _sparse_mm(A):
    return lambda x: torch.sparse.mm(A, x)


def mesh_graph(dev, name):
    from dual_dmp_amd import ops
    ei, n = K.mesh_edges()[name]
    rowptr, col, dinv = ops.csr_build_host(ei.numpy(), n)
    eid = ei.to(dev)
    return Gr(name, ops.graph_for(eid, n), n, n, _sparse_mm(K.sparse_operator(rowptr, col, dinv, n)), keep=eid)


def valued_graph(dev, name):
    from dual_dmp_amd import ops
    from edge_weight_route_worker import weights
    from gcnw_ref import dense_gcn_norm
    ei, n = K.mesh_edges()[name]
    w = weights(ei.shape[1], n)
    A = dense_gcn_norm(ei, w, n)
    At = A.t().contiguous()
    eid, wd = ei.to(dev), w.to(dev)
    g = ops.graph_for(eid, n, edge_weight=wd)
    assert g.valued
    t = ops.csr_build_valued_host(ei.numpy(), n, ops.valued_flags())
    return Gr(name, g, n, n, lambda x: A @ x, lambda x: At @ x, csr=(t["rowptr"], t["col"]), keep=(eid, wd))


def csr_graph(dev, name):
    from dual_dmp_amd import ops
    rowptr, col, dinv, nc = {"star": K.star_csr, "split70k": K.split70k_csr, "band70k": K.band70k_csr, "ring70k": K.ring70k_csr}[name]()
    return Gr(name, ops.Graph.from_csr_host(rowptr, col, dinv, nc), len(rowptr) - 1, nc,
              _sparse_mm(K.sparse_operator(rowptr, col, dinv, nc)), csr=(rowptr, col))


def patch_info(gr):
    from dual_dmp_amd import _lib
    kd, heavy, split = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().ddmp_graph_patch_info(gr.g.handle, ctypes.byref(kd), ctypes.byref(heavy), ctypes.byref(split)) == 0
    return kd.value, heavy.value, split.value


def answers(gr, entry, C, dtype, lay):
    """The library's selection queries for this call, as plain values (see gather_layout_cases.expected_route)."""
    from dual_dmp_amd import _lib
    L, h = _lib.lib(), gr.g.handle
    bf = dtype == torch.bfloat16
    if bf:
        lean = L.ddmp_spmm_lean_selected(h, 32, 32, 32)
    elif entry == "sddmm":
        lean = 0
    else:
        ldy = lay[2][0] if entry == "bnbwd" else lay[1][0]
        lean = L.ddmp_spmm_lean_selected(h, lay[0][0], ldy, C)
    form = K.PATCH_FORM[entry]
    patch = L.ddmp_spmm_patch_selected(h, C, 1 if bf else 0, form[0], form[1]) if form else 0
    return dict(lean=int(lean), patch=int(patch), n_heavy=patch_info(gr)[1])


class Buf:
    """The column block [off, off + C) of a [rows + PAD_ROWS, ld] buffer: NaN (inputs) or the sentinel (outputs) outside."""

    def __init__(self, data, rows, C, ld, off, dtype, dev, role):
        self.role, self.rows, self.C, self.off = role, rows, C, off
        self.buf = torch.full((rows + K.PAD_ROWS, ld), K.SENTINEL if role == "out" else NAN, dtype=dtype, device=dev)
        self.view = self.buf[:rows, off:off + C]
        if data is not None:
            self.view.copy_(data)
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(bits(self.buf), bits(self.before))

    def outside_unchanged(self):
        a, b = self.buf.clone(), self.before.clone()
        for t in (a, b):
            t[:self.rows, self.off:self.off + self.C] = 0
        return torch.equal(bits(a), bits(b))


class Coef:
    """A per-column float32 vector, `off` elements into its own [C + off] buffer."""

    def __init__(self, v, off):
        self.buf = torch.full((v.numel() + off,), NAN, dtype=torch.float32, device=v.device)
        self.view = self.buf[off:]
        self.view.copy_(v)
        self.before = self.buf.clone()

    def unchanged(self):
        return torch.equal(bits(self.buf), bits(self.before))


def _call(entry, gr, v, cf, C, dev):
    """-> (output tensor, float64 sums or None)"""
    from dual_dmp_amd import ops
    g = gr.g
    sums = None
    if entry in ("spmm", "v_spmm"):
        ops.spmm(g, v["x"], out=v["out"])
    elif entry == "v_spmm_t":
        ops.spmm(g, v["x"], out=v["out"], transpose=True)
    elif entry == "spmm+bias":
        ops.spmm(g, v["x"], out=v["out"], bias=cf["bias"])
    elif entry == "spmm+pro+bias":
        ops.spmm(g, v["x"], out=v["out"], bias=cf["bias"], pro=(cf["a"], cf["b"]))
    elif entry == "stats":
        sums = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        ops.spmm_stats(g, v["x"], v["out"], cf["ref"], sums, bias=cf["bias"], pro=(cf["a"], cf["b"]))
    elif entry == "bnred":
        sums = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        ops.spmm_bnred(g, v["x"], v["out"], v["yp"], cf["bn4"], sums)
    elif entry == "bnbwd":
        ops.spmm_bnbwd(g, v["dz"], v["yb"], cf["bn4"], cf["c10"], v["out"])
    elif entry == "axpby_z":
        ops.spmm_axpby(g, v["x"], out=v["out"], z=v["z"], a=K.AXPBY["a"], b=K.AXPBY["b"], c=K.AXPBY["c"])
    elif entry == "axpby_z_z2":
        ops.spmm_axpby(g, v["x"], out=v["out"], z=v["z"], z2=v["z2"], **K.AXPBY)
    elif entry == "axpby_alias":
        ops.spmm_axpby(g, v["x"], out=v["z"], z=v["z"], a=K.AXPBY["a"], b=K.AXPBY["b"], c=K.AXPBY["c"])
        return v["z"], None
    elif entry == "sddmm":
        ops.sddmm(g, v["dy"], v["h"], out=v["G"])
        return v["G"], None
    else:
        raise KeyError(entry)
    return v["out"], sums


class Result:
    def __init__(self, route, out, sums, err):
        self.route, self.out, self.sums, self.err = route, out, sums, err


def run_layout(dev, gr, entry, C, dtype, lname, inp, dinp, ref, base=None, say=print):
    """One call in layout `lname` with every assertion of the module docstring.  base: the contiguous call's Result (None: this IS
    the contiguous call, or that one was refused).  -> Result, or None for a layout that does not apply / a refusal."""
    from dual_dmp_amd._lib import DdmpError
    got = K.layout(lname, entry, C, dtype)
    if got is None:
        return None
    lay, coef_off = got
    dt = "bf16" if dtype == torch.bfloat16 else "f32"
    route = K.expected_route(entry, C, dtype, lay, coef_off, gr.n_cols, **answers(gr, entry, C, dtype, lay))
    key = (entry, gr.name, C, dt, lname)
    if DEFAULT_CONFIG and key in K.LISTED:
        assert route[0] == K.LISTED[key][1], (key, route, K.LISTED[key])
    tag = "%-13s %-8s C=%-3d %s %-15s %-13s" % (entry, gr.name, C, dt, route[0] + ("/" + route[1] if route[1] else ""), lname)
    bufs = {}
    for (name, kind, role), (ld, off) in zip(K.OPERANDS[entry], lay):
        rows = gr.n_cols if kind == "cols" else gr.n
        bufs[name] = Buf(None if role == "out" else dinp[name], rows, C, ld, off, dtype, dev, role)
    v = {k: b.view for k, b in bufs.items()}
    if entry == "sddmm":
        nnz = gr.g.nnz
        gbuf = torch.full((nnz + K.PAD_ROWS,), K.SENTINEL, dtype=torch.float32, device=dev)
        v["G"] = gbuf[:nnz]
    coefs = {}
    if entry in K.HAS_COEF:
        for k in ("bias", "a", "b", "ref"):
            coefs[k] = Coef(dinp[k], coef_off)
        coefs["bn4"] = [Coef(dinp["bn4"][i], coef_off) for i in range(4)]
        coefs["c10"] = [Coef(dinp["c10"][i], coef_off) for i in range(2)]
    cf = {k: ([c.view for c in x] if isinstance(x, list) else x.view) for k, x in coefs.items()}
    flat = [c for x in coefs.values() for c in (x if isinstance(x, list) else [x])]
    if route[0] == "refused":
        with pytest.raises(DdmpError):
            _call(entry, gr, v, cf, C, dev)
        torch.cuda.synchronize()
        assert all(b.unchanged() for b in bufs.values()) and all(c.unchanged() for c in flat), (tag, "a refused call wrote")
        say("gather layout %s refused (DdmpError), buffers untouched" % tag, flush=True)
        return None
    out, sums = _call(entry, gr, v, cf, C, dev)
    for name, b in bufs.items():
        if b.role == "in":
            assert b.unchanged(), (tag, "input buffer changed", name)
        else:
            assert b.outside_unchanged(), (tag, "written outside the operand", name)
    assert all(c.unchanged() for c in flat), (tag, "a per-column vector changed")
    if entry == "sddmm":
        assert bool((gbuf[nnz:] == K.SENTINEL).all()), (tag, "written behind the entries")
    bound = K.SDDMM_BOUND if entry == "sddmm" else K.out_bound(gr.name, dtype)
    err = relerr(out, ref)
    same = base is not None and base.route == route
    if same:
        assert torch.equal(bits(out.contiguous()), bits(base.out)), (tag, "differs from the contiguous call on the same route", err)
        if sums is not None:
            assert torch.equal(sums, base.sums), (tag, "sums differ from the contiguous call's on the same route")
    esum = None
    if sums is not None:
        want = K.stats_sums(out) if entry == "stats" else K.bnred_sums(out, inp)
        esum = relerr(sums.cpu(), want)
    say("gather layout %s rel-L2 %.2e%s%s" % (tag, err, "" if esum is None else " sums %.2e" % esum,
                                              " == contiguous bit for bit" if same else ""), flush=True)
    assert err < bound, (tag, err, bound)
    if esum is not None:
        assert esum < K.SUMS_BOUND[entry], (tag, esum)
    return Result(route, out.contiguous().clone() if base is None else None, sums, err)


def run_width(dev, gr, C, dtype, entries, layouts, keep=None, say=print, seed=0):
    """Every entry of `entries` that applies on graph `gr` at width C: the contiguous call, then every layout of `layouts`.
    keep: dict that receives the contiguous outputs (CPU numpy bits).  -> {(entry, layout): Result}"""
    inp = K.inputs(gr.n, gr.n_cols, C, dtype, seed)
    res = {}
    dt = "bf16" if dtype == torch.bfloat16 else "f32"
    for entry in entries:
        if not K.entry_applies(entry, C, dtype, gr.n == gr.n_cols):
            continue
        if entry == "sddmm":
            ref = K.sddmm_reference(gr.csr[0], gr.csr[1], inp)
        else:
            ref = K.reference(entry, gr.mm, inp, gr.mm_t)
        dinp = {k: t.to(dev) for k, t in inp.items()}
        dinp["ref"] = (ref.mean(0) * 1.01).float().to(dev) if ref.dim() == 2 else dinp["bias"]
        refd = ref.to(dev)
        base = run_layout(dev, gr, entry, C, dtype, "contig", inp, dinp, refd, None, say)
        res[(entry, "contig")] = base
        if keep is not None and base is not None:
            keep["%s|%s|%d|%s" % (entry, gr.name, C, dt)] = bits(base.out).cpu().numpy()
        for lname in layouts:
            r = run_layout(dev, gr, entry, C, dtype, lname, inp, dinp, refd, base, say)
            if r is not None or K.layout(lname, entry, C, dtype) is not None:
                res[(entry, lname)] = r
    return res


def run_restricted(dev, keep=None, say=print):
    """The table on "ico", "hub", "rcbhub" at widths 32, 96, 128: float32 (unvalued and valued graphs) and bfloat16.  Asserts the
    route the environment names."""
    forced_patch, forced_slab = os.environ.get("DDMP_SPMM_PATCH") == "1", os.environ.get("DDMP_SPMM_LEAN") == "0"
    for name in K.MESH_GRAPHS:
        plain = mesh_graph(dev, name)
        for gr, entries, dtype, layouts in ((plain, K.F32_ENTRIES, torch.float32, K.F32_LAYOUTS),
                                            (valued_graph(dev, name), K.VALUED_ENTRIES, torch.float32, K.F32_LAYOUTS),
                                            (plain, K.BF16_ENTRIES, torch.bfloat16, K.BF16_LAYOUTS)):
            for C in RESTRICTED_WIDTHS:
                res = run_width(dev, gr, C, dtype, entries, layouts, keep, say)
                for (entry, lname), r in res.items():
                    if r is None or lname not in ALIGNED_LAYOUTS or entry == "sddmm":
                        continue
                    named = r.route[1].split("+")[0] if r.route[0] == "composition" else r.route[0]
                    if forced_slab:
                        assert named == "slab", (entry, name, C, lname, r.route)
                    if forced_patch and name == "rcbhub" and C == 128 and entry in ("spmm", "spmm+bias", "v_spmm") and dtype == torch.float32:
                        assert r.route[0] == "patch+lean-list", (entry, name, C, lname, r.route)


if __name__ == "__main__":
    kept = {}
    run_restricted(torch.device("cuda:0"), kept)
    np.savez(sys.argv[1], **kept)

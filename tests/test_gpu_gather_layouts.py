"""Every route and fused form of the gather on blocked and offset operands (tests/gather_layout_cases.py, run by
tests/gather_layout_worker.py).

Every other GPU test of the gather hands it contiguous [n, C] tensors with ld = C; the multi-device path, the ChebConv drop-in and
callers of the C ABI hand it column blocks of wider buffers, and WHICH kernel runs is decided from the operands' leading dimensions
and alignment.  Here every operand is the column block [off, off + C) of a [rows + 3, ld] buffer that holds NaN (inputs) or the
sentinel -7.25 (outputs) outside the block, every entry point has a layout in which all of its leading dimensions differ, and for
each (entry point, graph, width, layout, dtype):

  1. the contiguous call meets the project's bounds against float64 (outputs 1e-6, 2e-6 on "star", 3e-6 on the 70k graphs;
     statistic sums 2e-6, reduction sums 2e-5, sddmm 1e-6, bfloat16 outputs 4e-3: test_gpu_irregular.py, test_gpu_edge_weight.py);
  2. the route, from ddmp_spmm_lean_selected asked with the call's OWN leading dimensions, ddmp_spmm_patch_selected and
     ddmp_graph_patch_info, is what gather_layout_cases.expected_route derives from the dispatch rules;
  3. where that is the contiguous call's route, output block and float64 sums are BITWISE the contiguous call's (a row's entries are
     summed in CSR order whatever the stride); else (odd-*: scalar kernel / composition; `mixed` on spmm_bnbwd: slab kernel) they
     meet the bound of (1);
  4. nothing outside the output block is written, no input buffer changes;
  5. a refusal (float32 spmm_bnbwd on odd-* operands and below C = 32; bfloat16 on a leading dimension that is no multiple of 8 or an
     operand 8 bytes off) raises DdmpError and leaves every buffer untouched.

Run with -s for one line per layout.  Under DDMP_SPMM_LEAN=0 / DDMP_SPMM_PATCH=0|1 set from outside the same assertions hold with
the routes those switches select; the cases that name a route of the default configuration skip.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gather_layout_cases as K
import gather_layout_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_CONFIG = W.DEFAULT_CONFIG
F32, BF16 = torch.float32, torch.bfloat16


def supported(answer, what):
    """A route that the configuration does not select: a failure in the default configuration, a skip under a switch."""
    if not answer:
        assert not DEFAULT_CONFIG, "%s not selected in the default configuration" % what
        pytest.skip("%s switched off in this configuration" % what)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graphs(dev):
    """name -> Gr, built on first use and once per module (the two 70k graphs among them)."""
    made = {}

    def get(name, valued=False):
        key = (name, valued)
        if key not in made:
            made[key] = (W.valued_graph(dev, name) if valued else
                         W.mesh_graph(dev, name) if name in K.MESH_GRAPHS else W.csr_graph(dev, name))
        return made[key]
    return get


@pytest.mark.parametrize("C", K.F32_WIDTHS)
@pytest.mark.parametrize("gname", K.GRAPHS)
def test_float32_forms_on_blocks_of_wider_buffers(dev, graphs, gname, C):
    res = W.run_width(dev, graphs(gname), C, F32, K.F32_ENTRIES, K.F32_LAYOUTS)
    assert sum(r is not None for r in res.values()) >= 20


@pytest.mark.parametrize("C", K.BF16_WIDTHS)
@pytest.mark.parametrize("gname", K.GRAPHS)
def test_bfloat16_forms_on_blocks_of_wider_buffers(dev, graphs, gname, C):
    res = W.run_width(dev, graphs(gname), C, BF16, K.BF16_ENTRIES, K.BF16_LAYOUTS)
    assert sum(r is not None for r in res.values()) >= 9
    assert all(res[(e, l)] is None for e, l in res if l.startswith("bf16-"))        # the refusals were refusals


@pytest.mark.parametrize("C", K.F32_WIDTHS)
@pytest.mark.parametrize("gname", K.MESH_GRAPHS)
def test_valued_gather_transpose_and_sddmm_on_blocks_of_wider_buffers(dev, graphs, gname, C):
    res = W.run_width(dev, graphs(gname, valued=True), C, F32, K.VALUED_ENTRIES, K.F32_LAYOUTS)
    assert sum(r is not None for r in res.values()) >= 15


def test_default_routes_of_the_70k_graphs(dev, graphs):
    """"split70k" gets patch tables with patch_kd = 3, one heavy chunk and four split slots: the patch kernel, its split records and
    the lean heavy list all run in the cases above; "band70k" gets tables without a heavy chunk."""
    if not DEFAULT_CONFIG:
        pytest.skip("names the default configuration's routes")
    assert W.patch_info(graphs("split70k")) == (3, 1, 4)
    assert W.patch_info(graphs("band70k"))[1:] == (0, 0)
    for name in K.MESH_GRAPHS + ("star",):
        lay = K.layout("block", "spmm", 128, F32)[0]
        assert W.answers(graphs(name), "spmm", 128, F32, lay) == dict(lean=1, patch=0, n_heavy=0), name


def test_patch_kernel_without_a_heavy_list(dev, graphs):
    """The LDS-patch kernel alone ("band70k": patch tables, no heavy chunk, no lean launch beside it): plain, the fused reductions
    and the BatchNorm backward on the gather, whose patch form carries ldyb of its own -- `mixed` stays on the patch kernel."""
    gr = graphs("band70k")
    lay = K.layout("block", "spmm", 128, F32)[0]
    supported(W.answers(gr, "spmm", 128, F32, lay)["patch"], "the LDS-patch gather")
    res = W.run_width(dev, gr, 128, F32, ("spmm", "stats", "bnred", "bnbwd"), ("block", "mixed", "mixed-same-in"))
    for (entry, lname), r in res.items():      # (without the lean gather spmm_stats is a composition: its fused form needs lean_plan)
        assert r.route == ("patch", None) or (entry == "stats" and not DEFAULT_CONFIG), (entry, lname, r.route)


def test_scalar_kernel_past_one_grid_pass(dev, graphs):
    """The scalar kernel's grid is capped at 4096 workgroups of 256 threads: ring70k x 20 = 1,400,000 elements need a second pass of
    its grid-stride loop.  Plain, prologue + bias and the affine form, contiguous and `block` (bitwise equal), against float64 at
    3e-6; and C = 3 with an operand 4 bytes off."""
    gr = graphs("ring70k")
    assert gr.n * 20 > K.SCALAR_GRID_ELEMS
    entries = ("spmm", "spmm+pro+bias", "axpby_z")
    res = W.run_width(dev, gr, 20, F32, entries, ("block",))
    for e in entries:
        assert res[(e, "contig")].route == res[(e, "block")].route == ("scalar", None)
    res = W.run_width(dev, gr, 3, F32, entries, ("odd-off",))
    assert all(r.route == ("scalar", None) for r in res.values())


def test_byte_offsets_beyond_2_to_the_32(dev, graphs):
    """The lean gather forms its addresses from 32-bit products in 16-BYTE units: x is the last 32 columns of a [n_cols + 3, 16384]
    float32 buffer (4.6 GB, row offsets up to 4.61e9 bytes), the output in `block` layout; plain, then spmm_bnred; against float64
    and bitwise against the contiguous call.  The same in bfloat16 with ld = 32768.  (The input-unchanged check is made on the
    block's rows only: no second 4.6 GB copy.)"""
    from dual_dmp_amd import ops
    gr = graphs("split70k")
    C = 32
    for dtype, ld in ((F32, 16384), (BF16, 32768)):
        inp = K.inputs(gr.n, gr.n_cols, C, dtype, seed=1)
        ref = K.reference("spmm", gr.mm, inp)
        lay = [(ld, ld - C), K.layout("block", "spmm", C, dtype)[0][1]]
        assert (gr.n_cols - 1) * ld * inp["x"].element_size() > 1 << 32
        route = K.expected_route("spmm", C, dtype, lay, 0, gr.n_cols, **W.answers(gr, "spmm", C, dtype, lay))
        contig = K.expected_route("spmm", C, dtype, [(C, 0), (C, 0)], 0, gr.n_cols,
                                  **W.answers(gr, "spmm", C, dtype, [(C, 0), (C, 0)]))
        if DEFAULT_CONFIG:
            assert route == ("lean", None)
        xd = inp["x"].to(dev)
        big = torch.full((gr.n_cols + K.PAD_ROWS, ld), W.NAN, dtype=dtype, device=dev)
        xv = big[:gr.n_cols, ld - C:]
        xv.copy_(xd)
        try:
            y0 = ops.spmm(gr.g, xd)
            out = W.Buf(None, gr.n, C, lay[1][0], lay[1][1], dtype, dev, "out")
            ops.spmm(gr.g, xv, out=out.view)
            e = W.relerr(out.view, ref)
            print("gather layout spmm          split70k C=32 %s %s x in [%d, %d] (%.2f GB) rel-L2 %.2e"
                  % (dtype, route[0], big.shape[0], ld, big.numel() * big.element_size() / 1e9, e))
            assert e < K.out_bound("split70k", dtype)
            assert out.outside_unchanged() and torch.equal(W.bits(xv), W.bits(xd))
            if route == contig:
                assert torch.equal(W.bits(out.view.contiguous()), W.bits(y0))
            yp = W.Buf(inp["yp"].to(dev), gr.n, C, *K.layout("mixed", "bnred", C, dtype)[0][2], dtype, dev, "in")
            bn4 = inp["bn4"].to(dev)
            out = W.Buf(None, gr.n, C, lay[1][0], lay[1][1], dtype, dev, "out")
            sums, sums0 = (torch.zeros(2 * C, dtype=torch.float64, device=dev) for _ in range(2))
            ops.spmm_bnred(gr.g, xv, out.view, yp.view, bn4, sums)
            ops.spmm_bnred(gr.g, xd, torch.empty_like(y0), inp["yp"].to(dev), bn4, sums0)
            es = W.relerr(sums.cpu(), K.bnred_sums(out.view, inp))
            print("gather layout bnred         split70k C=32 %s sums rel-L2 %.2e" % (dtype, es))
            assert torch.equal(W.bits(out.view.contiguous()), W.bits(y0)) or route != contig
            assert W.relerr(out.view, ref) < K.out_bound("split70k", dtype) and es < K.SUMS_BOUND["bnred"]
            assert route != contig or torch.equal(sums, sums0)
            assert out.outside_unchanged() and yp.unchanged() and torch.equal(W.bits(xv), W.bits(xd))
        finally:
            del big, xv
            torch.cuda.empty_cache()


def test_lean_gather_offset_limit_as_a_query(dev, graphs):
    """The lean gather's offsets are 32-bit counts of 16-byte units: n_cols * (ldx / 4) and n_rows * (ldy / 4) must stay below 2^32.
    Asked of ddmp_spmm_lean_selected only, no buffer is allocated: a RUN at that size needs about 68 GB for one operand
    (70,400 rows x 244,036 floats) and is left out on purpose -- the products beyond 2^32 BYTES are run above."""
    from dual_dmp_amd import _lib
    L, gr = _lib.lib(), graphs("split70k")
    supported(L.ddmp_spmm_lean_selected(gr.g.handle, 32, 32, 32), "the lean gather")
    for C in (32, 128):
        q = -(-(1 << 32) // gr.n_cols)
        assert L.ddmp_spmm_lean_selected(gr.g.handle, 4 * (q - 1), C, C) == 1
        assert L.ddmp_spmm_lean_selected(gr.g.handle, 4 * q, C, C) == 0
        q = -(-(1 << 32) // gr.n)
        assert L.ddmp_spmm_lean_selected(gr.g.handle, C, 4 * (q - 1), C) == 1
        assert L.ddmp_spmm_lean_selected(gr.g.handle, C, 4 * q, C) == 0


SWITCHES = [{"DDMP_SPMM_LEAN": "0"}, {"DDMP_SPMM_PATCH": "1"}]
_DEFAULT_OUTPUTS = {}


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_layouts_under_switched_routes(dev, tmp_path, env):
    """The table on "ico", "hub", "rcbhub" at widths 32, 96, 128 in a process of its own per setting (one at a time): under
    DDMP_SPMM_LEAN=0 every C % 32 == 0 case names the slab kernel and its outputs are bitwise the default route's (the slab kernel
    sums in the lean gather's order); under DDMP_SPMM_PATCH=1 "rcbhub" at C = 128 names patch+lean-list."""
    if any(k.startswith("DDMP_SPMM") for k in os.environ):
        pytest.skip("already inside a switched run")
    path = str(tmp_path / "out.npz")
    full = dict(os.environ)
    full.update(env)
    proc = subprocess.run([sys.executable, os.path.join(HERE, "gather_layout_worker.py"), path], env=full, capture_output=True,
                          text=True, timeout=600, cwd=os.path.dirname(HERE))
    print(proc.stdout[-4000:])
    assert proc.returncode == 0, (env, proc.stdout[-3000:], proc.stderr[-3000:])
    if env == {"DDMP_SPMM_LEAN": "0"}:
        if not _DEFAULT_OUTPUTS:
            W.run_restricted(dev, _DEFAULT_OUTPUTS, say=lambda *a, **k: None)
        got = np.load(path)
        assert set(got.files) == set(_DEFAULT_OUTPUTS) and len(got.files) >= 100
        for k in got.files:
            assert np.array_equal(got[k], _DEFAULT_OUTPUTS[k]), "slab route differs from the default route: %s" % k

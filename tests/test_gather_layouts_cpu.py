"""The cases of tests/test_gpu_gather_layouts.py, checked without a GPU and without the library (tests/gather_layout_cases.py): the
layouts are what they are named for, the float64 references agree with a dense evaluation, the graphs have the properties their
routes need, and the route function names the listed outcome of every listed case."""
import numpy as np
import pytest
import torch

import gather_layout_cases as K

F32, BF16 = torch.float32, torch.bfloat16
ALL_ENTRIES = tuple(K.OPERANDS)


def _layouts(dtype):
    return ("contig",) + (K.BF16_LAYOUTS if dtype == BF16 else K.F32_LAYOUTS)


def _cases():
    for dtype, widths in ((F32, K.F32_WIDTHS), (BF16, K.BF16_WIDTHS)):
        for entry in ALL_ENTRIES:
            for C in widths:
                for lname in _layouts(dtype):
                    got = K.layout(lname, entry, C, dtype)
                    if got is not None:
                        yield dtype, entry, C, lname, got[0], got[1]


def test_every_block_fits_its_buffer():
    n = 0
    for dtype, entry, C, lname, lay, coef_off in _cases():
        assert len(lay) == len(K.OPERANDS[entry])
        for ld, off in lay:
            assert off >= 0 and off + C <= ld, (entry, C, lname, ld, off)
        assert coef_off in (0, 1)
        n += 1
    assert n > 500


def test_layouts_have_the_alignment_they_are_named_for():
    for dtype, entry, C, lname, lay, coef_off in _cases():
        es = 2 if dtype == BF16 else 4
        lds, offs = [l for l, _ in lay], [o for _, o in lay]
        al = [(o * es) % 16 == 0 for o in offs]
        unit = 8 if dtype == BF16 else 4
        if lname in ("contig", "block", "mixed", "mixed-rot", "mixed-same-in", "odd-coef"):
            assert all(al) and (C % unit or all(l % unit == 0 for l in lds)), (entry, C, lname, lay)
        if lname == "block":
            assert all(o > 0 and l > C for l, o in lay)
        if lname == "mixed":
            assert len(set(lds)) == len(lds), (entry, C, lds)       # every leading dimension of the call differs
        if lname == "mixed-rot":
            assert entry == "bnred" and len(set(lds)) == 3 and lds[1] < lds[2]          # ldy < ldyp
        if lname == "mixed-same-in":
            assert entry == "bnbwd" and lds[0] == lds[1] != lds[2]
        if lname == "odd-ld":
            assert lds[0] == C + 5 and offs[0] == 0 and all(al)
            assert C % 4 or (lds[0] % 4 == 1 and all(l % 4 == 0 for l in lds[1:]))      # (widths that are multiples of 4)
        if lname == "odd-off":
            assert (C % 4 or lds[0] % 4 == 0) and (offs[0] * 4) % 16 == 4 and all(al[1:])
        if lname == "odd-out":
            i = [k for k, o in enumerate(K.OPERANDS[entry]) if o[2] != "in"][0]
            assert (C % 4 or lds[i] % 4 == 1) and not al[i] and all(a for k, a in enumerate(al) if k != i)
        assert (coef_off == 1) == (lname == "odd-coef")
        if lname == "bf16-ld":
            assert lds[0] % 8 == 4 and all(al)
        if lname == "bf16-off":
            assert lds[0] % 8 == 0 and (offs[0] * 2) % 16 == 8
    # every entry point has a layout in which all of its leading dimensions differ
    for entry in ALL_ENTRIES:
        lds = [l for l, _ in K.layout("mixed", entry, 32, F32)[0]]
        assert len(set(lds)) == len(K.OPERANDS[entry]) >= 2


def _small(name):
    if name == "star":
        return K.star_csr()
    ei, n = K.mesh_edges()[name]
    return K.gcn_csr(ei, n) + (n,)


@pytest.mark.parametrize("C", [3, 32])
@pytest.mark.parametrize("name", ["ico", "star"])
def test_float64_references_agree_with_a_dense_evaluation(name, C):
    rowptr, col, dinv, nc = _small(name)
    n = len(rowptr) - 1
    A, D = K.sparse_operator(rowptr, col, dinv, nc), K.dense_operator(rowptr, col, dinv, nc)
    inp = K.inputs(n, nc, C, F32)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    for entry in K.F32_ENTRIES:
        if entry == "bnbwd" and n != nc:
            continue
        got = K.reference(entry, lambda x: torch.sparse.mm(A, x), inp)
        want = K.reference(entry, lambda x: D @ x, inp)
        assert got.shape == (n, C) and rel(got, want) < 1e-12, (entry, rel(got, want))
    # the per-entry dot product against the dense dY H^T read at the entries
    G = K.sddmm_reference(rowptr, col, inp)
    full = inp["dy"].double() @ inp["h"].double().t()
    want = full[torch.from_numpy(K.entry_rows(rowptr)), torch.from_numpy(col.astype(np.int64))]
    assert rel(G, want) < 1e-12
    # the sums of the fused forms are the column sums of what they are documented to be
    out = K.reference("stats", lambda x: D @ x, inp).float()
    s = K.stats_sums(out)
    assert rel(s[:C], out.double().sum(0)) < 1e-12 and rel(s[C:], (out.double() ** 2).sum(0)) < 1e-12


def test_graphs_have_the_properties_their_routes_need():
    ico = _small("ico")
    assert len(ico[0]) - 1 == 642 and 642 % 64 != 0                  # a ragged last chunk
    hub = _small("hub")
    assert int(np.diff(hub[0]).max()) >= 1200
    assert K.largest_chunk_slots(hub[0]) > K.LEAN_SLOTS               # a chunk the lean gather cannot stage
    assert K.largest_chunk_slots(ico[0]) <= K.LEAN_SLOTS
    assert len(_small("rcbhub")[0]) - 1 == 4000
    rowptr, col, dinv, nc = K.star_csr()
    assert (len(rowptr) - 1, nc) == (200, 260) and rowptr[64] == 0     # an empty first chunk
    assert int(np.diff(rowptr).max()) == 1500 and K.largest_chunk_slots(rowptr) > K.LEAN_SLOTS
    assert col.min() >= 0 and col.max() < nc
    rowptr, col, dinv, nc = K.split70k_csr()
    assert len(rowptr) - 1 == nc == 70400 and col.min() >= 0 and col.max() < nc
    rowptr, col, dinv, nc = K.ring70k_csr()
    assert len(rowptr) - 1 == nc == 70000 and int(np.diff(rowptr).max()) == 5 and rowptr[64] == 0
    assert 70000 * 20 > K.SCALAR_GRID_ELEMS                            # the scalar kernel needs a second grid pass
    rowptr, col, dinv, nc = K.band70k_csr()
    assert len(rowptr) - 1 == nc == 70400 and int(np.diff(rowptr).max()) == 4 and int(np.abs(col - K.entry_rows(rowptr)).max()) <= 3
    for g in K.GRAPHS + ("ring70k", "band70k"):
        assert K.graph_cols(g) == (_small(g)[3] if g in K.MESH_GRAPHS + ("star",) else {"split70k": 70400, "band70k": 70400, "ring70k": 70000}[g])


@pytest.mark.parametrize("key", sorted(K.LISTED), ids=lambda k: "-".join(str(x) for x in k))
def test_route_function_names_the_listed_outcome(key):
    assert K.listed_route(key) == K.LISTED[key][1]


def test_every_route_is_listed():
    assert {v[1] for v in K.LISTED.values()} == {"scalar", "row", "lean", "slab", "patch", "patch+lean-list", "composition", "refused"}
    assert any(k[1] == "hub" and v[1] == "lean" for k, v in K.LISTED.items())          # lean with an unstaged chunk
    assert any(k[1] == "split70k" and v[1] == "patch+lean-list" for k, v in K.LISTED.items())   # with split chunks
    for entry in ("stats", "bnred"):
        assert any(k[0] == entry and v[1] == "composition" for k, v in K.LISTED.items())


def test_route_function_follows_the_query_answers():
    """The same call under other answers: what DDMP_SPMM_LEAN=0 / DDMP_SPMM_PATCH=1 change."""
    r = lambda entry, C, lname, dtype=F32, n_cols=4000, **ans: K.expected_route(entry, C, dtype, *K.layout(lname, entry, C, dtype), n_cols, **ans)
    assert r("spmm", 32, "block", lean=0, patch=0, n_heavy=0) == ("slab", None)
    assert r("spmm", 128, "block", lean=1, patch=1, n_heavy=1) == ("patch+lean-list", None)
    assert r("spmm", 128, "block", lean=0, patch=1, n_heavy=1) == ("slab", None)         # heavy chunks need the lean gather
    assert r("spmm", 128, "block", lean=0, patch=1, n_heavy=0) == ("patch", None)
    assert r("stats", 96, "mixed", lean=0, patch=0, n_heavy=0) == ("composition", "slab+scalar-sums")   # 96: no power of two
    assert r("stats", 16, "block", lean=0, patch=0, n_heavy=0) == ("composition", "row")
    assert r("bnred", 96, "odd-off", lean=1, patch=0, n_heavy=0) == ("composition", "scalar+scalar-sums")
    assert r("bnred", 16, "odd-coef", lean=0, patch=0, n_heavy=0) == ("composition", "row+scalar-sums")
    assert r("bnred", 16, "odd-off", lean=0, patch=0, n_heavy=0) == ("composition", "scalar")
    assert r("bnred", 96, "mixed", lean=0, patch=0, n_heavy=0) == ("slab", None)
    assert r("bnbwd", 128, "mixed", lean=1, patch=1, n_heavy=0) == ("patch", None)      # the patch kernel carries ldyb of its own
    assert r("axpby_z", 128, "block", lean=1, patch=0, n_heavy=1) == ("lean", None)
    assert r("spmm", 32, "block", BF16, lean=0, patch=0, n_heavy=0) == ("slab", None)
    # bfloat16: offsets in 16-byte units beyond 32 bits leave the lean staging
    big = [(1 << 20, 0), (32, 0)]
    assert K.expected_route("spmm", 32, BF16, big, 0, 70400, lean=1, patch=0, n_heavy=0) == ("slab", None)
    assert K.expected_route("spmm", 32, BF16, [(32768, 0), (40, 8)], 0, 70400, lean=1, patch=0, n_heavy=0) == ("lean", None)

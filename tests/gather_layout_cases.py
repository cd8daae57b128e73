"""Cases of tests/test_gpu_gather_layouts.py and tests/test_gather_layouts_cpu.py: the gather (ddmp_spmm*, ddmp_sddmm_f32) on operands
that are column blocks of wider buffers.  torch / numpy only: importable without a GPU and without the library.

Graphs: the smallest on which each route of the gather exists (``GRAPHS``; "ico", "hub", "rcbhub" are
edge_weight_route_worker.graphs(), the CSR builders of "star", "split70k" and "ring70k" live here and test_gpu_irregular.py
imports them; "band70k" is split70k without its designed chunks).  Widths: ``F32_WIDTHS`` / ``BF16_WIDTHS``.  Layouts: ``layout()``.  References: float64, ``reference()``.  The route a
call takes: ``expected_route()``, written from the dispatch rules of csrc/spmm.hip, spmm_lean.inc, spmm_patch.hip, spmm_b16.hip and
sddmm.hip, with the answers of the library's selection queries passed in as plain values.

Beyond the plain table: a call with four operands (spmm_axpby with z and z2) gets a fourth `mixed` pair so that all four leading
dimensions differ; `mixed-rot` gives spmm_bnred the one order of the pairs with ldy < ldyp; "band70k" exists for the LDS-patch
kernel WITHOUT a heavy list (every 70k graph with a designed chunk has one); bfloat16 has one kernel for every width, so its
routes are lean / slab / patch, never row or scalar.
"""
import numpy as np
import torch

SENTINEL = -7.25             # what output buffers hold before a call (exact in bfloat16)
PAD_ROWS = 3                 # rows of every buffer behind the operand's
GRAPHS = ("ico", "hub", "rcbhub", "star", "split70k")
MESH_GRAPHS = ("ico", "hub", "rcbhub")
F32_WIDTHS = (3, 20, 8, 16, 32, 96, 128)
BF16_WIDTHS = (16, 32, 96, 128)
LEAN_SLOTS = 1024            # entries (whole quads per row) of a 64-row chunk that the lean gather stages in LDS
SCALAR_GRID_ELEMS = 4096 * 256   # elements of one grid pass of the scalar kernel (4096 workgroups of 256 threads)


# ------------------------------------------------------------------------------------------------ graphs
def star_csr():
    """Hand-made rectangular CSR: 200 rows over 260 columns; rows 0..69 empty (an empty first chunk), row 100 has 1500 entries
    (repeats allowed: multi-edges), rows 150..155 empty, the rest 1..9 entries; arbitrary positive "dinv".
    -> (rowptr, col, dinv, n_cols)"""
    rng = np.random.default_rng(7)
    n, nc = 200, 260
    lens = rng.integers(1, 10, size=n)
    lens[:70] = 0
    lens[150:156] = 0
    lens[100] = 1500
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = rng.integers(0, nc, size=int(rowptr[-1])).astype(np.int32)
    dinv = (rng.random(nc) * 0.9 + 0.1).astype(np.float32)
    return rowptr, col, dinv, nc


def split70k_csr(special=None):
    """A designed graph: 70,400 rows with 4 local entries each (patches of ~70 rows: patch_kd = 3, 96-row buffers), and three chunks
    whose rows reference far-apart columns -- 2 distinct per row (whole patch 128: halves of 64 fit), 5 per row (halves 160,
    quarters 80 fit), 8 per row (quarters 128: stays heavy).  -> (rowptr, col, dinv, n_cols)"""
    n = 70400
    rng = np.random.default_rng(5)
    rows_cols = []
    if special is None:
        special = {100: 2, 500: 5, 900: 8}                        # chunk -> distinct far columns per row
    for c in range(n // 64):
        r = np.arange(64 * c, 64 * c + 64)
        k = special.get(c)
        if k is None:
            cols = np.stack([r, np.clip(r + 1, 0, n - 1), np.clip(r - 1, 0, n - 1), np.clip(r + 3, 0, n - 1)], 1)
        else:                                                     # row i of the chunk: k columns nobody else in the chunk references
            cols = (np.arange(64 * k).reshape(64, k) * 97 + 1000 * c) % n
        rows_cols.append(cols)
    lens = np.array([len(x) for cc in rows_cols for x in cc])
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.asarray(x) for cc in rows_cols for x in cc]).astype(np.int32)
    dinv = (rng.random(n) * 0.9 + 0.1).astype(np.float32)
    return rowptr, col, dinv, n


def band70k_csr():
    """split70k without its three designed chunks: every chunk's patch fits, so the graph gets patch tables and NO heavy chunk --
    the LDS-patch kernel alone."""
    return split70k_csr(special={})


def ring70k_csr():
    """A ring graph over 70,000 rows, 5 entries per row, with rows 0..63, every 97th row and the last row empty.
    -> (rowptr, col, dinv, n_cols)"""
    n = 70000
    lens = np.full(n, 5, dtype=np.int64)
    lens[:64] = 0
    lens[::97] = 0
    lens[-1] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = np.repeat(np.arange(n), lens)
    k = np.arange(int(rowptr[-1])) - rowptr[rows]
    col = ((rows + k - 2) % n).astype(np.int32)
    dinv = (np.random.default_rng(3).random(n) * 0.5 + 0.5).astype(np.float32)
    return rowptr, col, dinv, n


_MESH = {}


def mesh_edges():
    """name -> (edge_index, n) of edge_weight_route_worker.graphs(), built once per process."""
    if not _MESH:
        import edge_weight_route_worker
        _MESH.update(edge_weight_route_worker.graphs())
    return _MESH


def gcn_csr(ei, n):
    """(rowptr, col, dinv) of A + I with D^-1/2 from a symmetric edge_index without self loops and duplicates, in numpy: rows =
    targets, columns ascending (what ops.csr_build_host gives for such an input)."""
    src, dst = ei[0].numpy().astype(np.int64), ei[1].numpy().astype(np.int64)
    rows = np.concatenate([dst, np.arange(n)])
    cols = np.concatenate([src, np.arange(n)])
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    cnt = np.bincount(rows, minlength=n)
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    dinv = (1.0 / np.sqrt(cnt.astype(np.float64))).astype(np.float32)
    return rowptr, cols.astype(np.int32), dinv


def entry_rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def sparse_operator(rowptr, col, dinv, n_cols):
    """The float64 operator of an unvalued graph: entry (i, j) = dinv[i] * dinv[j], repeated entries add up."""
    rows = entry_rows(rowptr)
    w = dinv.astype(np.float64)[rows] * dinv.astype(np.float64)[col]
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, col.astype(np.int64)])), torch.from_numpy(w),
                                   (len(rowptr) - 1, n_cols)).coalesce()


def dense_operator(rowptr, col, dinv, n_cols):
    """The same operator as a dense float64 matrix, entry by entry (small graphs)."""
    A = torch.zeros(len(rowptr) - 1, n_cols, dtype=torch.float64)
    rows = torch.from_numpy(entry_rows(rowptr))
    w = torch.from_numpy(dinv.astype(np.float64))
    return A.index_put((rows, torch.from_numpy(col.astype(np.int64))), w[rows] * w[torch.from_numpy(col.astype(np.int64))], accumulate=True)


def largest_chunk_slots(rowptr):
    """The most LDS slots (whole quads per row) a 64-row chunk of this graph asks of the lean gather."""
    q = (np.diff(rowptr) + 3) // 4 * 4
    return max(int(q[i:i + 64].sum()) for i in range(0, len(q), 64))


# ------------------------------------------------------------------------------------------------ entry points
# operands in call order: (name, rows it has: "cols" = gathered (n_cols rows) | "rows" = row-wise (n_rows rows), role)
_XO = (("x", "cols", "in"), ("out", "rows", "out"))
OPERANDS = {
    "spmm": _XO, "spmm+bias": _XO, "spmm+pro+bias": _XO, "stats": _XO,
    "bnred": _XO + (("yp", "rows", "in"),),
    "bnbwd": (("dz", "cols", "in"), ("yb", "cols", "in"), ("out", "rows", "out")),
    "axpby_z": _XO + (("z", "rows", "in"),),
    "axpby_z_z2": _XO + (("z", "rows", "in"), ("z2", "rows", "in")),
    "axpby_alias": (("x", "cols", "in"), ("z", "rows", "inout")),
    "v_spmm": _XO, "v_spmm_t": _XO,
    "sddmm": (("dy", "rows", "in"), ("h", "cols", "in")),
}
HAS_COEF = ("spmm+bias", "spmm+pro+bias", "stats", "bnred", "bnbwd")
F32_ENTRIES = ("spmm", "spmm+bias", "spmm+pro+bias", "stats", "bnred", "bnbwd", "axpby_z", "axpby_z_z2", "axpby_alias")
VALUED_ENTRIES = ("v_spmm", "v_spmm_t", "sddmm")
BF16_ENTRIES = ("spmm", "stats", "bnred", "bnbwd")
# (has_pro, has_red) of ddmp_spmm_patch_selected for the entry's form; None: the entry never takes the LDS-patch kernel
PATCH_FORM = {"spmm": (0, 0), "spmm+bias": (0, 0), "spmm+pro+bias": (1, 0), "stats": (1, 2), "bnred": (0, 1), "bnbwd": (1, 3),
              "v_spmm": (0, 0), "v_spmm_t": (0, 0), "axpby_z": None, "axpby_z_z2": None, "axpby_alias": None, "sddmm": None}


def entry_applies(entry, C, dtype, square):
    """Is the entry point run at this width at all?  Every one at every width, but for the BatchNorm backward on the gather, which
    needs a square graph (dz and yb have n_cols rows); below C = 32 that entry is a refusal."""
    return square if entry == "bnbwd" else True


# ------------------------------------------------------------------------------------------------ layouts
F32_LAYOUTS = ("block", "mixed", "mixed-rot", "mixed-same-in", "odd-ld", "odd-off", "odd-out", "odd-coef")
BF16_LAYOUTS = ("block", "mixed", "mixed-same-in", "bf16-ld", "bf16-off")


def layout(name, entry, C, dtype):
    """-> ([(ld, off) per operand of the entry, in call order], coef_off) in elements, or None where the layout does not apply to
    the entry.  Every operand is the column block [off, off + C) of a [rows + PAD_ROWS, ld] buffer; coef_off: the per-column vectors
    (bias, pro, bn4 / c10 rows, ref) start that many elements into a [C + coef_off] buffer.

    contig         (C, 0)
    block          (C + 4, 4); bfloat16 (C + 8, 8)
    mixed          (C + 4, 4), (max(2C, C + 12), 12), (C + 8, 8) in turn over the operands, a fourth operand (max(2C, C + 12) + 8, 16): every
                   leading dimension of the call differs; bfloat16: offsets and paddings doubled
    mixed-rot      spmm_bnred only: the same pairs taken from the third on ((C + 8, 8), (C + 4, 4), (max(2C, C + 12), 12)), so that
                   ldy < ldyp where `mixed` has ldy > ldyp
    mixed-same-in  spmm_bnbwd only: as mixed, dz and yb on one leading dimension (the lean / patch route of that entry)
    odd-ld         float32: the first input (C + 5, 0), the rest `block`
    odd-off        float32: the first input (C + 4, 1)
    odd-out        float32: the output (C + 5, 1)
    odd-coef       float32: operands `block`, the per-column vectors one element into their buffers
    bf16-ld        bfloat16: the first input (C + 4, 0): a leading dimension that is no multiple of 8
    bf16-off       bfloat16: the first input (C + 8, 4): 8 bytes off
    """
    ops = OPERANDS[entry]
    bf = dtype == torch.bfloat16
    m = 2 if bf else 1
    if name == "contig":
        return [(C, 0)] * len(ops), 0
    blk = (C + 4 * m, 4 * m)
    if name == "block":
        return [blk] * len(ops), 0
    pairs = [(C + 4 * m, 4 * m), (max(2 * C, C + 12 * m), 12 * m), (C + 8 * m, 8 * m), (max(2 * C, C + 12 * m) + 8 * m, 16 * m)]
    if name == "mixed":
        return [pairs[i] for i in range(len(ops))], 0
    if name == "mixed-rot":
        return ([pairs[(i + 2) % 3] for i in range(len(ops))], 0) if entry == "bnred" and not bf else None
    if name == "mixed-same-in":
        return ([pairs[0], (pairs[0][0], pairs[0][1]), pairs[2]], 0) if entry == "bnbwd" else None
    if name in ("odd-ld", "odd-off", "odd-out", "odd-coef"):
        if bf:
            return None
        lay = [blk] * len(ops)
        if name == "odd-coef":
            return (lay, 1) if entry in HAS_COEF else None
        if name == "odd-out":
            outs = [i for i, o in enumerate(ops) if o[2] != "in"]
            if not outs:
                return None
            lay[outs[0]] = (C + 5, 1)
        else:
            lay[0] = (C + 5, 0) if name == "odd-ld" else (C + 4, 1)
        return lay, 0
    if name in ("bf16-ld", "bf16-off"):
        if not bf:
            return None
        lay = [blk] * len(ops)
        lay[0] = (C + 4, 0) if name == "bf16-ld" else (C + 8, 4)
        return lay, 0
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ the expected route
def _reduce_stage(C, lay, coef_off):
    """The second stage of a composed float32 route (bn_stats / bn_bwd_reduce of the stored output): the vector column reduction
    where it applies (C a power of two in [8, 1024], ld % 4 == 0, 16-byte aligned blocks and vectors), else the scalar one --
    another partition of the rows, so the float64 sums agree to rounding, not bit for bit."""
    vec = 8 <= C <= 1024 and C & (C - 1) == 0 and all(l % 4 == 0 and (o * 4) % 16 == 0 for l, o in lay) and coef_off == 0
    return "" if vec else "+scalar-sums"


def expected_route(entry, C, dtype, lay, coef_off, n_cols, *, lean, patch, n_heavy):
    """-> (outcome, inner): the kernel(s) the call runs, from the dispatch rules of the library.  outcome: "scalar" | "row" | "lean"
    | "slab" | "patch" | "patch+lean-list" | "composition" | "refused"; inner: the route of the plain gather inside a composition
    (+ "+scalar-sums" where its reduction stage is the scalar one, see _reduce_stage).

    lay: [(ld, off)] of layout(); the query answers as plain values --
    lean     float32: ddmp_spmm_lean_selected(g, ldx, ldy, C) with the call's OWN leading dimensions (spmm_bnbwd: lddz and ld_out);
             bfloat16: ddmp_spmm_lean_selected(g, 32, 32, 32), i.e. whether the lean staging is switched on at all -- the bfloat16
             kernel decides from n_cols * (ldx / 8) < 2^32 itself, which this function restates
    patch    ddmp_spmm_patch_selected(g, C, dtype, *PATCH_FORM[entry]) (False where PATCH_FORM has None)
    n_heavy  of ddmp_graph_patch_info
    """
    es = 2 if dtype == torch.bfloat16 else 4
    lds = [l for l, _ in lay]
    al = all((o * es) % 16 == 0 for _, o in lay) and (coef_off * 4) % 16 == 0
    patched = "patch+lean-list" if n_heavy > 0 else "patch"
    if dtype == torch.bfloat16:
        if C % 8 or any(l % 8 for l in lds) or not al:
            return "refused", None
        lean_b = bool(lean) and n_cols * (lds[0] >> 3) < (1 << 32) and (entry != "bnbwd" or lds[1] == lds[0])
        if entry == "stats" and (C % 16 or C > 1024):
            return "composition", expected_route("spmm", C, dtype, lay, coef_off, n_cols, lean=lean, patch=False, n_heavy=n_heavy)[0]
        if patch:
            return patched, None
        return ("lean" if lean_b else "slab"), None
    vec = C % 4 == 0 and all(l % 4 == 0 for l in lds) and al
    if entry == "sddmm":
        return ("row" if vec else "scalar"), None
    if entry.startswith("axpby"):
        if vec and C % 32 == 0:
            return ("lean" if lean else "slab"), None
        return ("row" if vec and C in (8, 16) else "scalar"), None
    if entry in ("spmm", "spmm+bias", "spmm+pro+bias", "v_spmm", "v_spmm_t"):
        if vec and C % 32 == 0:
            if patch and (lean or n_heavy == 0):
                return patched, None
            return ("lean" if lean else "slab"), None
        return ("row" if vec and C in (8, 16) else "scalar"), None
    if entry == "bnbwd":
        if C % 32 or C < 32 or not vec:
            return "refused", None
        lean_e = bool(lean) and lds[0] == lds[1]              # one staged offset serves dz and yb
        if patch and (lean_e or n_heavy == 0):
            return patched, None
        return ("lean" if lean_e else "slab"), None
    if entry == "stats":
        if C % 32 == 0 and 32 <= C <= 1024 and lean and vec:
            return (patched if patch else "lean"), None
        inner = expected_route("spmm+pro+bias", C, dtype, lay, coef_off, n_cols, lean=lean, patch=False, n_heavy=n_heavy)[0]
        return "composition", inner + _reduce_stage(C, lay[1:2], 0)
    if entry == "bnred":
        if C % 32 == 0 and vec:
            if patch and (lean or n_heavy == 0):
                return patched, None
            return ("lean" if lean else "slab"), None
        inner = expected_route("spmm", C, dtype, lay[:2], 0, n_cols, lean=lean, patch=False, n_heavy=n_heavy)[0]
        return "composition", inner + _reduce_stage(C, lay[1:3], coef_off)
    raise KeyError(entry)


# Cases whose route in the DEFAULT configuration is listed: (entry, graph, C, "f32" | "bf16", layout) -> (query answers, outcome).
# Between them every route of the gather is named: scalar, row, lean (on "hub" with a chunk it cannot stage), slab, patch,
# patch+lean-list (on "split70k": with split chunks), composition for spmm_stats and spmm_bnred, refused.
_L = dict(lean=1, patch=0, n_heavy=0)
_N = dict(lean=0, patch=0, n_heavy=0)
_P = dict(lean=1, patch=1, n_heavy=1)
_PN = dict(lean=0, patch=1, n_heavy=1)
_R = dict(lean=1, patch=1, n_heavy=0)
LISTED = {
    ("spmm", "ico", 3, "f32", "contig"): (_N, "scalar"),
    ("spmm", "ico", 20, "f32", "block"): (_N, "scalar"),
    ("spmm+bias", "hub", 8, "f32", "block"): (_N, "row"),
    ("spmm+pro+bias", "star", 16, "f32", "mixed"): (_N, "row"),
    ("spmm", "ico", 32, "f32", "block"): (_L, "lean"),
    ("spmm", "hub", 32, "f32", "mixed"): (_L, "lean"),
    ("spmm+pro+bias", "hub", 96, "f32", "block"): (_L, "lean"),
    ("spmm", "star", 96, "f32", "mixed"): (_L, "lean"),
    ("spmm", "rcbhub", 128, "f32", "block"): (_L, "lean"),
    ("spmm", "ico", 32, "f32", "odd-ld"): (_N, "scalar"),
    ("spmm", "ico", 32, "f32", "odd-off"): (_L, "scalar"),
    ("spmm", "ico", 32, "f32", "odd-out"): (_N, "scalar"),
    ("spmm+bias", "ico", 32, "f32", "odd-coef"): (_L, "scalar"),
    ("spmm", "split70k", 128, "f32", "block"): (_P, "patch+lean-list"),
    ("spmm+pro+bias", "split70k", 128, "f32", "mixed"): (_P, "patch+lean-list"),
    ("spmm", "split70k", 96, "f32", "mixed"): (_L | dict(n_heavy=1), "lean"),
    ("spmm", "band70k", 128, "f32", "block"): (_R, "patch"),
    ("bnred", "band70k", 128, "f32", "mixed"): (_R, "patch"),
    ("bnbwd", "band70k", 128, "f32", "mixed"): (_R, "patch"),
    ("spmm", "ring70k", 20, "f32", "block"): (_N, "scalar"),
    ("stats", "ico", 32, "f32", "mixed"): (_L, "lean"),
    ("stats", "split70k", 128, "f32", "block"): (_P, "patch+lean-list"),
    ("stats", "ico", 16, "f32", "block"): (_N, "composition"),
    ("stats", "ico", 3, "f32", "block"): (_N, "composition"),
    ("bnred", "hub", 20, "f32", "mixed"): (_N, "composition"),
    ("stats", "hub", 96, "f32", "odd-coef"): (_L, "composition"),
    ("stats", "hub", 96, "f32", "odd-out"): (_N, "composition"),
    ("bnred", "hub", 32, "f32", "mixed"): (_L, "lean"),
    ("bnred", "hub", 32, "f32", "mixed-rot"): (_L, "lean"),
    ("bnred", "split70k", 128, "f32", "mixed"): (_P, "patch+lean-list"),
    ("bnred", "star", 8, "f32", "block"): (_N, "composition"),
    ("bnred", "ico", 96, "f32", "odd-ld"): (_N, "composition"),
    ("bnbwd", "ico", 32, "f32", "mixed-same-in"): (_L, "lean"),
    ("bnbwd", "ico", 32, "f32", "mixed"): (_L, "slab"),
    ("bnbwd", "rcbhub", 96, "f32", "mixed"): (_L, "slab"),
    ("bnbwd", "split70k", 128, "f32", "mixed-same-in"): (_P, "patch+lean-list"),
    ("bnbwd", "split70k", 128, "f32", "mixed"): (_P, "slab"),
    ("bnbwd", "ico", 32, "f32", "odd-off"): (_L, "refused"),
    ("bnbwd", "ico", 32, "f32", "odd-coef"): (_L, "refused"),
    ("bnbwd", "ico", 16, "f32", "block"): (_N, "refused"),
    ("axpby_z", "ico", 3, "f32", "block"): (_N, "scalar"),
    ("axpby_z_z2", "hub", 16, "f32", "mixed"): (_N, "row"),
    ("axpby_z_z2", "hub", 96, "f32", "mixed"): (_L, "lean"),
    ("axpby_alias", "split70k", 128, "f32", "block"): (_L | dict(n_heavy=1), "lean"),
    ("axpby_z", "ico", 32, "f32", "odd-out"): (_N, "scalar"),
    ("v_spmm", "hub", 32, "f32", "mixed"): (_L, "lean"),
    ("v_spmm_t", "rcbhub", 128, "f32", "block"): (_L, "lean"),
    ("v_spmm", "ico", 20, "f32", "block"): (_N, "scalar"),
    ("sddmm", "ico", 20, "f32", "mixed"): (_N, "row"),
    ("sddmm", "hub", 3, "f32", "block"): (_N, "scalar"),
    ("sddmm", "hub", 32, "f32", "odd-off"): (_N, "scalar"),
    ("spmm", "ico", 16, "bf16", "block"): (_L, "lean"),
    ("stats", "hub", 96, "bf16", "mixed"): (_L, "lean"),
    ("bnred", "split70k", 128, "bf16", "mixed"): (_L | dict(n_heavy=1), "lean"),
    ("spmm", "split70k", 128, "bf16", "block"): (_P, "patch+lean-list"),
    ("bnbwd", "ico", 32, "bf16", "mixed"): (_L, "slab"),
    ("bnbwd", "ico", 32, "bf16", "mixed-same-in"): (_L, "lean"),
    ("spmm", "ico", 32, "bf16", "bf16-ld"): (_L, "refused"),
    ("bnred", "hub", 128, "bf16", "bf16-off"): (_L, "refused"),
}
del _L, _N, _P, _PN, _R


def graph_cols(graph):
    return {"ico": 642, "hub": 1800, "rcbhub": 4000, "star": 260, "split70k": 70400, "band70k": 70400, "ring70k": 70000}[graph]


def listed_route(key):
    entry, graph, C, dt, lname = key
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    lay, coef_off = layout(lname, entry, C, dtype)
    return expected_route(entry, C, dtype, lay, coef_off, graph_cols(graph), **LISTED[key][0])[0]


# ------------------------------------------------------------------------------------------------ inputs and float64 references
def f_ref(x, a, b, slope=0.01):
    z = x * a + b
    return torch.where(z > 0, z, slope * z)


def inputs(n, nc, C, dtype, seed=0):
    """CPU tensors of every operand of every entry point, in `dtype` (per-column vectors float32)."""
    gen = torch.Generator().manual_seed(1000 * C + n + seed)
    r = lambda *s: torch.randn(*s, generator=gen)
    u = lambda *s: torch.rand(*s, generator=gen)
    d = dict(x=r(nc, C).to(dtype), bias=r(C), a=u(C) + 0.5, b=r(C), yp=(r(n, C) * 2 + 0.3).to(dtype),
             bn4=torch.stack([u(C) + 0.5, r(C), r(C), u(C) + 0.5]), dz=r(nc, C).to(dtype), yb=(r(nc, C) * 2 + 0.5).to(dtype),
             c10=torch.stack([r(C) * 0.1, r(C) * 0.1]), z=r(n, C).to(dtype), z2=r(n, C).to(dtype), dy=r(n, C).to(dtype))
    d["h"] = d["x"]
    return d


AXPBY = dict(a=-1.2, b=0.4, c=-1.0, d=0.7)


def reference(entry, mm, inp, mm_t=None):
    """float64 reference of the entry's OUTPUT from the inputs of ``inputs()``; ``mm(X)`` applies the graph's float64 operator (the
    expressions of test_gpu_irregular._forms and edge_weight_route_worker.run)."""
    D = lambda k: inp[k].double()
    n = inp["z"].shape[0]
    if entry in ("spmm", "v_spmm"):
        return mm(D("x"))
    if entry == "v_spmm_t":
        return mm_t(D("x"))
    if entry == "spmm+bias":
        return mm(D("x")) + D("bias")
    if entry in ("spmm+pro+bias", "stats"):
        return mm(f_ref(D("x"), D("a"), D("b"))) + D("bias")
    if entry == "bnred":
        return mm(D("x"))
    if entry == "bnbwd":
        sc, sh = D("bn4")[0], D("bn4")[1]
        z = D("yb") * sc + sh
        return mm(sc * D("dz") * torch.where(z > 0, 1.0, 0.01) + D("c10")[0] * D("yb") + D("c10")[1])
    if entry.startswith("axpby"):
        y = AXPBY["a"] * mm(D("x")) + AXPBY["b"] * D("x")[:n] + AXPBY["c"] * D("z")
        return y + AXPBY["d"] * D("z2") if entry == "axpby_z_z2" else y
    raise KeyError(entry)


def stats_sums(out):
    """float64 [2C] of spmm_stats from the output as stored."""
    od = out.double().cpu()
    return torch.cat([od.sum(0), (od * od).sum(0)])


def bnred_sums(out, inp):
    """float64 [2C] of spmm_bnred from the output as stored (the knife edge a*y+b == 0 does not occur with random data)."""
    od, yd = out.double().cpu(), inp["yp"].double()
    sc, sh, mu, rs = (t.double() for t in inp["bn4"])
    gg = od * torch.where(yd * sc + sh > 0, 1.0, 0.01)
    return torch.cat([gg.sum(0), (gg * (yd - mu) * rs).sum(0)])


def sddmm_reference(rowptr, col, inp):
    """The per-entry float64 dot product G[e] = sum_c dy[row e, c] * h[col e, c]."""
    rows = torch.from_numpy(entry_rows(rowptr))
    return (inp["dy"][rows].double() * inp["h"][torch.from_numpy(np.asarray(col)).long()].double()).sum(1)


def out_bound(graph, dtype):
    """rel-L2 bound of a gather output against float64 (test_gpu_irregular.py / test_gpu_edge_weight.py)."""
    if dtype == torch.bfloat16:
        return 4e-3
    return {"star": 2e-6, "split70k": 3e-6, "band70k": 3e-6, "ring70k": 3e-6}.get(graph, 1e-6)


SUMS_BOUND = {"stats": 2e-6, "bnred": 2e-5}
SDDMM_BOUND = 1e-6

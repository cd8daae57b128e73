"""PPFConv on the GPU: the point-pair features of the entries (``ops.ppf_entries``), the arg-max gather of the edge-conditioned
message and its one-launch backward (``ops.gather_max_attr`` / ``ops.gather_max_attr_bwd``) and the drop-in against the float64
edge-list reference (tests/ppf_ref.py) on the icosphere (ragged last chunk, ragged last wave step), the open grid (boundary) and
the hub graph (one 1200-entry row), with duplicate edges and explicit loops on top, with one edgeless node, with and without
``add_self_loops``.  The geometry is random, not the mesh's (a regular mesh has exact ties by symmetry): pos ~ N(0, 1)^3, normals
uniform on the sphere.

Tolerance policy:
* features: every column against the float64 evaluation of the same float32 inputs, rel-L2 <= 1e-6 (the project's gather
  tolerance), also on a smooth input (pos = 100 + N(0, 1), all normals within 1e-3 rad), where a plain float32 cross product
  measures 4.7e-6 in the fourth column and the compensated one 5.7e-8; loop entries exactly 0;
* kernel level, on exact float32 B, F, E, dG: with E = 0 the gather is ``ops.gather_max`` bit for bit; otherwise y against float64
  rel-L2 <= 1e-6, the float64 message of arg[i, c] within 1e-6 rms of the float64 row maximum, arg equal to the float64 winner
  wherever the float64 top-two gap is >= 1e-3 rms; dB and dE against float64 sums over the kernel's OWN arg, rel-L2 <= 1e-6;
* operator level, against ``PPFConvRef`` in float64, EdgeConv's ambiguity rule stated for the full message: an output whose
  float64 top-two gap over the coalesced entries is below 1e-3 x rms (over all entries of the bias-free message) is ambiguous; dG
  is zeroed there on both sides, the ambiguous share must stay <= 1 % (printed), arg must equal the reference winner at every
  other output, and y, dx and every parameter gradient meet rel-L2 <= 1e-5."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import edge_weight_route_worker as W
import oracle_jobs as OJ
from ppf_ref import PPFConvRef, ppf_features, ppf_messages, ppf_winners_and_gaps

pytestmark = pytest.mark.gpu
relerr = W.relerr

OP_TOL = 1e-5
GATHER_TOL = 1e-6
AMB_GAP = 1e-3                  # x rms of the bias-free message
AMB_SHARE = 0.01

CASES = [(0, 3), (0, 8), (3, 3), (16, 4), (8, 32), (32, 40), (64, 64)]   # (in, out): scalar path, float4 path, a ragged packed
WIDTHS = sorted({c[1] for c in CASES})                                  # width, more than one column slab per lane


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graphs(dev):
    """name -> (edge_index, its device copy, n): the route worker's graphs + duplicates and explicit loops (two on node 5);
    "<name>-iso": one more node without any edge (an empty row where no loops are added)."""
    out = {}
    base = W.graphs()
    for name in ("ico", "grid", "hub"):
        ei, n = base[name]
        extra = torch.tensor([[3, 9, 5, 5, 40], [9, 3, 5, 5, 40]])
        dup = ei[:, :50]
        ei = torch.cat([ei, extra, dup, dup[[1, 0]]], 1).contiguous()
        out[name] = (ei, ei.to(dev), n)
        out[name + "-iso"] = (ei, ei.to(dev), n + 1)
    return out


def geometry(n, gen, smooth=False):
    pos = torch.randn(n, 3, generator=gen)
    nrm = torch.randn(n, 3, generator=gen)
    if smooth:
        pos = pos + 100.0
        nrm = torch.tensor([0.3, -0.5, 0.8]) + 5e-4 * nrm        # every pair within about 1e-3 rad
    return pos, nrm / nrm.norm(dim=1, keepdim=True)


def host_csr(ei, n, loops):
    """(rows, cols) int64 of the coalesced CSR entries in CSR order, empty [n] bool."""
    from dual_dmp_amd import ops
    t = ops.csr_build_valued_host(ei.numpy(), n, ops.GV_LOOPS if loops else 0)
    cnt = np.diff(t["rowptr"])
    return torch.from_numpy(np.repeat(np.arange(n), cnt)), torch.from_numpy(t["col"].astype(np.int64)), torch.from_numpy(cnt == 0)


def entry_of(rows, cols, n, arg):
    """The CSR entry (i, arg[i, c]) for every output [n, C]; -1 where the row has none (arg < 0)."""
    key = rows * n + cols                                        # ascending: CSR order
    want = torch.arange(n).view(-1, 1) * n + arg.long().clamp(min=0)
    e = torch.searchsorted(key, want.reshape(-1)).reshape(want.shape).clamp(max=len(key) - 1)
    assert bool((key[e] == want)[arg >= 0].all()), "arg names a node that is not a source of the row"
    return torch.where(arg >= 0, e, torch.full((), -1, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ 1. the features
@pytest.mark.parametrize("name", ["ico", "hub-iso"])
@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("smooth", [False, True])
def test_entries_match_float64(dev, graphs, name, loops, smooth):
    from dual_dmp_amd import ops
    ei, eid, n = graphs[name]
    rows, cols, _ = host_csr(ei, n, loops)
    pos, nrm = geometry(n, torch.Generator().manual_seed(n + 4), smooth)
    g = ops.graph_for(eid, n, norm="gat", add_self_loops=loops)
    pd, nd = pos.to(dev), nrm.to(dev)
    f = ops.ppf_entries(g, pd, nd)
    assert f.shape == (len(rows), 4) and f.dtype == torch.float32
    want = ppf_features(pos.double(), nrm.double(), torch.stack([cols, rows]))
    loop = rows == cols
    assert bool(loop.any()) and bool((f.cpu()[loop] == 0).all())            # exactly 0, not n x n under FMA contraction
    want[loop] = 0.0
    for d in range(4):
        e = relerr(f[:, d], want[:, d])
        print("%s loops=%s smooth=%s column %d: rel-L2 %.2e (tolerance %.0e)" % (name, loops, smooth, d, e, GATHER_TOL))
        assert e <= GATHER_TOL, (d, e)
    # the cache: same tensors -> the same result object; an in-place change of pos -> a new evaluation
    assert ops.ppf_entries(g, pd, nd) is f
    pd.mul_(2.0)
    f2 = ops.ppf_entries(g, pd, nd)
    assert f2 is not f and relerr(f2[:, 0], 2.0 * want[:, 0]) <= GATHER_TOL and relerr(f2[:, 3], want[:, 3]) <= GATHER_TOL
    assert ops.ppf_entries(g, pd, nd.clone()) is not f2                     # another tensor object: no hit
    # column blocks of a wider row buffer
    z = torch.cat([pos * 2.0, nrm, torch.zeros(n, 1)], 1).to(dev)
    assert torch.equal(ops.ppf_entries(g, z[:, :3], z[:, 3:6]), f2)


# ------------------------------------------------------------------------------------------------ 2. the kernels
def db_from_arg(dg, arg, rows, cols, n):
    """float64 dB from a given arg: dB[j, c] = sum over the entries (j, i) of row j of dG[i, c] where arg[i, c] == j."""
    hit = arg.long()[cols] == rows.view(-1, 1)
    return torch.zeros((n, dg.shape[1]), dtype=torch.float64).index_add_(0, rows, torch.where(hit, dg.double()[cols], torch.zeros((), dtype=torch.float64)))


def de_from_arg(dg, arg, f, rows, cols, n):
    """float64 dE [4, C] from a given arg and F: sum_i dG[i, c] F[entry(i, arg[i, c]), :]."""
    e = entry_of(rows, cols, n, arg)
    fsel = torch.where((e >= 0).unsqueeze(-1), f.double()[e.clamp(min=0)], torch.zeros((), dtype=torch.float64))   # [n, C, 4]
    return torch.einsum("nc,ncd->dc", dg.double(), fsel)


@pytest.mark.parametrize("name,loops", [("ico", True), ("ico", False), ("grid", True), ("hub", False), ("ico-iso", False),
                                        ("hub-iso", False), ("hub-iso", True)])
@pytest.mark.parametrize("C", WIDTHS)
def test_kernels_match_float64(dev, graphs, name, loops, C):
    from dual_dmp_amd import ops
    ei, eid, n = graphs[name]
    gen = torch.Generator().manual_seed(n + C)
    pos, nrm = geometry(n, gen)
    b, dg = torch.randn(n, C, generator=gen), torch.randn(n, C, generator=gen)
    e = torch.randn(4, C, generator=gen) * 0.5
    rows, cols, empty = host_csr(ei, n, loops)
    assert bool(empty.any()) == (name.endswith("-iso") and not loops)
    g = ops.graph_for(eid, n, norm="gat", add_self_loops=loops)
    assert g.nnz == len(rows)
    fd = ops.ppf_entries(g, pos.to(dev), nrm.to(dev))
    f = fd.cpu()
    cp = (C + 3) // 4 * 4                                        # the operator's layouts: B a column block of a row buffer
    buf = torch.zeros(n, 2 * cp, device=dev)
    buf[:, cp:cp + C] = b.to(dev)
    bd, dgd, ed = buf[:, cp:cp + C], dg.to(dev), e.to(dev)
    # E = 0: ops.gather_max, bit for bit
    y0, arg0 = ops.gather_max_attr(g, bd, fd, torch.zeros_like(ed))
    ym, argm = ops.gather_max(g, bd)
    assert torch.equal(y0, ym) and torch.equal(arg0, argm)
    ybuf = torch.full((n, cp + 4), float("nan"), device=dev)
    y, arg = ops.gather_max_attr(g, bd, fd, ed, out=ybuf[:, :C])
    y_noarg, none = ops.gather_max_attr(g, bd, fd, ed, want_arg=False)
    y_nob, arg_nob = ops.gather_max_attr(g, None, fd, ed)
    gbuf = torch.full((n, cp + 4), float("nan"), device=dev)
    db, parts = ops.gather_max_attr_bwd(g, dgd, arg, fd, out=gbuf[:, :C])
    db2, none2 = ops.gather_max_attr_bwd(g, dgd, arg, fd, want_parts=False)
    de = ops.gatv2_datt(parts, 4)
    torch.cuda.synchronize()
    assert y.shape == (n, C) and arg.shape == (n, C) and arg.dtype == torch.int32 and none is None and none2 is None
    assert y.data_ptr() == ybuf.data_ptr() and db.data_ptr() == gbuf.data_ptr()
    assert parts.shape == ((n + 7) // 8, 4 * C) and de.shape == (4, C)
    assert torch.equal(y_noarg, y) and torch.equal(db2, db)
    y, arg, db = y.cpu(), arg.cpu(), db.cpu()
    # forward against float64
    fe = f.double() @ e.double()
    for got_y, got_arg, msg in ((y, arg, fe + b.double()[cols]), (y_nob.cpu(), arg_nob.cpu(), fe)):
        rms = float(msg.pow(2).mean().sqrt())
        ref_arg, gap, ref_empty = ppf_winners_and_gaps(rows, cols, msg, n)
        assert torch.equal(ref_empty, empty)
        idx = rows.view(-1, 1).expand(-1, C)
        mx = torch.zeros((n, C), dtype=torch.float64).scatter_reduce(0, idx, msg, "amax", include_self=False)
        err = relerr(got_y, mx)
        print("%s loops=%s C=%d y: rel-L2 %.2e (tolerance %.0e)" % (name, loops, C, err, GATHER_TOL))
        assert err <= GATHER_TOL
        ent = entry_of(rows, cols, n, got_arg)
        ne = ~empty
        won = msg.gather(0, ent[ne])                             # the float64 message of the kernel's winner
        assert float((mx[ne] - won).max()) <= GATHER_TOL * rms
        sure = gap >= AMB_GAP * rms
        assert torch.equal(got_arg.long()[sure], ref_arg[sure])
        assert bool((got_y[empty] == 0).all()) and bool((got_arg[empty] == -1).all())
    # backward against float64 sums over the kernel's own arg
    err_b = relerr(db, db_from_arg(dg, arg, rows, cols, n))
    err_e = relerr(de, de_from_arg(dg, arg, f, rows, cols, n))
    print("%s loops=%s C=%d dB: rel-L2 %.2e, dE: rel-L2 %.2e (tolerance %.0e)" % (name, loops, C, err_b, err_e, GATHER_TOL))
    assert err_b <= GATHER_TOL and err_e <= GATHER_TOL
    for t in (ybuf, gbuf):                                       # the padding columns stay NaN, everything else is finite
        assert bool(torch.isnan(t[:, C:]).all()) and bool(torch.isfinite(t[:, :C]).all())
    assert bool(torch.isfinite(parts).all())


@pytest.mark.parametrize("C", [3, 8, 40])
def test_ties_go_to_the_first_entry(dev, graphs, C):
    """All rows of B equal and all points equal (every F is exactly 0): every entry ties, the first entry in CSR order (the
    smallest source id) wins, and the whole of dG[i] lands on it."""
    from dual_dmp_amd import ops
    ei, eid, n = graphs["hub-iso"]
    rows, cols, empty = host_csr(ei, n, False)
    gen = torch.Generator().manual_seed(C)
    dg, e = torch.randn(n, C, generator=gen), torch.randn(4, C, generator=gen)
    b = torch.randn(1, C, generator=gen).expand(n, C).contiguous()
    pos = torch.tensor([[0.3, -1.7, 2.9]]).expand(n, 3).contiguous()
    nrm = torch.tensor([[0.36, 0.48, 0.8]]).expand(n, 3).contiguous()
    g = ops.graph_for(eid, n, norm="gat", add_self_loops=False)
    fd = ops.ppf_entries(g, pos.to(dev), nrm.to(dev))
    assert bool((fd == 0).all())
    y, arg = ops.gather_max_attr(g, b.to(dev), fd, e.to(dev))
    db, parts = ops.gather_max_attr_bwd(g, dg.to(dev), arg, fd)
    ne = ~empty
    assert bool((cols[1:] > cols[:-1])[rows[1:] == rows[:-1]].all())          # CSR order ascends: the first entry is the smallest id
    first = torch.full((n,), n, dtype=torch.int64).scatter_reduce(0, rows, cols, "amin")
    first[empty] = -1
    assert torch.equal(y.cpu()[ne], b[ne]) and torch.equal(arg.cpu().long(), first.view(-1, 1).expand(-1, C))
    want = torch.zeros((n, C), dtype=torch.float64).index_add_(0, first[ne], dg[ne].double())
    assert relerr(db, want) <= GATHER_TOL and bool((parts == 0).all())


def test_bad_arguments_are_refused(dev, graphs):
    import ctypes
    from dual_dmp_amd import ops
    ei, eid, n = graphs["grid"]
    g = ops.graph_for(eid, n, norm="gat", add_self_loops=False)
    plain = ops.graph_for(eid, n)                                # not a valued graph
    pos, nrm = (t.to(dev) for t in geometry(n, torch.Generator().manual_seed(0)))
    f = ops.ppf_entries(g, pos, nrm)
    b, e = torch.randn(n, 8, device=dev), torch.randn(4, 8, device=dev)
    y, arg = ops.gather_max_attr(g, b, f, e)
    for bad in (lambda: ops.ppf_entries(plain, pos, nrm), lambda: ops.ppf_entries(g, pos.cpu(), nrm),
                lambda: ops.ppf_entries(g, pos[: n - 1], nrm), lambda: ops.ppf_entries(g, pos, nrm.double()),
                lambda: ops.ppf_entries(g, torch.randn(n, 4, device=dev), nrm),
                lambda: ops.gather_max_attr(plain, b, f, e), lambda: ops.gather_max_attr(g, b[: n - 1], f, e),
                lambda: ops.gather_max_attr(g, b.cpu(), f, e), lambda: ops.gather_max_attr(g, b, f[:-1], e),
                lambda: ops.gather_max_attr(g, b, f[:, :3], e), lambda: ops.gather_max_attr(g, b, f.double(), e),
                lambda: ops.gather_max_attr(g, b, f, e[:3]), lambda: ops.gather_max_attr(g, b, f, torch.randn(4, 4, device=dev)),
                lambda: ops.gather_max_attr(g, b, f, e.t().contiguous().t()),
                lambda: ops.gather_max_attr_bwd(plain, b, arg, f), lambda: ops.gather_max_attr_bwd(g, b, arg.long(), f),
                lambda: ops.gather_max_attr_bwd(g, b, arg[:, :4], f), lambda: ops.gather_max_attr_bwd(g, b.cpu(), arg, f),
                lambda: ops.gather_max_attr_bwd(g, b, arg, f[:-1]),
                lambda: ops.gather_max_attr_bwd(g, b, arg, f, out=torch.empty(n, 4, device=dev))):
        with pytest.raises(ops.DdmpError):
            bad()
    L = ops._lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops._stream()
    db = torch.empty_like(b)
    assert L.ddmp_ppf_entries_f32(None, p(pos), 3, p(nrm), 3, p(f), st) != 0
    assert L.ddmp_ppf_entries_f32(plain.handle, p(pos), 3, p(nrm), 3, p(f), st) != 0
    assert L.ddmp_ppf_entries_f32(g.handle, p(pos), 2, p(nrm), 3, p(f), st) != 0
    assert L.ddmp_ppf_entries_f32(g.handle, p(pos), 3, None, 3, p(f), st) != 0
    assert L.ddmp_ppf_entries_f32(g.handle, p(pos), 3, p(nrm), 3, p(pos), st) != 0
    assert L.ddmp_gather_max_attr_f32(None, p(b), 8, p(f), p(e), 8, p(y), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_attr_f32(plain.handle, p(b), 8, p(f), p(e), 8, p(y), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_attr_f32(g.handle, p(b), 8, p(f), p(e), 0, p(y), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_attr_f32(g.handle, p(b), 4, p(f), p(e), 8, p(y), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_attr_f32(g.handle, p(b), 8, None, p(e), 8, p(y), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_attr_f32(g.handle, p(b), 8, p(f), None, 8, p(y), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_attr_f32(g.handle, p(b), 8, p(f), p(e), 8, p(b), 8, None, 0, st) != 0
    assert L.ddmp_gather_max_attr_f32(g.handle, p(b), 8, p(f), p(e), 8, p(y), 8, p(arg), 4, st) != 0
    assert L.ddmp_gather_max_attr_bwd_f32(g.handle, p(b), 8, p(arg), 4, p(f), 8, p(db), 8, None, st) != 0
    assert L.ddmp_gather_max_attr_bwd_f32(g.handle, p(b), 8, None, 8, p(f), 8, p(db), 8, None, st) != 0
    assert L.ddmp_gather_max_attr_bwd_f32(g.handle, p(b), 8, p(arg), 8, None, 8, p(db), 8, None, st) != 0
    assert L.ddmp_gather_max_attr_bwd_f32(g.handle, p(b), 8, p(arg), 8, p(f), 8, p(b), 8, None, st) != 0
    assert L.ddmp_gather_max_attr_bwd_f32(g.handle, p(b), 8, p(arg), 8, p(f), 8, p(db), 8, p(db), st) != 0
    assert L.ddmp_gather_max_attr_bwd_f32(plain.handle, p(b), 8, p(arg), 8, p(f), 8, p(db), 8, None, st) != 0


# ------------------------------------------------------------------------------------------------ 3. the operator
def _make_local(cin, cout, kind, gen):
    a = 1.0 / math.sqrt(cin + 4)
    lin = nn.Linear(cin + 4, cout, bias=kind != "nobias")
    with torch.no_grad():
        for p in lin.parameters():
            p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * a)
    return nn.Sequential(lin, nn.LeakyReLU(0.2)) if kind == "leaky" else lin


def _lin_of(fn):
    return fn[0] if isinstance(fn, nn.Sequential) else fn


def _run(conv, x, pos, nrm, ei, t):
    x = None if x is None else x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, pos, nrm, ei)
    (y * t).sum().backward()
    return [y.detach()] + ([x.grad] if x is not None else []) + [p.grad for p in conv.parameters()]


def _record_arg(monkeypatch):
    """Every arg ``ops.gather_max_attr`` returns from here on, in call order."""
    from dual_dmp_amd import ops
    args, real = [], ops.gather_max_attr

    def recording(*a, **kw):
        y, arg = real(*a, **kw)
        args.append(arg)
        return y, arg

    monkeypatch.setattr(ops, "gather_max_attr", recording)
    return args


@pytest.mark.parametrize("cin,cout", CASES)
@pytest.mark.parametrize("name", ["ico-iso", "grid", "hub-iso"])
@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("kind", ["bias", "nobias", "leaky"])
def test_operator_matches_the_float64_reference(dev, graphs, monkeypatch, cin, cout, name, loops, kind):
    from dual_dmp_amd.nn_ops import PPFConv
    ei, eid, n = graphs[name]
    gen = torch.Generator().manual_seed(n + cout)
    pos, nrm = geometry(n, gen)
    x = torch.randn(n, cin, generator=gen) if cin else None
    fn = _make_local(cin, cout, kind, gen)
    t = torch.randn(n, cout, generator=gen)
    ref = PPFConvRef(fn, add_self_loops=loops)
    x64 = None if x is None else x.double()
    dst, src, msg = ppf_messages(x64, pos.double(), nrm.double(), ei, _lin_of(ref.local_nn).weight.detach(), loops)
    ref_arg, gap, _ = ppf_winners_and_gaps(dst, src, msg, n)
    rms = float(msg.pow(2).mean().sqrt())
    amb = gap < AMB_GAP * rms
    share = float(amb.double().mean())
    print("%s (%d, %d) %s loops=%s: ambiguous share %.3f %% (limit %.0f %%), smallest gap %.1e rms"
          % (name, cin, cout, kind, loops, 100 * share, 100 * AMB_SHARE, float(gap.min()) / rms))
    assert share <= AMB_SHARE
    t = t.masked_fill(amb, 0.0)
    want = _run(ref, x64, pos.double(), nrm.double(), ei, t.double())
    args = _record_arg(monkeypatch)
    conv = PPFConv(fn, add_self_loops=loops).to(dev)
    got = _run(conv, None if x is None else x.to(dev), pos.to(dev), nrm.to(dev), eid, t.to(dev))
    assert len(args) == 1 and torch.equal(args[0].cpu().long()[~amb], ref_arg[~amb])
    names = (["y"] + (["dx"] if cin else []) + ["dW"] + ([] if kind == "nobias" else ["db"]))
    assert len(got) == len(want) == len(names)
    for k, a, b in zip(names, got, want):
        assert a.shape == b.shape, k
        e = relerr(a, b)
        print("%s: rel-L2 %.2e (tolerance %.0e)" % (k, e, OP_TOL))
        assert e <= OP_TOL, (k, e)


def test_global_nn_runs_on_the_result(dev, graphs):
    from dual_dmp_amd.nn_ops import PPFConv
    ei, eid, n = graphs["grid"]
    gen = torch.Generator().manual_seed(11)
    pos, nrm = geometry(n, gen)
    x, t = torch.randn(n, 6, generator=gen), torch.randn(n, 5, generator=gen)
    torch.manual_seed(2)
    local, glob = _make_local(6, 12, "leaky", gen), nn.Sequential(nn.Linear(12, 5), nn.Tanh())
    want = _run(PPFConvRef(local, glob), x.double(), pos.double(), nrm.double(), ei, t.double())
    got = _run(PPFConv(local, glob).to(dev), x.to(dev), pos.to(dev), nrm.to(dev), eid, t.to(dev))
    assert len(got) == len(want) == 6
    for a, b in zip(got, want):
        assert relerr(a, b) <= OP_TOL


def test_no_grad_forward_keeps_no_arg(dev, graphs, monkeypatch):
    from dual_dmp_amd.nn_ops import PPFConv
    ei, eid, n = graphs["grid"]
    args = _record_arg(monkeypatch)
    conv = PPFConv(nn.Linear(12, 12)).to(dev)
    pos, nrm = (t.to(dev) for t in geometry(n, torch.Generator().manual_seed(1)))
    x = torch.randn(n, 8, device=dev)
    with torch.no_grad():
        y0 = conv(x, pos, nrm, eid)
    y1 = conv(x, pos, nrm, eid)
    assert args[0] is None and args[1] is not None and torch.equal(y0, y1.detach())


def test_two_runs_give_the_same_bits(dev, graphs, monkeypatch):
    from dual_dmp_amd.nn_ops import PPFConv
    ei, eid, n = graphs["hub"]
    args = _record_arg(monkeypatch)
    pos, nrm = (t.to(dev) for t in geometry(n, torch.Generator().manual_seed(3)))
    for cin, cout in CASES:
        torch.manual_seed(1)
        conv = PPFConv(nn.Sequential(nn.Linear(cin + 4, cout), nn.LeakyReLU(0.2))).to(dev)
        x, t = (torch.randn(n, cin, device=dev) if cin else None), torch.randn(n, cout, device=dev)
        del args[:]
        a = [v.clone() for v in _run(conv, x, pos, nrm, eid, t)]
        b = _run(conv, x, pos, nrm, eid, t)
        assert len(a) == (4 if cin else 3) and torch.equal(args[0], args[1])
        for k, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), (cin, cout, k)


# ------------------------------------------------------------------------------------------------ 4. index width
def test_offsets_beyond_2_31_bytes(dev):
    """1,100,000-node vertex graph of a torus, C = 256, B one half of one [N, 512] buffer: N * 512 * 4 bytes = 2.25e9 > 2^31.
    Forward and backward once; y, arg, dB and the 8-row partials of 250 sampled 8-row groups (2,000 rows, the last sixteen rows
    among them) are recomputed on the CPU from their one-ring neighbourhoods."""
    from dual_dmp_amd import ops, synth
    C = 256
    v, f = synth.torus(1100, 1000)
    n = len(v)
    assert n == 1100000 and n * 2 * C * 4 > 2 ** 31 and n % 8 == 0
    f = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // n, key % n])).contiguous()
    t = ops.csr_build_valued_host(ei.numpy(), n, 0)
    rowptr, col = t["rowptr"].astype(np.int64), t["col"].astype(np.int64)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    torch.manual_seed(7)
    buf = torch.randn(n, 2 * C, device=dev)
    b = buf[:, C:]
    dg = torch.randn(n, C, device=dev)
    ed = torch.randn(4, C, device=dev) * 0.5
    nrm = torch.randn(n, 3, device=dev)
    fd = ops.ppf_entries(g, torch.randn(n, 3, device=dev), nrm / nrm.norm(dim=1, keepdim=True))
    y, arg = ops.gather_max_attr(g, b, fd, ed)
    db, parts = ops.gather_max_attr_bwd(g, dg, arg, fd)
    torch.cuda.synchronize()
    assert parts.shape == (n // 8, 4 * C)
    # sampled 8-row groups, the last two among them: the largest offsets
    rng = np.random.default_rng(0)
    grp = np.unique(np.concatenate([rng.choice(n // 8 - 2, 248, replace=False), np.arange(n // 8 - 2, n // 8)]))
    s0 = (grp[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
    assert len(s0) == 2000 and s0[-1] == n - 1
    ent = np.concatenate([np.arange(rowptr[r], rowptr[r + 1]) for r in s0])
    cnt = rowptr[s0 + 1] - rowptr[s0]
    assert cnt.min() > 0
    erow, ecol = np.repeat(s0, cnt), col[ent]
    i0 = torch.from_numpy(np.repeat(np.arange(len(s0)), cnt))
    fetch = lambda m, r: m[torch.from_numpy(r).to(dev)].cpu()
    idx = i0.view(-1, 1).expand(-1, C)
    fe = fetch(fd, ent).double()
    msg = fe @ ed.cpu().double() + fetch(b, ecol).double()
    rms = float(msg.pow(2).mean().sqrt())
    mx = torch.full((len(s0), C), -float("inf"), dtype=torch.float64).scatter_reduce(0, idx, msg, "amax")
    ys, args_ = fetch(y, s0), fetch(arg, s0).long()
    err = relerr(ys, mx)
    match = torch.from_numpy(ecol).view(-1, 1) == args_[i0]      # [entries, C]: the entry the kernel's winner names
    assert bool((torch.zeros((len(s0), C)).index_add_(0, i0, match.float()) == 1).all())
    won = torch.zeros((len(s0), C), dtype=torch.float64).index_add_(0, i0, torch.where(match, msg, torch.zeros((), dtype=torch.float64)))
    assert err <= GATHER_TOL and float((mx - won).max()) <= GATHER_TOL * rms
    hit = fetch(arg, ecol).long() == torch.from_numpy(erow).view(-1, 1)
    want_b = torch.zeros((len(s0), C), dtype=torch.float64).index_add_(0, i0, torch.where(hit, fetch(dg, ecol).double(), torch.zeros((), dtype=torch.float64)))
    err_b = relerr(fetch(db, s0), want_b)
    dgs = fetch(dg, s0).double()
    per = fe.unsqueeze(-1) * (match.double() * dgs[i0]).unsqueeze(1)                           # [entries, 4, C]
    want_p = torch.zeros((len(grp), 4, C), dtype=torch.float64).index_add_(0, i0 // 8, per).reshape(len(grp), 4 * C)
    err_p = relerr(fetch(parts, grp), want_p)
    print("1.1M nodes x 256: y rel-L2 %.2e, dB %.2e, partials %.2e over %d sampled rows (tolerance %.0e)" % (err, err_b, err_p, len(s0), GATHER_TOL))
    assert err_b <= GATHER_TOL and err_p <= GATHER_TOL


# ------------------------------------------------------------------------------------------------ 5. nets
def test_normalnet_runs_with_conv_ppf(dev, monkeypatch):
    from dual_dmp_amd import ops
    from dual_dmp_amd.networks import NormalNet
    from dual_dmp_amd.nn_ops import PPFConv
    gt, noisy, smooth, data = OJ.case("ico3")
    torch.manual_seed(6)
    net = NormalNet(dev, fused=False, conv="ppf")
    assert all(isinstance(getattr(net, "conv%d" % i), PPFConv) for i in range(1, 13))
    feats, real = [], ops.ppf_entries
    monkeypatch.setattr(ops, "ppf_entries", lambda *a: feats.append(real(*a)) or feats[-1])
    net.train()
    o = net(data)
    assert o.shape == (len(noisy.faces), 3) and bool(torch.isfinite(o).all())
    o.backward(torch.randn(len(noisy.faces), 3, device=dev))
    for name, p in net.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name
    net(data)                                                    # a second forward reuses the cached features
    assert len(feats) == 24 and all(f is feats[0] for f in feats)

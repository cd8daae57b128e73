"""PNAConv on the GPU: the fused neighbour-moments gather and its backward (``ops.gather_moments`` / ``ops.gather_moments_bwd``) and the
drop-in against the float64 edge-list reference (tests/pna_ref.py) on icosphere(3) (645 rows with the special ones: more chunks than
XCDs and a partial last chunk), the open grid (boundary) and the hub graph (one 1200-entry row), with test_gpu_sage.py's duplicate
edges and explicit loops on top, and with one pendant node, one node whose entries are all the same source, and one edgeless node.

Tolerance policy (the project's: ``GATHER_TOL`` = 1e-6 and ``OP_TOL`` = 1e-5, both rel-L2):
* kernel level, on exact float32 inputs: Mx / Mn are comparisons and one addition of the root, so they must equal torch's float32
  ``segment_max(B) + R`` bit for bit; the args must be the smallest source id that attains the extremum, -1 on an empty row; invdeg
  is one correctly rounded division: exact; without a root and with tw == C every block and arg that ``ops.gather_stats`` also has
  carries its bits; a block of a fused call has the bits of the same block requested alone; the mean, the sum, mu, var and std
  differ from a float64 TWO-PASS evaluation on the same float32 inputs only in rounding and summation order: <= GATHER_TOL.
* the std threshold: std switches to 0 at var <= 1e-5, so an input whose float64 variance lies in (0, 1e-4) could legitimately land
  on either side; the inputs are chosen (by seed, asserted) so that none does, and nothing has to be left out.  Rows whose
  variance is exactly 0 (the pendant node, the one-source node) must give exactly 0.
* the hard column B = 1000 + N(0, 1): var and std <= 1e-5 rel-L2 against float64.  A float32 mean(x^2) - mean(x)^2 is off by 5e-2
  to 9e-2 in var there (1.4e-1 to 2.3e-1 in std), the first-entry-shifted float32 sums by 6e-7 (CPU restatements on these meshes).
* backward kernel: dB against a float64 evaluation of the formula from the kernel's own args, invdeg and mu: <= GATHER_TOL.
* operator level, against ``PNAConvRef`` in float64: test_gpu_sage.py's near-tie policy unchanged.  An output (i, c) of a max / min
  block whose float64 top-two gap is below 1e-3 x rms(B) is ambiguous; the gradient reaching it is zeroed on both sides, the
  ambiguous share must stay <= 1 % (printed), the arg must equal the reference winner everywhere else, and y, dx and every
  parameter gradient meet OP_TOL.  A gradient that is exactly 0 in exact arithmetic (the pre bias under std / var alone) is compared
  with the reference norm floored at 1.
* the hard-column input at operator level (x = 1000 + N(0, 1)): the same bound, OP_TOL, for y, dx and every parameter gradient.
  The operator centres x by its first row before the pre GEMM (the message is invariant to it), so B is of the size of the
  features' spread and std / var and their chain rule are as well conditioned as at any other input."""
import ctypes
import itertools

import pytest
import torch

import edge_weight_route_worker as W
import gat_ops_stub
from pna_ref import PNAConvRef, degree_histogram, extremum_winners, moments64
from test_pna_cpu import AGGRS, DIMS, SCALERS, ids, with_special_rows

pytestmark = pytest.mark.gpu
relerr = W.relerr

OP_TOL = 1e-5
GATHER_TOL = 1e-6
HARD_TOL = 1e-5
AMB_GAP = 1e-3                  # x rms(B)
AMB_SHARE = 0.01

# (C, tw): the scalar path, one float4, a full slab, a ragged width, two slabs; towers of 8, of 20, and of 6 (scalar path)
LAYOUTS = [(3, 3), (4, 4), (32, 32), (40, 40), (64, 64), (32, 8), (40, 20), (12, 6)]
NAMES = ["ico", "grid", "hub"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graphs():
    """name -> (edge_index, n): the route worker's graphs + test_gpu_sage.py's duplicates and explicit loops (two on node 5), then
    the pendant node n - 3, the one-source node n - 2 and the edgeless node n - 1."""
    out = {}
    base = W.graphs()
    for name in NAMES:
        ei, n = base[name]
        extra = torch.tensor([[3, 9, 5, 5, 40], [9, 3, 5, 5, 40]])
        dup = ei[:, :50]
        out[name] = with_special_rows(torch.cat([ei, extra, dup, dup[[1, 0]]], 1).contiguous(), n)
    assert out["ico"][1] == 645
    return out


@pytest.fixture(scope="module")
def host(graphs):
    """name -> the HOST structure of the valued graph without loop handling (row, col, a, mirror, rowptr of the coalesced CSR)."""
    return {name: gat_ops_stub.Graph(ei, n, 0) for name, (ei, n) in graphs.items()}


def _rowsum64(h, v):
    return torch.zeros((h.n_rows,) + tuple(v.shape[1:]), dtype=torch.float64).index_add_(0, h.row, v)


def _segment(x, h, op):
    idx = h.row.view(-1, 1).expand(-1, x.shape[1])
    return torch.zeros((h.n_rows, x.shape[1])).scatter_reduce(0, idx, x[h.col], op, include_self=False)


def _inputs(h, n, C, seed, offset=0.0):
    """float32 B = offset + N(0, 1) [n, C] from the first seed >= ``seed`` whose float64 variances avoid (0, 1e-4) (asserted): the
    std threshold then cannot be met from the other side, and nothing has to be left out."""
    for s in range(seed, seed + 8):
        b = (offset + torch.randn(n, C, generator=torch.Generator().manual_seed(s))).float()
        var = moments64(b, h)[3]
        if not bool(((var > 0) & (var < 1e-4)).any()):
            break
    assert not bool(((var > 0) & (var < 1e-4)).any()), "no seed in [%d, %d) keeps the variances out of (0, 1e-4)" % (seed, seed + 8)
    return b


def _std64(var):
    return torch.where(var > 1e-5, var.sqrt(), torch.zeros((), dtype=torch.float64))


def _flat(blk):
    return blk.reshape(blk.shape[0], -1).cpu()


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("C,tw", LAYOUTS)
def test_kernels_match_torch(dev, graphs, host, name, C, tw):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    h = host[name]
    b = _inputs(h, n, C, n + C)
    r = torch.randn(n, C, generator=torch.Generator().manual_seed(C))
    has = (h.rowptr[1:] > h.rowptr[:-1]).view(-1, 1)
    assert int((~has).sum()) == 1
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    assert g.nnz == h.nnz
    s64, deg, mean64, var64 = moments64(b, h)
    assert float(deg.sum()) == ei.shape[1]                       # every input edge counts, duplicates and loops included
    inv32 = torch.where(has.view(-1), 1.0 / deg.float(), torch.zeros(()))
    seg = {"max": _segment(b, h, "amax"), "min": _segment(b, h, "amin")}
    ref_arg = {k: extremum_winners(b, ei, n, k)[0] for k in ("max", "min")}
    bd, T = b.to(dev), C // tw
    for root in (None, r):
        rd = None if root is None else root.to(dev)
        r64 = torch.zeros((n, C), dtype=torch.float64) if root is None else root.double()
        zero = torch.zeros((), dtype=torch.float64)
        ref = {"sum": torch.where(has, s64 + deg.view(-1, 1) * r64, zero), "mean": torch.where(has, mean64 + r64, zero),
               "var": var64, "std": _std64(var64)}
        alone = {}
        for k in ops.MOMENTS:                                    # each statistic on its own
            (blk,), (arg,), invdeg, mu = ops.gather_moments(g, bd, want=(k,), root=rd, tower_width=tw)
            assert tuple(blk.shape) == ((n, C) if T == 1 else (n, T, tw))
            alone[k] = (_flat(blk), None if arg is None else arg.cpu(), None if mu is None else mu.cpu())
            assert torch.equal(invdeg.cpu(), inv32)              # exact
            assert (mu is not None) == (k in ("std", "var")) and (arg is not None) == (k in ("max", "min"))
            if k in ("max", "min"):
                want = seg[k] if root is None else torch.where(has, seg[k] + root, torch.zeros(()))
                assert torch.equal(alone[k][0], want)            # bit for bit; an empty row gets 0 whatever the root is
                assert torch.equal(arg.cpu().long(), ref_arg[k])  # the smallest source id attaining it, -1 on an empty row
            else:
                e = relerr(alone[k][0], ref[k])
                print("%s C=%d tw=%d root=%s %s alone: rel-L2 %.2e (tolerance %.0e)" % (name, C, tw, root is not None, k, e, GATHER_TOL))
                assert e <= GATHER_TOL, (k, e)
                assert bool((alone[k][0][~has.view(-1)] == 0).all())
            if mu is not None:
                e = relerr(mu, mean64)
                assert e <= GATHER_TOL and bool((mu.cpu()[~has.view(-1)] == 0).all()), e
                for row in (n - 3, n - 2):                       # variance exactly 0: exactly 0 out
                    assert bool((alone[k][0][row] == 0).all()), (k, row)
        for want in (("mean", "min", "max", "std"), ("sum", "max", "min", "var"), ("std", "mean"), ("var",), ("min", "sum")):
            nb = len(want)
            width = (nb * C + 3) // 4 * 4 + 4
            buf = torch.full((n, width), float("nan"), device=dev)
            blocks, args, invdeg, mu = ops.gather_moments(g, bd, want=want, root=rd, tower_width=tw, out=buf)
            again = torch.full((n, width), float("nan"), device=dev)
            _, args2, _, mu2 = ops.gather_moments(g, bd, want=want, root=rd, tower_width=tw, out=again)
            torch.cuda.synchronize()
            assert bool(torch.isnan(buf[:, nb * C:]).all()) and bool(torch.isfinite(buf[:, :nb * C]).all())
            assert torch.equal(buf[:, :nb * C], again[:, :nb * C])                          # two calls, equal bits
            # the tower-major layout: [tower][statistic][tw], every block with the bits of the block requested alone
            layout = torch.stack([alone[k][0].view(n, T, tw) for k in want], 2).reshape(n, nb * C)
            assert torch.equal(buf[:, :nb * C].cpu(), layout), want
            for k, blk, arg, arg2 in zip(want, blocks, args, args2):
                assert torch.equal(_flat(blk), alone[k][0]), (want, k)
                if arg is not None:
                    assert torch.equal(arg.cpu(), alone[k][1]) and torch.equal(arg, arg2), (want, k)
                if k in ("std", "var"):
                    assert torch.equal(mu.cpu(), alone[k][2]) and torch.equal(mu, mu2)
            noarg = ops.gather_moments(g, bd, want=want, root=rd, tower_width=tw, want_arg=False)
            assert all(a is None for a in noarg[1]) and all(torch.equal(u, v) for u, v in zip(noarg[0], blocks))
        if root is None and tw == C:                             # the shared blocks and args: the bits of ops.gather_stats
            (s, mx, mn), (_, amx, amn), inv = ops.gather_stats(g, bd, want=("mean", "max", "min"))
            (sa,), _, _ = ops.gather_stats(g, bd, want=("add",))
            for k, blk, arg in (("mean", s, None), ("max", mx, amx), ("min", mn, amn), ("sum", sa, None)):
                assert torch.equal(blk.cpu(), alone[k][0]), k
                assert arg is None or torch.equal(arg.cpu(), alone[k][1]), k
            assert torch.equal(inv.cpu(), inv32)


# ------------------------------------------------------------------------------------------------ 2. / 3. threshold, hard column
@pytest.mark.parametrize("name", NAMES)
def test_std_threshold_and_zero_variance_rows(dev, graphs, host, name):
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    h = host[name]
    b = _inputs(h, n, 8, 0)
    var64 = moments64(b, h)[3]
    assert not bool(((var64 > 0) & (var64 < 1e-4)).any())        # nothing near the threshold: nothing has to be left out
    zero_rows = (var64 == 0).all(1)
    assert bool(zero_rows[n - 3]) and bool(zero_rows[n - 2]) and bool(zero_rows[n - 1]) and int(zero_rows.sum()) == 3
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    for k in ("std", "var"):
        (v,), _, _, mu = ops.gather_moments(g, b.to(dev), want=(k,))
        v = v.cpu()
        assert bool((v[zero_rows] == 0).all()) and bool((v[~zero_rows] > 0).all())
        e = relerr(v, var64 if k == "var" else _std64(var64))
        print("%s %s: rel-L2 %.2e (tolerance %.0e)" % (name, k, e, GATHER_TOL))
        assert e <= GATHER_TOL
    assert torch.equal(mu.cpu()[n - 3], b[0])                    # the pendant node's mean is its one neighbour, exactly


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("C", [8, 3])
def test_hard_column(dev, graphs, host, name, C):
    """B = 1000 + N(0, 1): the variance is ~1 and the squares are ~1e6."""
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    h = host[name]
    b = _inputs(h, n, C, 0, offset=1000.0)
    _, _, mean64, var64 = moments64(b, h)
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    for k in ("var", "std"):
        (v,), _, _, mu = ops.gather_moments(g, b.to(dev), want=(k,))
        e = relerr(v, var64 if k == "var" else _std64(var64))
        print("%s C=%d hard column %s: rel-L2 %.2e (tolerance %.0e)" % (name, C, k, e, HARD_TOL))
        assert e <= HARD_TOL, (k, e)
        assert relerr(mu, mean64) <= GATHER_TOL
    (_, v), _, _, _ = ops.gather_moments(g, b.to(dev), want=("mean", "std"), root=torch.randn(n, C).to(dev))
    assert relerr(v, _std64(var64)) <= HARD_TOL                  # the root is never added to the moment


# ------------------------------------------------------------------------------------------------ 4. the backward kernel
# every subset of the streams {dS (the sum family), dQ (std / var; it comes with dS), max, min} that PNAConv can produce
BWD_SUBSETS = [s for r in (1, 2, 3, 4) for s in itertools.combinations(("s", "q", "x", "n"), r) if "q" not in s or "s" in s]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("C", [3, 4, 40, 64])
def test_backward_kernel(dev, graphs, host, name, C):
    from dual_dmp_amd import ops
    assert len(BWD_SUBSETS) == 11
    ei, n = graphs[name]
    h = host[name]
    gen = torch.Generator().manual_seed(n + C)
    b, ds, dq, dmx, dmn = (torch.randn(n, C, generator=gen) for _ in range(5))
    b = b + 3.0
    empty = h.rowptr[1:] == h.rowptr[:-1]
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    bd = b.to(dev)
    _, (amx, amn, _), invdeg, mu = ops.gather_moments(g, bd, want=("max", "min", "std"))
    inv64 = invdeg.cpu().double()
    dev_of = {"s": ds.to(dev), "q": dq.to(dev), "x": dmx.to(dev), "n": dmn.to(dev)}
    for subset in BWD_SUBSETS:
        for weighted in (True, False):
            f = h.a[h.mirror] * (inv64[h.col] if weighted else 1.0)
            want64 = torch.zeros((n, C), dtype=torch.float64)
            op = {}
            if "s" in subset:
                op["ds"], op["invdeg"] = dev_of["s"], (invdeg if weighted else None)
                want64 += _rowsum64(h, f.view(-1, 1) * ds.double()[h.col])
            if "q" in subset:
                op["dq"], op["b"] = dev_of["q"], bd
                want64 += b.double() * _rowsum64(h, f.view(-1, 1) * dq.double()[h.col])
            for key, dm, arg in (("x", dmx, amx), ("n", dmn, amn)):
                if key in subset:
                    op["d" + ("mx" if key == "x" else "mn")], op["arg" + ("mx" if key == "x" else "mn")] = dev_of[key], arg
                    hit = arg.cpu().long()[h.col] == h.row.view(-1, 1)
                    want64 += _rowsum64(h, torch.where(hit, dm.double()[h.col], torch.zeros((), dtype=torch.float64)))
            if "s" not in subset and not weighted:
                continue                                         # (without dS the factor is not read: one run is enough)
            gbuf = torch.full((n, (2 * C + 3) // 4 * 4 + 4), float("nan"), device=dev)
            cp = (C + 3) // 4 * 4
            db = ops.gather_moments_bwd(g, out=gbuf[:, cp:cp + C], **op)                    # a column block of a wider buffer
            db2 = ops.gather_moments_bwd(g, **op)
            torch.cuda.synchronize()
            assert db.data_ptr() == gbuf[:, cp:].data_ptr() and torch.equal(db, db2)        # two calls, equal bits
            assert bool(torch.isnan(gbuf[:, :cp]).all()) and bool(torch.isnan(gbuf[:, cp + C:]).all())
            e = relerr(db, want64)
            print("%s C=%d %s weighted=%s dB: rel-L2 %.2e (tolerance %.0e)" % (name, C, "".join(subset), weighted, e, GATHER_TOL))
            assert e <= GATHER_TOL, (subset, e)
            assert bool((db.cpu()[empty] == 0).all())            # a row without entries gets zeros


@pytest.mark.parametrize("name", ["hub", "ico"])                 # the long row; the pendant, one-source and edgeless rows
@pytest.mark.parametrize("C", [3, 4, 40])                        # the scalar path, one float4, a ragged width
def test_backward_has_the_bits_of_gather_stats_bwd(dev, graphs, name, C):
    """For the streams that both backward entry points know (dS with and without invdeg, the maximum's, the minimum's) nstat.hip and
    pna.hip perform the same operations in the same order, so the bits are equal -- the backward's counterpart of the forward
    equality that ``test_kernels_match_torch`` asserts, and the guard that a fix to one copy reaches the other."""
    from dual_dmp_amd import ops
    ei, n = graphs[name]
    gen = torch.Generator().manual_seed(n + C)
    b, ds, dmx, dmn = (torch.randn(n, C, generator=gen).to(dev) for _ in range(4))
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    _, (_, amx, amn), invdeg, _ = ops.gather_moments(g, b, want=("mean", "max", "min"))
    for streams in (dict(ds=ds, invdeg=invdeg), dict(ds=ds), dict(dmx=dmx, argmx=amx), dict(dmn=dmn, argmn=amn),
                    dict(ds=ds, invdeg=invdeg, dmx=dmx, argmx=amx, dmn=dmn, argmn=amn)):
        assert torch.equal(ops.gather_stats_bwd(g, **streams)[0], ops.gather_moments_bwd(g, **streams)), sorted(streams)


# ------------------------------------------------------------------------------------------------ 5. the operator
def _record(monkeypatch, masks):
    """Every ``ops.gather_moments`` result from here on, in call order; and the gradients reaching the ambiguous outputs of the
    max / min blocks (``masks``: {"max": bool [n, T F], "min": ...}) are zeroed where the operator's backward hands the blocks'
    gradients to the aggregators' chain rule (``nn_ops._pna_aggr_bwd``), as the reference's hook zeroes them."""
    from dual_dmp_amd import nn_ops, ops
    seen, fwd, chain = [], ops.gather_moments, nn_ops._pna_aggr_bwd

    def recording(*a, **kw):
        out = fwd(*a, **kw)
        seen.append((tuple(kw.get("want", ("mean",))), out))
        return out

    def masking(graph, aggrs, grads, *rest):
        grads = [d.masked_fill(masks[k].to(d.device), 0.0) if k in masks else d for k, d in zip(aggrs, grads)]
        return chain(graph, aggrs, grads, *rest)

    monkeypatch.setattr(ops, "gather_moments", recording)
    monkeypatch.setattr(nn_ops, "_pna_aggr_bwd", masking)
    return seen


def _run(conv, x, ei, t):
    x = x.clone().requires_grad_(True)
    for p in conv.parameters():
        p.grad = None
    y = conv(x, ei)
    (y * t).sum().backward()
    return dict([("y", y.detach()), ("dx", x.grad)] + [(k, p.grad) for k, p in conv.named_parameters()])


def _floored(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1.0))


def _operator_case(dev, graphs, monkeypatch, name, cin, cout, towers, aggrs, scalers, offset=0.0):
    """(got, want) of the drop-in and of the float64 reference under the ambiguity policy."""
    from dual_dmp_amd.nn_ops import PNAConv
    ei, n = graphs[name]
    gen = torch.Generator().manual_seed(n + cin)
    x = (offset + torch.randn(n, cin, generator=gen)).float()
    t = torch.randn(n, cout, generator=gen)
    torch.manual_seed(n + cout)
    deg = degree_histogram(ei, n)
    ref = PNAConvRef(cin, cout, aggrs, scalers, deg, towers)
    b64 = torch.cat([x.double() @ s[0].weight.detach()[:, cin:].t() for s in ref.pre_nns], 1)                 # B [n, T F]
    rms = float(b64.pow(2).mean().sqrt())
    masks, winners = {}, {}
    for k in aggrs:
        if k in ("max", "min"):
            winners[k], gap, _ = extremum_winners(b64, ei, n, k)
            masks[k] = gap < AMB_GAP * rms
            share = float(masks[k].double().mean())
            print("%s (%d, %d, %d) %s: ambiguous share of %s %.3f %% (limit %.0f %%), smallest gap %.1e rms"
                  % (name, cin, cout, towers, ids(aggrs), k, 100 * share, 100 * AMB_SHARE, float(gap.min()) / rms))
            assert share <= AMB_SHARE
    ref.on_block = lambda k, blk: (blk.register_hook(lambda grad, k=k: grad.masked_fill(masks[k].view(grad.shape), 0.0))
                                   if k in masks else None)
    want = _run(ref, x.double(), ei, t.double())
    seen = _record(monkeypatch, masks)
    conv = PNAConv(cin, cout, aggrs, scalers, deg, towers=towers).to(dev)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    got = _run(conv, x.to(dev), ei.to(dev), t.to(dev))
    assert len(seen) == 1 and seen[0][0] == tuple(aggrs)
    for k, arg in zip(aggrs, seen[0][1][1]):
        if k in masks:
            assert torch.equal(arg.cpu().long()[~masks[k]], winners[k][~masks[k]]), k
    return got, want


@pytest.mark.parametrize("cin,cout,towers", DIMS)
@pytest.mark.parametrize("aggrs", AGGRS, ids=ids)
@pytest.mark.parametrize("scalers", SCALERS, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_operator_matches_the_float64_reference(dev, graphs, monkeypatch, name, cin, cout, towers, aggrs, scalers):
    got, want = _operator_case(dev, graphs, monkeypatch, name, cin, cout, towers, aggrs, scalers)
    assert sorted(got) == sorted(want) and len(got) == 2 + 4 * towers + 2
    for k in want:
        assert got[k].shape == want[k].shape, k
        e = _floored(got[k], want[k])
        print("%s: rel-L2 %.2e (tolerance %.0e)" % (k, e, OP_TOL))
        assert e <= OP_TOL, (k, e)


@pytest.mark.parametrize("aggrs", [["std"], ["sum", "var"]], ids=ids)
def test_operator_at_the_hard_column(dev, graphs, monkeypatch, aggrs):
    """x = 1000 + N(0, 1): y, dx and every parameter gradient at the operator tolerance."""
    got, want = _operator_case(dev, graphs, monkeypatch, "grid", 8, 8, 2, aggrs, SCALERS[0], offset=1000.0)
    assert sorted(got) == sorted(want)
    for k in want:
        e = _floored(got[k], want[k])
        print("hard column %s %s: rel-L2 %.2e (tolerance %.0e)" % (ids(aggrs), k, e, OP_TOL))
        assert e <= OP_TOL, (k, e)


def test_no_grad_forward_keeps_no_arg_and_two_runs_give_the_same_bits(dev, graphs, monkeypatch):
    from dual_dmp_amd.nn_ops import PNAConv
    ei, n = graphs["hub"]
    eid = ei.to(dev)
    seen = _record(monkeypatch, {})
    deg = degree_histogram(ei, n)
    for cin, cout, towers in DIMS:
        torch.manual_seed(1)
        conv = PNAConv(cin, cout, ["mean", "min", "max", "std"], SCALERS[0], deg, towers=towers).to(dev)
        x, t = torch.randn(n, cin, device=dev), torch.randn(n, cout, device=dev)
        del seen[:]
        with torch.no_grad():
            y0 = conv(x, eid)
        a = {k: v.clone() for k, v in _run(conv, x, eid, t).items()}
        b = _run(conv, x, eid, t)
        assert all(arg is None for arg in seen[0][1][1]) and seen[1][1][1][1] is not None and torch.equal(y0, a["y"])
        for k in a:
            assert torch.equal(a[k], b[k]), (cin, cout, towers, k)


# ------------------------------------------------------------------------------------------------ training
class _Net(torch.nn.Module):
    def __init__(self, make):
        super().__init__()
        self.conv1, self.conv2, self.act = make(3, 16, 2), make(16, 3, 1), torch.nn.LeakyReLU(0.2)

    def forward(self, x, ei):
        return self.conv2(self.act(self.conv1(x, ei)), ei)


def test_two_layer_net_follows_the_reference_for_five_sgd_steps(dev, graphs):
    """Free-running: both nets start from the same parameters and take their own five SGD steps; the loss and the whole
    parameter vector are compared at every step."""
    from dual_dmp_amd.nn_ops import PNAConv
    ei, n = graphs["ico"]
    gen = torch.Generator().manual_seed(n)
    x, target = torch.randn(n, 3, generator=gen), torch.randn(n, 3, generator=gen)
    deg = degree_histogram(ei, n)
    aggrs, scalers = ["mean", "max", "std"], ["identity", "amplification", "attenuation"]
    torch.manual_seed(3)
    ref = _Net(lambda i, o, t: PNAConvRef(i, o, aggrs, scalers, deg, t))
    net = _Net(lambda i, o, t: PNAConv(i, o, aggrs, scalers, deg, towers=t)).to(dev)
    net.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    o_ref, o_net = torch.optim.SGD(ref.parameters(), lr=0.02), torch.optim.SGD(net.parameters(), lr=0.02)
    xd, eid, td = x.to(dev), ei.to(dev), target.to(dev)
    cat = lambda m: torch.cat([p.detach().reshape(-1).double().cpu() for _, p in sorted(m.named_parameters())])
    for step in range(5):
        o_ref.zero_grad()
        l_ref = ((ref(x.double(), ei) - target.double()) ** 2).mean()
        l_ref.backward()
        o_ref.step()
        o_net.zero_grad()
        l_net = ((net(xd, eid) - td) ** 2).mean()
        l_net.backward()
        o_net.step()
        l_net, l_ref = l_net.item(), l_ref.item()
        el, ep = abs(l_net - l_ref) / l_ref, relerr(cat(net), cat(ref))
        print("step %d: loss %.6f rel %.2e, parameters rel-L2 %.2e (tolerance %.0e)" % (step, l_ref, el, ep, OP_TOL))
        assert el <= OP_TOL and ep <= OP_TOL, (step, el, ep)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_bad_arguments_are_refused(dev, graphs):
    from dual_dmp_amd import ops
    ei, n = graphs["grid"]
    g = ops.graph_for(ei.to(dev), n, norm="gat", add_self_loops=False)
    plain = ops.graph_for(ei.to(dev), n)                         # not a valued graph
    loops = ops.graph_for(ei.to(dev), n, norm="gat")             # loop handling: a_e no longer counts input edges
    x = torch.randn(n, 8, device=dev)
    for bad in (plain, loops):
        with pytest.raises(ops.DdmpError):
            ops.gather_moments(bad, x)
    for kw in (dict(want=()), dict(want=("mean", "sum")), dict(want=("std", "var")), dict(want=("add",)), dict(tower_width=3),
               dict(tower_width=0), dict(root=torch.randn(n, 4, device=dev)), dict(want=("mean", "std"), out=torch.empty(n, 12, device=dev))):
        with pytest.raises(ops.DdmpError):
            ops.gather_moments(g, x, **kw)
    with pytest.raises(ops.DdmpError):
        ops.gather_moments(g, x.cpu())
    with pytest.raises(ops.DdmpError):
        ops.gather_stats(g, x, want=("std",))                    # the statistics keep refusing the second moment
    (_, _), (amx, _), invdeg, mu = ops.gather_moments(g, x, want=("max", "std"))
    for kw in (dict(), dict(dmx=x), dict(dmx=x, argmx=amx.long()), dict(dmx=x, argmx=amx, invdeg=invdeg), dict(ds=x, dq=x),
               dict(dmx=x, argmx=amx, dq=x, b=x), dict(ds=x, out=torch.empty(n, 4, device=dev))):
        with pytest.raises(ops.DdmpError):
            ops.gather_moments_bwd(g, **kw)
    # the C ABI: every refusal is the error status, without a launch
    L = ops._lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ops._stream()
    y, v, m = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)

    def fwd(gh, B=p(x), C=8, ldb=8, mean=0, as_std=0, tw=8, tstride=8, S=p(y), lds=8, Mx=None, argmx=None, V=None, mu=None):
        return L.ddmp_gather_moments_f32(gh, B, ldb, C, mean, as_std, None, 0, tw, tstride, S, lds, Mx, 8, argmx, 8, None, 0, None, 0,
                                         V, 8, mu, 8, None, st)

    assert fwd(g.handle) == 0 and fwd(g.handle, V=p(v), mu=p(m), as_std=1) == 0
    assert fwd(None) != 0 and fwd(plain.handle) != 0 and fwd(loops.handle) != 0
    assert fwd(g.handle, B=None) != 0                            # a null B
    assert fwd(g.handle, S=None) != 0                            # nothing requested
    assert fwd(g.handle, S=p(x)) != 0 and fwd(g.handle, Mx=p(y)) != 0 and fwd(g.handle, V=p(y), mu=p(m)) != 0   # aliasing outputs
    assert fwd(g.handle, V=p(v), mu=p(v)) != 0
    assert fwd(g.handle, tw=3) != 0 and fwd(g.handle, tw=0) != 0 and fwd(g.handle, tw=16) != 0                 # tw must divide C
    assert fwd(g.handle, tw=4, tstride=2) != 0 and fwd(g.handle, tw=4, tstride=8, lds=8) != 0                  # towers past the row
    assert fwd(g.handle, tw=4, tstride=4) == 0
    assert fwd(g.handle, V=p(v)) != 0 and fwd(g.handle, mu=p(m)) != 0                                          # V without mu, mu without V
    assert fwd(g.handle, S=None, mean=1, Mx=p(v)) != 0 and fwd(g.handle, as_std=1) != 0 and fwd(g.handle, argmx=p(amx)) != 0
    assert fwd(g.handle, C=0) != 0 and fwd(g.handle, ldb=4) != 0 and fwd(g.handle, lds=4) != 0

    def bwd(gh, C=8, dS=p(x), dQ=None, B=None, dMx=None, argmx=None, dB=p(y), lddb=8):
        return L.ddmp_gather_moments_bwd_f32(gh, C, dS, 8, dQ, 8, B, 8, None, dMx, 8, argmx, 8, None, 0, None, 0, dB, lddb, st)

    assert bwd(g.handle) == 0 and bwd(g.handle, dQ=p(v), B=p(x)) == 0
    assert bwd(None) != 0 and bwd(plain.handle) != 0 and bwd(loops.handle) != 0
    assert bwd(g.handle, dS=None) != 0 and bwd(g.handle, dMx=p(v)) != 0 and bwd(g.handle, C=0) != 0 and bwd(g.handle, lddb=4) != 0
    assert bwd(g.handle, dQ=p(v)) != 0 and bwd(g.handle, B=p(x)) != 0
    assert bwd(g.handle, dS=None, dQ=p(v), B=p(x), dMx=p(v), argmx=p(amx)) != 0                                  # dQ without dS
    assert bwd(g.handle, dB=p(x)) != 0 and bwd(g.handle, dQ=p(v), B=p(y)) != 0                                   # dB aliases an operand
    torch.cuda.synchronize()

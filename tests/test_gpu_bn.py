"""The BatchNorm + LeakyReLU kernels (csrc/bn.hip, csrc/finalize.h) and every route that restates their arithmetic, at the
column families, shapes, bounds and references of tests/bn_cases.py (the float64 reference has CONSISTENT statistics: every
coefficient a route is given comes from the chain on the same y).

A  the stand-alone chain against the reference: every width, n = 1 .. 3, every workgroup count of the second stage, past one
   grid pass of bn_lrelu_apply, with the analytic identities of the bias gradient
B  operands as column blocks of wider buffers and n_rows below the tensors' rows: bitwise the contiguous result, nothing
   written outside; the refusals
C  running statistics over three calls, sums added over row halves (n_total != n_rows), the coefficient rows as exact
   functions of each other, tail-fused coefficients at the families, the variance clamp
D  the bfloat16 passes
E  the fused routes (GEMM / SpMM operand loads and epilogues) on consistent coefficients

Every test prints its figures (`pytest -s`): worst error per quantity in units of eps32 x the column's scale."""
import os
from fractions import Fraction

import pytest
import torch

import bn_cases as bc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DEFAULT_CONFIG = not any(k.startswith("DDMP_") and k != "DDMP_LIB" for k in os.environ)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def graphs(dev):
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    for name, (v, f) in {"ico3": synth.icosphere(3), "grid": synth.open_grid(9, 7)}.items():
        v, f = synth.permute_vertices(v, f, 1)
        m = Mesh(vs=v, faces=f)
        out[name + "_f"] = (torch.from_numpy(m.f_edges), len(f))
    return out


def dense_ahat(ei, n):
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((ei[1], ei[0]), torch.ones(ei.shape[1], dtype=torch.float64), accumulate=True)
    A += torch.eye(n, dtype=torch.float64)
    d = A.sum(1).pow(-0.5)
    return d[:, None] * A * d[None, :]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def supported(answer, what):
    """A `*_supported` predicate answering no: a failure in the default configuration, a skip under a switch."""
    if not answer:
        assert not DEFAULT_CONFIG, "%s refused in the default configuration" % what
        pytest.skip("%s switched off in this configuration" % what)


_SETUPS = {}


def setup(case, dev, calls=1):
    """case -> (Data, operands on the device, float64 reference on the device, scales, the chain's results).  Kept for the
    small cases that several tests share; nothing in it is written afterwards."""
    key = (case.id, case.families, calls)
    if key in _SETUPS:
        return _SETUPS[key]
    from dual_dmp_amd import ops
    d = case.make()
    ref = bc.reference(d, device=dev, calls=calls)
    sc = bc.scales(d, ref)
    dt = BF if case.bf16 else torch.float32
    T = dict(y=d.y.to(dev).to(dt), dz=d.dz.to(dev).to(dt), gamma=d.gamma.to(dev), beta=d.beta.to(dev))
    run = [t.to(dev) for t in d.running_start()]
    got = bc.run_chain(ops, T["y"], T["dz"], T["gamma"], T["beta"], (run[0], run[1]), calls=calls)
    out = (d, T, ref, sc, got)
    if not bc.is_large(case):
        _SETUPS[key] = out
    return out


def hold(case, d, got, ref, sc, calls=1, rel=0.0):
    rat = bc.ratios(got, d, ref, sc, rel=rel)
    print("BNFIG", case.id, "ambiguous %.1e" % sc["amb_share"], {q: round(v, 3) for q, v in bc.worst(rat).items()})
    bad = bc.misses(rat, d.families(), calls=calls)
    assert not bad, bad[:8]
    assert sc["amb_share"] <= bc.AMB_SHARE
    return rat


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("case", bc.CHAIN_CASES, ids=[c.id for c in bc.CHAIN_CASES])
def test_chain_against_the_float64_reference(dev, case):
    from dual_dmp_amd import ops, _lib
    n, C = case.n, case.C
    nblk = bc.NBLK_AT_1024.get(n) if C == 1024 else (1024 if (n, C) == (65541, 512) else None)
    if nblk is not None:                                           # the second stage sees the workgroup count the case is there for
        assert _lib.lib().ddmp_colreduce_workspace_bytes(n, C) == (nblk * 2 * C + 2 * C) * 8
    d, T, ref, sc, got = setup(case, dev)
    hold(case, d, got, ref, sc)
    y64, dz64 = T["y"].double(), T["dz"].double()
    assert bc.sum_misses(got["sums"][:C], y64) <= 1e-12 and bc.sum_misses(got["sums"][C:], y64 * y64) <= 1e-12
    assert bc.sum_misses(ops.colsum(T["dz"]), dz64) <= 1e-12
    if case.kind == "correlated":
        # the bias gradient: column sums of the STORED dY, which are analytically zero
        assert bc.sum_misses(got["dbias"], got["dy"]) <= 1e-12
        lim = bc.KD * bc.EPS32 * n * sc["sd"] + n * sc["amb_dy"]
        assert bool((got["dbias"].abs() <= lim).all()), float((got["dbias"].abs() / lim.clamp_min(1e-300)).max())
        dy1 = torch.empty_like(got["dy"])
        ops.bn_bwd_apply(T["dz"], T["y"], got["bn4"], got["c10"], dy1, None)
        assert torch.equal(bits(dy1), bits(got["dy"]))


# ---------------------------------------------------------------------------------------------------------------- B
SENT = -7.25


def _blocked(t, ld, rows, off=4):
    """A [rows, ld] buffer of sentinels whose column block [off, off + C) holds t in its first t.shape[0] rows -> (buffer, block)."""
    buf = torch.full((rows, ld), SENT, dtype=t.dtype, device=t.device)
    blk = buf[:, off:off + t.shape[1]]
    blk[:t.shape[0]].copy_(t)
    return buf, blk


def _untouched(buf, n, C, off=4):
    """Everything outside rows [0, n) x columns [off, off + C) is still the sentinel, bit for bit."""
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:n, off:off + C] = False
    return bool((bits(buf)[mask] == bits(torch.full((1,), SENT, dtype=buf.dtype, device=buf.device))[0]).all())


@pytest.mark.parametrize("wide", ["C+4", "2C", "mixed"])
@pytest.mark.parametrize("C", [32, 256])
def test_column_blocks_of_wider_buffers_are_bitwise_the_contiguous_run(dev, C, wide):
    from dual_dmp_amd import ops
    case = bc.Case(257, C, "correlated")
    d, T, ref, sc, got = setup(case, dev)
    n, extra = case.n, 3
    # mixed: every operand with a leading dimension of its own (y the narrowest, dz the widest)
    ldy, lddz, ldo = {"C+4": (C + 4,) * 3, "2C": (2 * C,) * 3, "mixed": (C + 4, 2 * C, C + 8)}[wide]
    off = 4
    ybuf, y = _blocked(T["y"], ldy, n + extra, off)
    dzbuf, dz = _blocked(T["dz"], lddz, n + extra, off)
    zbuf, z = _blocked(torch.full((n, C), SENT, device=dev), ldo, n + extra, off)
    dybuf, dy = _blocked(torch.full((n, C), SENT, device=dev), ldo, n + extra, off)
    y0, dz0 = ybuf.clone(), dzbuf.clone()
    bn4, c10 = got["bn4"], got["c10"]
    assert torch.equal(ops.bn_stats(y, n_rows=n), got["sums"])
    assert torch.equal(ops.colsum(dz, n_rows=n), ops.colsum(T["dz"]))
    ops.bn_lrelu_apply(y[:n], bn4[0], bn4[1], out=z[:n])
    assert torch.equal(bits(z[:n]), bits(got["z"])) and _untouched(zbuf, n, C, off)
    assert torch.equal(ops.bn_bwd_reduce(dz, y, bn4, n_rows=n), got["sums2"])
    dbs = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    ops.bn_bwd_apply(dz, y, bn4, c10, dy, dbs, n_rows=n)
    assert torch.equal(bits(dy[:n]), bits(got["dy"])) and _untouched(dybuf, n, C, off)
    assert torch.equal(dbs[:C], got["dbias"])
    dybuf.fill_(SENT)
    ops.bn_bwd_apply(dz, y, bn4, c10, dy, None, n_rows=n)
    assert torch.equal(bits(dy[:n]), bits(got["dy"])) and _untouched(dybuf, n, C, off)
    assert torch.equal(bits(ybuf), bits(y0)) and torch.equal(bits(dzbuf), bits(dz0))


def test_refusals_return_the_argument_error_and_write_nothing(dev):
    """ld % 4 != 0, ld < C, C = 24, C = 2048: DDMP_EINVAL (-1) from every entry point that reads or writes an [n, C] block, and
    no output touched.  (bn_lrelu_apply is elementwise and takes any C % 4 == 0: only the two ld refusals apply to it.)"""
    from dual_dmp_amd import ops, _lib
    L = _lib.lib()
    n, C = 64, 32
    p, st = ops._p, ops._stream()
    big = torch.full((n, 2048 + 8), 0.5, device=dev)
    bn4, c10 = torch.full((4, 2048), 0.5, device=dev), torch.full((2, 2048), 0.5, device=dev)
    ws = torch.zeros(8 << 20, dtype=torch.uint8, device=dev)       # ample for any width: the refusal is not about the workspace
    for ld, width in ((C + 2, C), (C - 4, C), (24, 24), (2048, 2048)):
        out = torch.full((n, 2048 + 8), SENT, device=dev)
        sums = torch.full((2 * 2048,), SENT, dtype=torch.float64, device=dev)
        a = (p(bn4[0]), p(bn4[1]), p(bn4[2]), p(bn4[3]))
        calls = {
            "bn_stats": L.ddmp_bn_stats_f32(p(big), ld, n, width, p(sums), p(ws), ws.numel(), st),
            "colsum": L.ddmp_colsum_f32(p(big), ld, n, width, p(sums), p(ws), ws.numel(), st),
            "bn_bwd_reduce": L.ddmp_bn_bwd_reduce(p(big), ld, p(big), ld, n, width, 0, *a, 0.01, p(sums), p(ws), ws.numel(), st),
            "bn_bwd_apply": L.ddmp_bn_bwd_apply(p(big), ld, p(big), ld, p(out), ld, n, width, 0, a[0], a[1], p(c10[0]), p(c10[1]),
                                                0.01, p(sums), p(ws), ws.numel(), st),
        }
        if width == C:
            calls["bn_lrelu_apply"] = L.ddmp_bn_lrelu_apply_f32(p(big), ld, p(out), ld, n, width, a[0], a[1], 0.01, st)
        torch.cuda.synchronize()
        assert all(v == -1 for v in calls.values()), (ld, width, calls)
        assert bool((out == SENT).all()) and bool((sums == SENT).all()), (ld, width)
    assert L.ddmp_colreduce_workspace_bytes(n, 24) == 0 and L.ddmp_colreduce_workspace_bytes(n, 2048) == 0
    with pytest.raises(ops.DdmpError):
        ops.bn_stats(big[:, :24])


# ---------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("case", [bc.Case(257, 32, "correlated"), bc.Case(2, 8, "random", 1), bc.Case(1, 8, "random", families=bc.N1_FAMILIES),
                                  bc.Case(2000, 1024, "random")], ids=lambda c: c.id)
def test_running_statistics_over_three_calls(dev, case):
    d, T, ref, sc, got = setup(case, dev, calls=3)
    rat = hold(case, d, got, ref, sc, calls=3)
    assert "run_mean" in rat and "run_var" in rat


def _ulps(a, b):
    assert bool(torch.isfinite(a).all() and torch.isfinite(b).all())
    ia, ib = bits(a).long(), bits(b).long()
    ia, ib = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia), torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int((ia - ib).abs().max())


@pytest.mark.parametrize("case", [bc.Case(257, 32, "correlated"), bc.Case(2000, 1024, "correlated")], ids=lambda c: c.id)
def test_sums_added_over_row_halves_give_the_coefficients_of_the_whole(dev, case):
    """What the two-rank path relies on: n_total != n_rows.  float64 sums of two row ranges, added, prepared with
    n_total = n: the coefficients of the whole within 2 ulp of float32, forward and backward."""
    from dual_dmp_amd import ops
    d, T, ref, sc, got = setup(case, dev)
    n, C, h = case.n, case.C, case.n // 2 + 1
    y, dz = T["y"], T["dz"]
    s = ops.bn_stats(y[:h]).clone() + ops.bn_stats(y[h:])
    assert bc.sum_misses(s[:C], y.double()) <= 1e-12
    bn4 = torch.empty(4, C, device=dev)
    run = [t.to(dev) for t in d.running_start()]
    ops.bn_prepare(s, n, T["gamma"], T["beta"], bn4, running=(run[0], run[1]))
    # shift = beta - mean * scale is a difference: its ulp is not the yardstick where it cancels; 2 ulp of the larger operand
    for i in (0, 2, 3):
        assert _ulps(bn4[i], got["bn4"][i]) <= 2, i
    big = torch.maximum((got["bn4"][2] * got["bn4"][0]).abs(), T["beta"].abs())
    assert bool(((bn4[1] - got["bn4"][1]).abs() <= 2 * 2.0 ** -23 * big).all())
    assert _ulps(run[0], got["run_mean"]) <= 2 and _ulps(run[1], got["run_var"]) <= 2
    # backward, on the coefficients of the whole
    s2 = ops.bn_bwd_reduce(dz[:h], y[:h], got["bn4"]).clone() + ops.bn_bwd_reduce(dz[h:], y[h:], got["bn4"])
    dgamma, dbeta, c10 = torch.empty(C, device=dev), torch.empty(C, device=dev), torch.empty(2, C, device=dev)
    ops.bn_bwd_prepare(s2, n, got["bn4"], dgamma, dbeta, c10)
    # the two sums are sums of signed terms: 2 ulp of the result, or 1e-12 of the sum of magnitudes where they cancel
    tol_b = torch.maximum(2 * 2.0 ** -23 * got["dbeta"].abs(), (1e-12 * sc["sb"]).float())
    tol_g = torch.maximum(2 * 2.0 ** -23 * got["dgamma"].abs(), (1e-12 * sc["sg"]).float())
    assert bool(((dbeta - got["dbeta"]).abs() <= tol_b).all()) and bool(((dgamma - got["dgamma"]).abs() <= tol_g).all())
    a, r, mu = (got["bn4"][i].double().abs() for i in (0, 3, 2))
    assert bool(((c10[0] - got["c10"][0]).abs() <= 2 * 2.0 ** -23 * got["c10"][0].abs() + a * r * tol_g / n).all())
    tol_0 = 2 * 2.0 ** -23 * torch.maximum((a * got["dbeta"].double() / n).abs(), (got["c10"][0].double() * mu).abs())
    assert bool(((c10[1] - got["c10"][1]).abs() <= tol_0 + a * tol_b / n + a * r * tol_g / n * mu.abs()).all())


def _round_to_f32(x):
    """The float32 nearest to the exact rational x (ties to even), as a Fraction."""
    import numpy as np
    c = np.float32(float(x))
    cands = sorted({Fraction(float(v)) for v in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf)))},
                   key=lambda v: (abs(v - x), int(np.float32(float(v)).view(np.uint32)) & 1))
    return cands[0]


@pytest.mark.parametrize("case", [bc.Case(257, 32, "correlated"), bc.Case(2000, 1024, "random")], ids=lambda c: c.id)
def test_coefficient_rows_are_the_stated_arithmetic(dev, case):
    """What every prologue and every fused backward assumes of the rows it is handed: scale = gamma * rstd (one float32
    product) and shift = fma(-mean, scale, beta) of the STORED float32 mean and scale rows, exactly -- so that
    fma(y, scale, shift) = scale * (y - mean) + beta up to one rounding, with the mean the backward's yhat subtracts."""
    d, T, ref, sc, got = setup(case, dev)
    bn4 = got["bn4"].cpu()
    assert torch.equal(bits(bn4[0]), bits(d.gamma * bn4[3]))
    mean, scale, beta, shift = (t.tolist() for t in (bn4[2], bn4[0], d.beta, bn4[1]))
    for c in range(case.C):
        want = _round_to_f32(-Fraction(mean[c]) * Fraction(scale[c]) + Fraction(beta[c]))
        assert Fraction(shift[c]) == want, (c, case.family(c), shift[c], float(want))


@pytest.mark.parametrize("case", [bc.Case(257, 32, "correlated"), bc.Case(2000, 1024, "correlated"), bc.Case(3, 8, "random", 1),
                                  bc.Case(257, 128, "correlated", families=bc.BF16_FAMILIES, bf16=True)], ids=lambda c: c.id)
def test_tail_fused_coefficients_at_the_families(dev, case):
    """BnFwd on bn_stats, BnBwd on bn_bwd_reduce: bitwise what the stand-alone prepare kernels write, at every family."""
    from dual_dmp_amd import ops
    d, T, ref, sc, got = setup(case, dev)
    n, C = case.n, case.C
    bn4 = torch.zeros(4, C, device=dev)
    run = [t.to(dev) for t in d.running_start()]
    sums = ops.bn_stats(T["y"], bn=ops.BnFwd(n, T["gamma"], T["beta"], bn4, running=(run[0], run[1])))
    assert torch.equal(sums, got["sums"]) and torch.equal(bits(bn4), bits(got["bn4"]))
    assert torch.equal(bits(run[0]), bits(got["run_mean"])) and torch.equal(bits(run[1]), bits(got["run_var"]))
    dgamma, dbeta, c10 = torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(2, C, device=dev)
    s2 = ops.bn_bwd_reduce(T["dz"], T["y"], bn4, bn=ops.BnBwd(n, bn4, dgamma, dbeta, c10))
    assert torch.equal(s2, got["sums2"]) and torch.equal(bits(c10), bits(got["c10"]))
    assert torch.equal(bits(dgamma), bits(got["dgamma"])) and torch.equal(bits(dbeta), bits(got["dbeta"]))
    assert ops.next_pending() == 0


def test_a_negative_variance_residue_is_clamped(dev):
    """s1/n - (s0/n)^2 from float64 sums is a rounding residue of either sign on a constant column; sums made by hand with a
    negative one (a constant 3 over 4 rows, the sum of squares one short): variance 0, rstd = 1/sqrt(eps), finite everywhere."""
    from dual_dmp_amd import ops
    C, n = 8, 4
    sums = torch.cat([torch.full((C,), 3.0 * n), torch.full((C,), 9.0 * n - 1.0)]).double().to(dev)
    gamma, beta = torch.full((C,), 0.75, device=dev), torch.full((C,), 0.5, device=dev)
    bn4 = torch.zeros(4, C, device=dev)
    run = [torch.full((C,), 0.25, device=dev), torch.full((C,), 2.0, device=dev)]
    ops.bn_prepare(sums, n, gamma, beta, bn4, running=(run[0], run[1]))
    rs = 1.0 / (float(torch.tensor(bc.BN_EPS, dtype=torch.float32)) ** 0.5)
    assert bool(torch.isfinite(bn4).all()) and bool(torch.isfinite(run[1]).all())
    assert bool(((bn4[3].double() - rs).abs() <= bc.EPS32 * rs).all()) and bool((bn4[2] == 3.0).all())
    assert bool(((run[1].double() - 0.9 * 2.0).abs() <= bc.KR * bc.EPS32 * 1.8).all())


# ---------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("case", bc.BF16_CASES, ids=[c.id for c in bc.BF16_CASES])
def test_bf16_passes_against_the_float64_reference(dev, case):
    """z and dY are rounded once on the store: half a bfloat16 ulp of the reference (2^-8 relative, as close_bf16 of
    tests/test_gpu_bf16.py has it) on top of the float32 bound; the sums and the float32 coefficients as in float32."""
    from dual_dmp_amd import ops
    d, T, ref, sc, got = setup(case, dev)
    C = case.C
    assert got["z"].dtype == BF and got["dy"].dtype == BF
    hold(case, d, got, ref, sc, rel=2.0 ** -8)
    y64 = T["y"].double()
    assert bc.sum_misses(got["sums"][:C], y64) <= 1e-12 and bc.sum_misses(got["sums"][C:], y64 * y64) <= 1e-12
    assert bc.sum_misses(got["dbias"], got["dy"]) <= 1e-12
    dy1 = torch.empty_like(got["dy"])
    ops.bn_bwd_apply(T["dz"], T["y"], got["bn4"], got["c10"], dy1, None)
    assert torch.equal(bits(dy1), bits(got["dy"]))


# ---------------------------------------------------------------------------------------------------------------- E
# Elementwise yardsticks of the fused routes, in eps32 units of the absolute product (what the bf16 GEMM tests use as their
# atol yardstick: sum_k |operand_ik| |W_kj| with the dY operand weighted by its scale Sd_c).  Each constant is the rel-L2
# tolerance the route's existing test in tests/test_gpu_kernels.py asserts, divided by eps32 -- the same budget, asked of
# every element against the absolute product instead of once of the whole matrix against its norm:
K_GEMM = 3e-6 / bc.EPS32       # 50.3: test_gemm_bnbwd_fused_matches_composition, test_first_layer_wgrad_... (f16x3 planes: ~1e-6)
K_SPMM = 1e-6 / bc.EPS32       # 16.8: test_spmm_with_bn_backward_on_the_gather (float32 gather of <= 4 entries per row)
K_RED = 1e-5 / bc.EPS32        # 168: test_spmm_with_bn_backward_reduce / test_gemm_nn_with_bn_backward_reductions against float64
                               # (the epilogues sum 16 .. 64 rows in float32 before float64 takes over)
K_STAT = 2e-6 / bc.EPS32       # 33.6: test_spmm_with_forward_statistics (float32 around `ref` over 16 rows)


def _moved_by_flips(d, ref, sc):
    """[n, C]: what the ambiguous elements may move an element of dY by (its own flip + the column's coefficients)."""
    dz = d.dz.to(ref["z"].device).double()
    return (1.0 - bc.SLOPE) * (sc["amb"] * (ref["scale"] * dz).abs()) + sc["amb_dy"][None, :]


def _within(name, got, want, bound, extra=None):
    err = (got.double() - want).abs()
    if extra is not None:
        err = (err - extra).clamp_min(0)
    r = bc._ratio(err, bound)
    print("BNFIG", name, "worst / bound %.3f" % float(r.max()))
    assert bool((r <= 1.0).all()), (name, float(r.max()))


def _lrelu64(x, a, b):
    v = x.double() * a.double() + b.double()
    return torch.where(v > 0, v, bc.SLOPE * v)


def _gemm_operands(case, cin, dev):
    gen = torch.Generator().manual_seed(case.n + cin)
    w = (torch.randn(case.C, cin, generator=gen) / case.C ** 0.5).to(dev)
    p = torch.randn(case.n, cin, generator=gen).to(dev)
    psc, psh = (torch.rand(cin, generator=gen) + 0.5).to(dev), torch.randn(cin, generator=gen).to(dev)
    return w, p, (psc, psh)


@pytest.mark.parametrize("n,cin,cout", [(65537, 256, 512), (66001, 32, 64)])
def test_dgrad_rebuilds_dy_from_consistent_coefficients(dev, n, cin, cout):
    """gemm_nn_bnbwd: dY is rebuilt on the operand load from the chain's own coefficients of the same y, and the product is
    held against the reference dY pushed through the float64 product."""
    from dual_dmp_amd import ops
    supported(ops.gemm_bnbwd_supported(cout, cin, n), "gemm_nn_bnbwd")
    case = bc.Case(n, cout, "correlated")
    d, T, ref, sc, got = setup(case, dev)
    w = _gemm_operands(case, cin, dev)[0]
    dx = ops.gemm_nn_bnbwd(T["dz"], T["y"], w, got["bn4"], got["c10"])
    wa = w.double().abs()
    _within("dgrad %s" % case.id, dx, ref["dy"] @ w.double(), K_GEMM * bc.EPS32 * (sc["sd"][None, :] @ wa), _moved_by_flips(d, ref, sc) @ wa)


@pytest.mark.parametrize("n,cin,cout", [(65537, 256, 512), (66001, 32, 64), (70001, 16, 32)])
def test_wgrad_rebuilds_dy_from_consistent_coefficients(dev, n, cin, cout):
    """gemm_tn_bnbwd with and without pro= (at 16 -> 32: the first layer's wgrad): row c of dW against
    K_GEMM eps32 Sd_c sum_r |f(Z)_rj|, per family.

    This test found a defect, fixed together with it.  At (65537, 256 -> 512) the wide f16x3 wgrad split the
    rebuilt dY into two f16 planes scaled by ONE power of two taken from its global maximum: fixed point with a floor of 2^-40 of
    that maximum, and the rows of dW of the `big` columns (dY at 2^-41 of the loudest column's) came out exactly 0 -- 657 x the
    bound without and 1490 x with the prologue, every other family below 0.015.  The kernel now lifts every column whose scale a
    is more than 12 binades below the largest a to that binade (a power of two folded into a, b, c1, c0 where they are staged,
    undone per row of dW: f16s_colnorm, csrc/gemm_f16s.inc) and leaves the others bit for bit as they were; on an MI355X `big`
    reads 0.0002 / 0.0025 of the bound, like its neighbours."""
    from dual_dmp_amd import ops
    supported(ops.gemm_tn_bnbwd_supported(cout, cin, n), "gemm_tn_bnbwd")
    case = bc.Case(n, cout, "correlated")
    d, T, ref, sc, got = setup(case, dev)
    w, p, pro_rows = _gemm_operands(case, cin, dev)
    flips, sd, fams = _moved_by_flips(d, ref, sc), sc["sd"], d.families()
    worst = {}
    for pro in (None, pro_rows):
        f = p.double() if pro is None else _lrelu64(p, *pro)
        dw = ops.gemm_tn_bnbwd(T["dz"], T["y"], p, got["bn4"], got["c10"], pro=pro)
        err = ((dw.double() - ref["dy"].t() @ f).abs() - flips.t() @ f.abs()).clamp_min(0)
        r = bc._ratio(err, K_GEMM * bc.EPS32 * sd[:, None] * f.abs().sum(0)[None, :]).amax(1).cpu()
        per = {fam: float(r[[c for c, x in enumerate(fams) if x == fam]].max()) for fam in dict.fromkeys(fams)}
        print("BNFIG wgrad %s pro=%s worst / bound per family" % (case.id, pro is not None), {k: "%.3g" % v for k, v in per.items()})
        worst[pro is not None] = per
    bad = [(pro, fam, v) for pro, per in worst.items() for fam, v in per.items() if not v <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("gname", ["grid_f", "ico3_f"])
def test_gathers_rebuild_or_reduce_from_consistent_coefficients(dev, graphs, gname, C):
    """spmm_bnbwd (A_hat . dY, dY rebuilt on the gather) and spmm_bnred (A_hat . x with the BatchNorm-backward reductions of
    its output from the epilogue) on a family y and the chain's coefficients of that y."""
    from dual_dmp_amd import ops
    ei, n = graphs[gname]
    case = bc.Case(n, C, "correlated")
    d, T, ref, sc, got = setup(case, dev)
    g = ops.graph_for(ei.to(dev), n)
    A = dense_ahat(ei, n).to(dev)
    supported(ops.spmm_bnbwd_supported(C), "spmm_bnbwd")
    out = torch.empty(n, C, device=dev)
    ops.spmm_bnbwd(g, T["dz"], T["y"], got["bn4"], got["c10"], out)
    _within("spmm_bnbwd %s %s" % (gname, case.id), out, A @ ref["dy"], K_SPMM * bc.EPS32 * A.sum(1)[:, None] * sc["sd"][None, :],
            A @ _moved_by_flips(d, ref, sc))
    # the reductions: the gradient is A_hat . x, x = the case's dz
    out = torch.empty(n, C, device=dev)
    sums = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    ops.spmm_bnred(g, T["dz"], out, T["y"], got["bn4"], sums)
    assert torch.equal(bits(out), bits(ops.spmm(g, T["dz"])))
    _reductions_hold("spmm_bnred %s %s" % (gname, case.id), sums, A @ T["dz"].double(), A @ T["dz"].double().abs(), ref, sc, C)


def _reductions_hold(name, sums, G, Gabs, ref, sc, C):
    """sums = (sum g, sum g yhat), g = G lrelu'(pre), against float64; Gabs: the absolute product behind G."""
    lg = torch.where(ref["pre"] > 0, 1.0, bc.SLOPE)
    g, ga = G * lg, Gabs * lg
    flip = (1.0 - bc.SLOPE) * (sc["amb"] * Gabs)
    sb = ga.sum(0)
    sg = (ga * ref["yhat"].abs()).sum(0) + ref["mean"].abs() * ref["rstd"] * sb
    _within(name + " sum g", sums[:C], g.sum(0), K_RED * bc.EPS32 * sb, flip.sum(0))
    _within(name + " sum g yhat", sums[C:], (g * ref["yhat"]).sum(0), K_RED * bc.EPS32 * sg, (flip * ref["yhat"].abs()).sum(0))


def test_dgrad_epilogue_reduces_on_consistent_coefficients(dev):
    """gemm_nn_bnred at (20300, 64 -> 256): out = dH . W and the BatchNorm-backward reductions of out against the family y of
    the layer below, from the epilogue."""
    from dual_dmp_amd import ops
    n, M, K = 20300, 64, 256
    supported(ops.gemm_nn_bnred_supported(M, K, n), "gemm_nn_bnred")
    case = bc.Case(n, K, "correlated")
    d, T, ref, sc, got = setup(case, dev)
    gen = torch.Generator().manual_seed(n + M + K)
    dh, w = (torch.randn(n, M, generator=gen) * 2.0 ** -7).to(dev), (torch.randn(M, K, generator=gen) / M ** 0.5).to(dev)
    sums = torch.zeros(2 * K, dtype=torch.float64, device=dev)
    out = ops.gemm_nn_bnred(dh, w, T["y"], got["bn4"], sums)
    assert torch.equal(bits(out), bits(ops.gemm_nn(dh, w)))
    G, Gabs = dh.double() @ w.double(), dh.double().abs() @ w.double().abs()
    _within("gemm_nn_bnred out", out, G, K_GEMM * bc.EPS32 * Gabs)
    _reductions_hold("gemm_nn_bnred %s" % case.id, sums, G, Gabs, ref, sc, K)


def _variance_holds(name, sums, stored, n, fams, tol, skip=("const", "tiny")):
    C = stored.shape[1]
    s = stored.double()
    var_ref = s.var(0, unbiased=False)
    var = sums[C:] / n - (sums[:C] / n) ** 2
    keep = torch.tensor([f not in skip for f in fams], device=s.device)
    r = bc._ratio((var - var_ref).abs(), var_ref)
    print("BNFIG", name, "variance rel", {f: "%.1e" % float(r[[i for i, x in enumerate(fams) if x == f]].max()) for f in dict.fromkeys(fams)})
    assert bool((r[keep] <= tol).all()), (name, [(fams[i], float(r[i])) for i in torch.nonzero(keep & ~(r <= tol)).flatten().tolist()])


@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("gname", ["grid_f", "ico3_f"])
def test_gather_statistics_of_a_family_output(dev, graphs, gname, C):
    """spmm_stats whose OUTPUT is a family matrix: x carries the families' spreads, bias their offsets.  The output is the plain
    gather's bit for bit, the sums are those of the stored output to the float32-over-16-rows budget, and with ref = 1.01 mean
    the variance keeps 2e-5 relative (what test_spmm_with_forward_statistics states) on every family but const and tiny.

    offset1k sits at that bound's edge by arithmetic: its reference is 0.01 x 1024 / 0.6 = 17 sigma from the mean, so the
    variance is a difference with condition 290, and float32 sums over 16 rows leave 290 x eps32 x O(1) = 1.7e-5 x O(1).
    Default configuration on an MI355X: 4.1e-6 .. 1.3e-5 (every other family <= 8e-8).  With DDMP_SPMM_PATCH=1, which puts the
    96-row grid on the LDS-patch kernel, [grid_f-256] reads 2.14e-5 and this test fails there; the bound stays."""
    from dual_dmp_amd import ops
    supported(ops.spmm_stats_supported(C), "spmm_stats")
    ei, n = graphs[gname]
    case = bc.Case(n, C, "correlated")
    d = case.make()
    fams = d.families()
    off = torch.tensor([bc.FAMILY_AFFINE[f][0] for f in fams])
    x, bias = (d.y - off).to(dev), off.to(dev)
    g = ops.graph_for(ei.to(dev), n)
    plain = ops.spmm(g, x, bias=bias)
    s64 = plain.double()
    mean = (s64.sum(0) / n).float()
    for ref_row, tol in ((torch.zeros(C, device=dev), None), ((mean * 1.01).contiguous(), 2e-5)):
        out = torch.empty_like(plain)
        sums = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        ops.spmm_stats(g, x, out, ref_row, sums, bias=bias)
        assert torch.equal(bits(out), bits(plain))
        name = "spmm_stats %s %s ref=%s" % (gname, case.id, "0" if tol is None else "1.01mean")
        _within(name + " sum", sums[:C], s64.sum(0), K_STAT * bc.EPS32 * s64.abs().sum(0))
        _within(name + " sumsq", sums[C:], (s64 * s64).sum(0), K_STAT * bc.EPS32 * (s64 * s64).sum(0))
        if tol is not None:
            _variance_holds(name, sums, plain, n, fams, tol)


def test_gemm_statistics_of_a_family_output(dev):
    """gemm_nt_stats at (20500, 32 -> 64) whose output columns are the families (rows of W carry the spreads, bias the offsets):
    the output against the float64 product elementwise, the sums against the stored output (float64 partials: 1e-12), the
    variance from them to 1e-6 (test_gemm_nt_stats_matches_bn_stats) on every family but const and tiny."""
    from dual_dmp_amd import ops
    n, K, M = 20500, 32, 64
    case = bc.Case(n, M, "correlated")
    fams = [case.family(c) for c in range(M)]
    gen = torch.Generator().manual_seed(n + M)
    a = torch.randn(n, K, generator=gen).to(dev)
    spread = torch.tensor([bc.FAMILY_AFFINE[f][1] for f in fams])
    w = (torch.randn(M, K, generator=gen) / K ** 0.5 * spread[:, None]).to(dev)
    bias = torch.tensor([bc.FAMILY_AFFINE[f][0] for f in fams]).to(dev)
    sums = torch.zeros(2 * M, dtype=torch.float64, device=dev)
    y = ops.gemm_nt_stats(a, w, sums, bias=bias)
    want = a.double() @ w.double().t() + bias.double()
    k = K_GEMM * (10.0 if ops.get_gemm_mode() == 3 else 1.0)        # bf16x3 planes: GEMM_TOL of tests/test_gpu_kernels.py, 3e-5
    _within("gemm_nt_stats out", y, want, k * bc.EPS32 * (a.double().abs() @ w.double().abs().t() + bias.double().abs()))
    y64 = y.double()
    assert bc.sum_misses(sums[:M], y64) <= 1e-12 and bc.sum_misses(sums[M:], y64 * y64) <= 1e-12
    _variance_holds("gemm_nt_stats", sums, y, n, fams, 1e-6)

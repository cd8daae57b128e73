"""The operand families of tests/extreme_operands.py hold what they promise, and the references stay usable on them -- checked
without a GPU, so that tests/test_gpu_extremes.py compares the kernels with numbers that mean something:

* the family's score-range condition, asserted on the reference's own z;
* the float64 edge-list reference against the dense reference of the same ``*_ref.py`` (forward, 1e-10);
* the reference is finite in float64 and in float32;
* the float32-vs-float64 yardstick is finite and below 1e-3 for every quantity the GPU test compares;
* the float64 restatement of clip + Adam against ``torch.optim.Adam`` on float64 parameters.

The dense GATv2 form holds an [N, N, heads, C] array: on the 1801-node hub graph that is 0.6 to 6.6 GB per temporary, so GATv2 is
compared with its dense form on the grid only (GAT and Transformer, [N, N, heads], on both graphs)."""
import math

import numpy as np
import pytest
import torch

import extreme_operands as X
from extreme_operands import graphs  # noqa: F401  (the fixture of test_gpu_gat.py)

relerr = X.relerr


def _dense(op, o, ei, n, heads, loops):
    from gat_ref import dense_gat
    from gatv2_ref import dense_gatv2
    from transformer_ref import dense_transformer
    d = lambda t: t.double()
    hc = o["dout"].shape[1]
    eye, zero = torch.eye(hc, dtype=torch.float64), torch.zeros(hc, hc, dtype=torch.float64)
    with torch.no_grad():
        if op == "gat":
            return dense_gat(d(o["hf"]), ei, eye, d(o["att_src"]), d(o["att_dst"]), d(o["bias"]), heads, True, 0.2, loops)
        if op == "gatv2":
            x = torch.cat([d(o["xl"]), d(o["xr"])], 1)
            return dense_gatv2(x, ei, torch.cat([eye, zero], 1), None, torch.cat([zero, eye], 1), None, d(o["att"]), d(o["bias"]),
                               heads, True, 0.2, loops)
        x = torch.cat([d(o[k]) for k in ("q", "k", "v", "skip")], 1)
        sel = lambda i: torch.cat([eye if j == i else zero for j in range(4)], 1)
        return dense_transformer(x, ei, sel(0), None, sel(1), None, sel(2), None, sel(3), None, None, heads, True)


@pytest.mark.parametrize("op,family,name,loops,C,heads", X.softmax_cases())
def test_softmax_families_hold_their_conditions(graphs, op, family, name, loops, C, heads):
    ei, n = graphs[name]
    o = X.softmax_operands(op, family, n, C, heads)
    for t in o.values():
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    z, dst, src = X.softmax_scores(op, o, ei, n, heads, loops)
    X.check_softmax_condition(family, z, dst, src, n)
    ref, rows = X.softmax_reference(op, o, ei, n, heads, loops, torch.float64)
    r32, _ = X.softmax_reference(op, o, ei, n, heads, loops, torch.float32)
    if not (op == "gatv2" and n > 1000):
        e = relerr(ref["y"], _dense(op, o, ei, n, heads, loops))
        assert e < 1e-10, e
    bad = []
    for k in ref:
        assert bool(torch.isfinite(ref[k]).all()) and bool(torch.isfinite(r32[k]).all()), k
        yard = X.measure(op, family, k, r32, ref)
        print("%s %s %s C=%d heads=%d %s: float32 CPU yardstick %.2e" % (op, family, name, C, heads, k, yard))
        if not (math.isfinite(yard) and yard < 1e-3):
            bad.append((k, yard))
    assert not bad, bad
    # alpha of the reference: rows sum to 1, one-hot / multiplicity shares where the family says so
    alpha = ref["alpha"]
    sums = torch.zeros((n, heads), dtype=torch.float64).index_add_(0, rows, alpha)
    live = torch.from_numpy(np.bincount(rows.numpy(), minlength=n) > 0)
    assert bool((~live).any()) == name.endswith("-iso")
    assert float((sums[live] - 1).abs().max()) < 1e-12
    if family == "dominant":                                     # exactly one-hot in float32; within e^-200 of it in float64
        a32 = r32["alpha"]
        assert bool(((a32 == 0) | (a32 == 1)).all()) and float((alpha - a32.double()).abs().max()) < 1e-80
        assert not r32["dz" if "dz" in r32 else "ds"].any()
    if family == "ties":
        mult = X.multiplicities(ei, n, loops)
        share = mult / torch.zeros(n, dtype=torch.float64).index_add_(0, rows, mult)[rows]
        assert float((alpha - share.unsqueeze(1)).abs().max()) < 1e-15


@pytest.mark.parametrize("family", X.HEAD_FAMILIES)
@pytest.mark.parametrize("n", [257, 131073])
def test_head_families_hold_their_conditions(family, n):
    o = X.head_operands(family, n, 1)
    r64, r32 = X.head_reference(o, 1, torch.float64), X.head_reference(o, 1, torch.float32)
    u = r64["u"]
    third = torch.arange(n) % 3 == 0
    if family == "saturated":
        assert float(u[third].abs().min()) >= 20.0
        v = torch.tanh(u[third].float())
        assert bool((v.abs() == 1).all()) and not r32["dz"][third].any() and not r64["dz"][third].any()
        assert float(u[~third].abs().max()) < 9.0                                     # 1 - tanh(9)^2 = 6e-8: not yet lost
    elif family == "zero":
        assert not u.any() and not X.head_reference(o, 1, torch.float32)["u"].any()
        assert not r64["out"].any()
        assert float(r64["dz"].abs().max()) > 1e9                                     # the 1 / 1e-12 factor decides
    else:
        assert float(u.abs().max()) < 20.0
    for k in X.HEAD_KEYS:
        assert bool(torch.isfinite(r64[k]).all()) and bool(torch.isfinite(r32[k]).all()), k
        yard = relerr(r32[k], r64[k])
        print("head %s n=%d %s: float32 CPU yardstick %.2e" % (family, n, k, yard))
        assert math.isfinite(yard) and yard < 1e-3, (k, yard)


@pytest.mark.parametrize("kind", X.OPT_SETS + ("below", "zero"))
@pytest.mark.parametrize("n", X.OPT_SIZES[:3])
def test_clip_adam_restatement_equals_torch_adam_in_float64(kind, n):
    f32 = lambda x: float(np.float32(x))
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    pt = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([pt], lr=f32(X.LR), betas=(f32(X.BETAS[0]), f32(X.BETAS[1])), eps=f32(X.ADAM_EPS))
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        g = X.optimizer_gradient(kind, n, step)
        assert g.dtype == torch.float32 and bool(torch.isfinite(g).all())
        if kind == "below":
            assert 0.2 < float(g.double().norm()) <= 0.4 < X.MAX_NORM
        pt.grad = g.double().clone()
        torch.nn.utils.clip_grad_norm_([pt], f32(X.MAX_NORM))
        opt.step()
        p, m, v, gc = X.clip_adam_f64(p, m, v, g, step)
        st = opt.state[pt]
        assert relerr(gc, pt.grad) < 1e-12
        for a, b in ((p, pt.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert bool(torch.isfinite(a).all()) and relerr(a, b) < 1e-12, (kind, n, step)


@pytest.mark.parametrize("family", X.FEAST_FAMILIES)
@pytest.mark.parametrize("name,loops", X.FEAST_GRAPHS)
@pytest.mark.parametrize("C,heads", X.FEAST_WIDTHS)
def test_feast_families_hold_their_conditions(graphs, family, name, loops, C, heads):
    from feast_ref import dense_feast
    ei, n = graphs[name]
    o = X.feast_operands(family, n, C, heads)
    ref, rows, aux = X.feast_reference(o, ei, n, heads, loops, torch.float64)
    r32, _, _ = X.feast_reference(o, ei, n, heads, loops, torch.float32)
    X.check_feast_condition(family, aux["z"].detach())
    hc = heads * C
    eye = torch.eye(hc + heads, dtype=torch.float64)
    with torch.no_grad():
        dense = dense_feast(torch.cat([o["hf"], o["p"]], 1).double(), ei, eye[:hc], eye[hc:], o["c"].double(), o["bias"].double(),
                            heads, loops)
    assert relerr(ref["y"], dense) < 1e-10
    bad = []
    for k in ref:
        assert bool(torch.isfinite(ref[k]).all()) and bool(torch.isfinite(r32[k]).all()), k
        yard = relerr(r32[k], ref[k])
        print("feast %s %s C=%d heads=%d %s: float32 CPU yardstick %.2e" % (family, name, C, heads, k, yard))
        if not (math.isfinite(yard) and yard < 1e-3):
            bad.append((k, yard))
    assert not bad, bad
    if family == "flat":
        assert bool((aux["q"] == 1.0 / heads).all())


@pytest.mark.parametrize("family", X.GMM_FAMILIES)
@pytest.mark.parametrize("C,K,dim", X.GMM_WIDTHS)
@pytest.mark.parametrize("root", [True, False])
def test_gmm_families_hold_their_conditions(graphs, family, C, K, dim, root):
    from gmm_ref import dense_gmm
    ei, n = graphs[X.GMM_GRAPH]
    o = X.gmm_operands(family, n, ei.shape[1], C, K, dim)
    ref, rows, aux = X.gmm_reference(o, ei, n, K, torch.float64, root)
    r32, _, _ = X.gmm_reference(o, ei, n, K, torch.float32, root)
    X.check_gmm_condition(family, o, aux["gamma"].detach(), aux["dst"], n)
    hc = K * C
    eye = torch.eye(hc + C, dtype=torch.float64)
    d = lambda t: t.double()
    with torch.no_grad():
        x = torch.cat([o["hf"], o["r"] if root else torch.zeros_like(o["r"])], 1).double()
        dense = dense_gmm(x, ei, d(o["attr"]), eye[:, :hc], d(o["mu"]), d(o["sigma"]), eye[hc:], d(o["bias"]), K)
    assert relerr(ref["y"], dense) < 1e-10
    bad = []
    for k in ref:
        assert bool(torch.isfinite(ref[k]).all()) and bool(torch.isfinite(r32[k]).all()), k
        yard = relerr(r32[k], ref[k])
        print("gmm %s C=%d K=%d dim=%d root=%s %s: float32 CPU yardstick %.2e" % (family, C, K, dim, root, k, yard))
        if not (math.isfinite(yard) and yard < 1e-3):
            bad.append((k, yard))
    assert not bad, bad

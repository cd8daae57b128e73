"""Operand families at which float32 arithmetic breaks unless the kernel guards it, for tests/test_extremes_cpu.py (which checks
that every family holds its stated condition on the reference's own scores) and tests/test_gpu_extremes.py (which runs the kernels
on them).  Plain module, no GPU.  Every generator is deterministic (a seeded ``torch.Generator``) and every scaling is a power
of two, so the float32 operands are the float64 operands exactly.

The references are the edge-list forms of tests/*_ref.py, reached through the ``kernel_reference`` functions of the operators'
own GPU test files; the graphs, the yardstick bound and the entry map come from test_gpu_gat.py.

Softmax families (GATConv, GATv2Conv, TransformerConv kernel-level operands), conditions on the post-leaky-ReLU score z:
* overflow  -- the largest z of most rows lies in [100, 1e4]: exp(z) without the row maximum is inf in float32;
* underflow -- the largest z of every non-empty row is <= -104: exp(z) without the row maximum is 0 on the whole row;
* dominant  -- on every non-empty row one coalesced entry exceeds all others by >= 200: alpha is exactly one-hot in float32;
* ties      -- all z of a row are equal (a zero attention vector / query): alpha_e = mult_e / sum(mult).

FeaStConv (a softmax over heads per edge) and GMMConv families: see ``feast_operands`` and ``gmm_operands``.
Head families (kind 1, the NormalNet head): ordinary | saturated | zero -- see ``head_operands``.
Optimizer operand sets: see ``optimizer_gradient``."""
import math

import numpy as np
import torch

import edge_weight_route_worker as W
from test_gpu_gat import FLOOR, OP_TOL, bound, entry_map, graphs  # noqa: F401  (re-exported: one place to import them from)
from test_gpu_gat import kernel_reference as gat_kernel_reference
from test_gpu_gatv2 import kernel_reference as gatv2_kernel_reference
from test_gpu_transformer import kernel_reference as tconv_kernel_reference

relerr = W.relerr

SOFTMAX_FAMILIES = ("overflow", "underflow", "dominant", "ties")
SOFTMAX_OPS = ("gat", "gatv2", "tconv")
SOFTMAX_GRAPHS = (("grid", True), ("hub-iso", False))           # (name, self loops where the operator has the option)
SOFTMAX_WIDTHS = ((3, 2), (8, 3))                               # (C per head, heads): scalar kernels | two lanes per head
OVERFLOW_ONLY_WIDTHS = ((64, 4),)


def softmax_cases():
    """-> [(op, family, graph name, loops, C, heads)]: what both test files run."""
    out = []
    for op in SOFTMAX_OPS:
        for fam in SOFTMAX_FAMILIES:
            for name, loops in SOFTMAX_GRAPHS:
                for C, heads in SOFTMAX_WIDTHS + (OVERFLOW_ONLY_WIDTHS if fam == "overflow" else ()):
                    out.append((op, fam, name, loops and op != "tconv", C, heads))
    return out


def _ranks(n, heads, gen):
    """[n, heads] float32: per head a permutation of 1..n -- distinct integers, exact in float32 far beyond these n."""
    return torch.stack([torch.randperm(n, generator=gen) for _ in range(heads)], 1).to(torch.float32) + 1.0


def softmax_operands(op, family, n, C, heads, seed=0):
    """-> dict of float32 CPU operands of the kernel-level calls of ``op``.

    gat:   hf, att_src, att_dst, bias, dout     (z = leaky(Hf[j].att_src + Hf[i].att_dst))
    gatv2: xl, xr, att, bias, dout              (z = att . leaky(Xl[j] + Xr[i]))
    tconv: q, k, v, skip, dout                  (z = Q[i] . K[j] / sqrt(C))"""
    gen = torch.Generator().manual_seed(1000 * seed + 31 * n + 7 * C + heads)
    hc = heads * C
    rn = lambda *s: torch.randn(*s, generator=gen)
    pos = lambda *s: rn(*s).abs() + 1.0                          # >= 1
    o = {"dout": rn(n, hc)}
    if op == "gat":
        o.update(hf=rn(n, hc), att_src=rn(heads, C) * 0.5, att_dst=rn(heads, C) * 0.5, bias=rn(hc))
        if family == "overflow":
            o["att_src"] *= 2.0 ** 8
            o["att_dst"] *= 2.0 ** 8
        elif family == "underflow":                              # every s <= -C * 2^8 / 2, z = 0.2 (s_src + s_dst) <= -0.2 C 2^8
            o["hf"] = -pos(n, hc)
            o["att_src"], o["att_dst"] = (rn(heads, C).abs() + 0.5) * 2.0 ** 8, (rn(heads, C).abs() + 0.5) * 2.0 ** 8
        elif family == "dominant":                               # s_src[j] = 2^11 rank_h(j) > 0, s_dst = 0
            o["hf"].view(n, heads, C)[:, :, 0] = _ranks(n, heads, gen)
            o["att_src"], o["att_dst"] = torch.zeros(heads, C), torch.zeros(heads, C)
            o["att_src"][:, 0] = 2.0 ** 11
        elif family == "ties":
            o["att_src"], o["att_dst"] = torch.zeros(heads, C), torch.zeros(heads, C)
    elif op == "gatv2":
        o.update(xl=rn(n, hc), xr=rn(n, hc), att=rn(heads, C) * 0.5, bias=rn(hc))
        if family == "overflow":                                 # att > 0: a row's largest score is positive
            o["att"] = o["att"].abs() * 2.0 ** 8
        elif family == "underflow":
            # components 1..: u >= 2 and att <= -2^k with (C - 1) 2^k 2 >= 112, no more: the float32 rounding of z grows with |z|
            # and att.  Component 0 keeps ordinary Xl, Xr (both signs) and a small att <= 0, worth at most +0.2 |att u| ~ 3:
            # with one leaky branch on a whole row, dXr = att leaky' sum(dz) would be zero in exact arithmetic, without a
            # relative error of its own
            free = (o["xl"].view(n, heads, C)[:, :, 0].clone(), o["xr"].view(n, heads, C)[:, :, 0].clone(), -o["att"][:, 0].abs())
            o["xl"], o["xr"] = pos(n, hc), pos(n, hc)
            o["att"] = -(rn(heads, C).abs() + 1.0) * 2.0 ** math.ceil(math.log2(56.0 / (C - 1)))
            o["xl"].view(n, heads, C)[:, :, 0], o["xr"].view(n, heads, C)[:, :, 0], o["att"][:, 0] = free
        elif family == "dominant":                               # z = 2^8 rank_h(j)
            o["xl"].view(n, heads, C)[:, :, 0] = _ranks(n, heads, gen)
            o["xr"].view(n, heads, C)[:, :, 0] = 0.0
            o["att"] = torch.zeros(heads, C)
            o["att"][:, 0] = 2.0 ** 8
        elif family == "ties":
            o["att"] = torch.zeros(heads, C)
    elif op == "tconv":
        o.update(q=rn(n, hc), k=rn(n, hc), v=rn(n, hc), skip=rn(n, hc))
        if family == "overflow":
            o["q"] *= 2.0 ** 7
        elif family == "underflow":                              # q >= 2^7, k <= -1: z <= -2^7 sqrt(C)
            o["q"], o["k"] = pos(n, hc) * 2.0 ** 7, -pos(n, hc)
        elif family == "dominant":                               # z = 2^10 rank_h(j) / sqrt(C)
            o["k"].view(n, heads, C)[:, :, 0] = _ranks(n, heads, gen)
            o["q"] = torch.zeros(n, hc)
            o["q"].view(n, heads, C)[:, :, 0] = 2.0 ** 10
        elif family == "ties":
            o["q"] = torch.zeros(n, hc)
    else:
        raise ValueError(op)
    return o


def softmax_reference(op, o, ei, n, heads, loops, dtype):
    """-> (dict of everything the kernels of ``op`` produce, rows of the coalesced entries), from the edge-list reference."""
    if op == "gat":
        return gat_kernel_reference(o["hf"], o["att_src"], o["att_dst"], o["bias"], o["dout"], ei, n, heads, loops, dtype)
    if op == "gatv2":
        return gatv2_kernel_reference(o["xl"], o["xr"], o["att"], o["bias"], o["dout"], ei, n, heads, loops, dtype)
    return tconv_kernel_reference(o["q"], o["k"], o["v"], o["skip"], o["dout"], ei, n, heads, dtype)


def softmax_scores(op, o, ei, n, heads, loops):
    """The reference's own z in float64 -> (z [E, heads], dst [E], src [E]) over the edges it attends over."""
    from gat_ref import gat_edge_list
    from gatv2_ref import gatv2_core
    from transformer_ref import transformer_core
    d = lambda t: t.double()
    if op == "gat":
        hc = o["hf"].shape[1]
        _, aux = gat_edge_list(d(o["hf"]).requires_grad_(True), ei, torch.eye(hc, dtype=torch.float64), d(o["att_src"]),
                               d(o["att_dst"]), d(o["bias"]), heads, True, 0.2, loops, full=True)      # (``full`` retains a gradient)
        z = torch.nn.functional.leaky_relu(aux["pre"], 0.2)
    elif op == "gatv2":
        _, aux = gatv2_core(d(o["xl"]), d(o["xr"]), ei, d(o["att"]), d(o["bias"]), heads, True, 0.2, loops, full=True)
        z = aux["z"]
    else:
        _, aux = transformer_core(d(o["q"]), d(o["k"]), d(o["v"]), ei, heads, True, full=True)
        z = aux["z"]
    return z.detach(), aux["dst"], aux["src"]


# Quantities that are ZERO in exact arithmetic, so the reference, its float32 evaluation and the device all hold rounding noise
# and there is no relative error of their own.  GAT's ds_dst[i] = sum over row i of ds, and ds = alpha (dal - delta) leaky'(pre):
# when every entry of the row that carries weight sits on ONE leaky branch the sum is that slope times sum(alpha (dal - delta))
# = 0.  Underflow forces pre < 0 on the whole row, ties have pre = 0, and with a row maximum >= 100 every entry within e^-100 of
# it has pre > 0.  datt_dst = sum_i ds_dst[i] Hf[i] inherits it.  As test_gpu_transformer.py does for the gradient of
# lin_key.bias, their error is taken relative to the norm of the sibling of the same shape and scale (the same sums of ds,
# taken down the columns instead of along the rows).
ZERO_IN_EXACT = {("gat", fam): {"ds_dst": "ds_src", "datt_dst": "datt_src"} for fam in ("overflow", "underflow", "ties")}


def measure(op, family, key, got, ref):
    """rel-L2 of ``got[key]`` from ``ref[key]``; for the ZERO_IN_EXACT quantities relative to the sibling's norm."""
    sib = ZERO_IN_EXACT.get((op, family), {}).get(key)
    if sib is None:
        return relerr(got[key], ref[key])
    return float((got[key].double().cpu() - ref[key].double().cpu()).norm() / (ref[sib].double().cpu().norm() + 1e-30))


def multiplicities(ei, n, loops):
    """float64 [entries]: how many edges of the attended edge list each coalesced entry stands for."""
    from gat_ref import gat_edges
    src, dst = gat_edges(ei, n, loops)
    _, rows, ent = entry_map(ei, n, loops, src, dst)
    return torch.bincount(ent, minlength=len(rows)).double()


def row_top_two(z, dst, src, n):
    """Per row and head the largest z and the largest z among the edges from ANOTHER source (duplicate edges are one coalesced
    entry) -> (top [n, heads], second [n, heads]); -inf where a row has no such edge."""
    heads = z.shape[1]
    idx = dst.view(-1, 1).expand(-1, heads)
    ninf = lambda: torch.full((n, heads), -math.inf, dtype=z.dtype)
    top = ninf().scatter_reduce(0, idx, z, "amax")
    arg = torch.full((n, heads), -1, dtype=torch.long)                    # the source of the top edge
    hit = z == top[dst]
    for h in range(heads):
        arg[dst[hit[:, h]], h] = src[hit[:, h]]
    other = torch.where(src.view(-1, 1) != arg[dst], z, torch.full_like(z, -math.inf))
    return top, ninf().scatter_reduce(0, idx, other, "amax")


def check_softmax_condition(family, z, dst, src, n):
    """Asserts the family's condition on the reference's scores."""
    top, second = row_top_two(z, dst, src, n)
    live = torch.isfinite(top)
    assert bool(live.any())
    if family == "overflow":
        inside = ((top >= 100) & (top <= 1e4))[live]
        assert float(inside.double().mean()) > 0.5, float(inside.double().mean())
        assert float(top[live].max()) <= 1e4
    elif family == "underflow":
        assert float(top[live].max()) <= -104, float(top[live].max())
    elif family == "dominant":
        gap = (top - second)[live]
        assert float(gap.min()) >= 200, float(gap.min())
    elif family == "ties":
        low = torch.full_like(top, math.inf).scatter_reduce(0, dst.view(-1, 1).expand(-1, z.shape[1]), z, "amin")
        assert torch.equal(top[live], low[live])


# ------------------------------------------------------------------------------------------------ heads
HEAD_FAMILIES = ("ordinary", "saturated", "zero")
SLOPE = 0.01


def head_operands(family, n, kind, seed=0):
    """Float32 CPU operands of ``ops.head_fwd`` / ``ops.head_bwd``: y [n, 32], a, b (the BatchNorm scale and shift of the load
    prologue), W1, b1, W2, b2, x_pos, dout.

    * ordinary  -- what test_gpu_kernels.py::test_heads_forward_backward draws.
    * saturated -- every third row has |u_o| >= 20 in all three outputs: tanh(u) = +-1 exactly and 1 - v^2 = 0 in float32 (and in
      float64: 1 - tanh(20) < 2^-53).  b2 is one vector for all rows and cannot single out a third of them, so the rows' own y
      does it: randn rows scaled by 2^7, SELECTED from four times as many candidates by |u| of the float64 forward.  The other rows
      are the ordinary family's.
    * zero      -- b1 = b2 = 0 and y = -b / a with a a power of two: z, t and u are exactly 0 on every row."""
    gen = torch.Generator().manual_seed(100 * seed + 10 * kind + HEAD_FAMILIES.index(family) + n)
    rn = lambda *s: torch.randn(*s, generator=gen)
    y = rn(n, 32)
    a, b = torch.rand(32, generator=gen) + 0.5, rn(32)
    W1, b1, W2, b2 = rn(16, 32) / 5, rn(16), rn(3, 16) / 3, rn(3)
    x_pos, dout = rn(n, 3), rn(n, 3)
    if family == "saturated":
        third = torch.arange(n) % 3 == 0
        want = int(third.sum())
        cand = rn(4 * want + 64, 32) * 2.0 ** 7
        u = head_reference(dict(y=cand, a=a, b=b, W1=W1, b1=b1, W2=W2, b2=b2), 1, torch.float64, forward_only=True)["u"]
        sat = cand[u.abs().min(1).values >= 20.0]
        if len(sat) < want:
            raise ValueError("head family 'saturated': %d of %d candidate rows saturate all three outputs" % (len(sat), want))
        y[third] = sat[:want]
    elif family == "zero":
        a = 2.0 ** torch.randint(-1, 2, (32,), generator=gen).float()
        b = torch.randint(-8, 9, (32,), generator=gen).float() / 8
        y = (-b / a).expand(n, 32).contiguous()
        b1, b2 = torch.zeros(16), torch.zeros(3)
    return dict(y=y, a=a, b=b, W1=W1, b1=b1, W2=W2, b2=b2, x_pos=x_pos, dout=dout)


def head_reference(o, kind, dtype, n_rows=None, forward_only=False):
    """The composition of test_heads_forward_backward in ``dtype`` -> dict(u, out, dz, dW1, db1, dW2, db2); ``n_rows``: the rows
    that take part (out and dz have that many)."""
    c = lambda t: t.to(dtype)
    y = c(o["y"])[:n_rows]
    z0 = y * c(o["a"]) + c(o["b"])
    z = torch.where(z0 > 0, z0, SLOPE * z0).requires_grad_(not forward_only)
    P = [c(o[k]).clone().requires_grad_(not forward_only) for k in ("W1", "b1", "W2", "b2")]
    t = torch.nn.functional.leaky_relu(z @ P[0].t() + P[1], SLOPE)
    u = t @ P[2].t() + P[3]
    if forward_only:
        return dict(u=u)
    if kind == 0:
        out = c(o["x_pos"])[:n_rows] + u
    else:
        v = torch.tanh(u)
        out = v * torch.reciprocal(torch.norm(v, dim=1, keepdim=True) + 1e-12)
    g = torch.autograd.grad(out, [z] + P, c(o["dout"])[:n_rows])
    return dict(u=u.detach(), out=out.detach(), dz=g[0], dW1=g[1], db1=g[2], dW2=g[3], db2=g[4])


HEAD_KEYS = ("out", "dz", "dW1", "db1", "dW2", "db2")
HEAD_TOL = dict(out=2e-6, dz=1e-5, dW1=1e-5, db1=1e-5, dW2=1e-5, db2=1e-5)     # the bounds of test_heads_forward_backward


# ------------------------------------------------------------------------------------------------ optimizer
OPT_SIZES = (1, 257, 65537, 524289)                             # 524289 = 2048 * 256 + 1: adam_kernel starts striding
OPT_SETS = ("huge", "tiny", "mixed")
LR, BETAS, ADAM_EPS, MAX_NORM = 0.01, (0.9, 0.999), 1e-8, 0.8


def optimizer_gradient(kind, n, step, seed=0):
    """float32 [n] gradient of one step.  "huge": every element +-1e20 (squares leave float32, the sum of squares is float64 by
    design); "tiny": +-1e-30 (squares underflow float32); "mixed": alternately +-1e20 and +-1e-30; "below": randn scaled by a
    power of two to a norm in (0.2, 0.4], below MAX_NORM; "zero"."""
    gen = torch.Generator().manual_seed(7919 * seed + 13 * n + step)
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    mag = torch.rand(n, generator=gen) + 1.0                      # [1, 2)
    if kind == "huge":
        return sign * mag * 1e20
    if kind == "tiny":
        return sign * mag * 1e-30
    if kind == "mixed":
        return sign * mag * torch.where(torch.arange(n) % 2 == 0, torch.tensor(1e20), torch.tensor(1e-30))
    if kind == "zero":
        return torch.zeros(n)
    if kind == "below":
        g = torch.randn(n, generator=gen)
        if n == 1:
            g = g.abs() + 0.5
        return g * 2.0 ** (math.floor(math.log2(0.4 / float(g.double().norm()))))
    raise ValueError(kind)


def clip_adam_f64(p, m, v, g, step, lr=LR, betas=BETAS, eps=ADAM_EPS, max_norm=MAX_NORM):
    """clip_grad_norm_(max_norm) + one torch.optim.Adam step restated in float64 -> (p, m, v, clipped g); ``max_norm`` None: no
    clip.  lr, betas and eps are the float32 values the library receives."""
    f32 = lambda x: float(np.float32(x))
    lr, b1, b2, eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)
    p, m, v, g = p.double(), m.double(), v.double(), g.double()
    if max_norm is not None:
        c = f32(max_norm) / (float(g.norm()) + 1e-6)
        g = g * min(c, 1.0)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1 - b2 ** step) + eps
    return p - lr / (1 - b1 ** step) * (m / denom), m, v, g


def adam_coefficients(t, lr=LR, betas=BETAS):
    """(lr / (1 - b1^t), sqrt(1 - b2^t)) in float64 from the float32 lr and betas."""
    lr, b1, b2 = (float(np.float32(x)) for x in (lr, betas[0], betas[1]))
    return lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)


# ------------------------------------------------------------------------------------------------ FeaStConv (softmax over heads)
FEAST_FAMILIES = ("steep", "offsets", "flat")
FEAST_WIDTHS = ((3, 2), (40, 3))                                 # (C, heads): two of test_gpu_feast.py's CASES
FEAST_GRAPHS = (("grid", True), ("hub-iso", False))


def feast_operands(family, n, C, heads, seed=0):
    """hf [n, heads * C], p [n, heads], c [heads], bias [C], dout [n, C]; the logits of an edge j -> i are P[j] - P[i] + c.
    "steep": p scaled by 2^7 -- on most edges one head leads by more than exp can hold, the softmax over heads is one-hot there;
    "offsets": c = +300, -300, +300, ...; "flat": p = 0 and c = 0 -- every head gets exactly 1 / heads."""
    gen = torch.Generator().manual_seed(1000 * seed + 31 * n + 7 * C + heads + 5)
    rn = lambda *s: torch.randn(*s, generator=gen)
    o = dict(hf=rn(n, heads * C), p=rn(n, heads), c=rn(heads) * 0.5, bias=rn(C), dout=rn(n, C))
    if family == "steep":
        o["p"] *= 2.0 ** 7
    elif family == "offsets":
        o["c"] = 300.0 * (1.0 - 2.0 * (torch.arange(heads) % 2).float())
    elif family == "flat":
        o["p"], o["c"] = torch.zeros(n, heads), torch.zeros(heads)
    return o


def feast_reference(o, ei, n, heads, loops, dtype):
    from test_gpu_feast import kernel_reference
    ref, rows, ent, aux = kernel_reference(o["hf"], o["p"], o["c"], o["bias"], o["dout"], ei, n, heads, loops, dtype)
    return ref, rows, aux


def check_feast_condition(family, z):
    """``z``: the reference's own logits [E, heads]."""
    top = z.max(1).values
    gap = top - z.topk(2, 1).values[:, 1]
    if family == "steep":                                        # on a third of the edges or more (an added self loop has z = c):
        # exp(top) overflows without the maximum, and every other head underflows to exactly 0 beside it
        assert float((top > 88.7).double().mean()) > 1 / 3 and float((gap > 104).double().mean()) > 1 / 3
    elif family == "offsets":
        assert float(top.min()) >= 290 and float((top - z.min(1).values).min()) >= 590
    else:
        assert not z.any()


# ------------------------------------------------------------------------------------------------ GMMConv
GMM_FAMILIES = ("tiny-sigma", "zero-sigma", "huge-sigma", "far-mu")
GMM_WIDTHS = ((3, 2, 3), (40, 3, 1))                             # (C, K, dim): two of test_gpu_gmm.py's CASES
GMM_GRAPH = "hub-iso"


def gmm_operands(family, n, E, C, K, dim, seed=0):
    """hf [n, K * C], r [n, C] (the root term), attr [E, dim], mu, sigma [K, dim], bias [C], dout [n, C] as test_gpu_gmm.py draws
    them (attr, mu in [0, 1], sigma in [0.3, 1]), then: "tiny-sigma": sigma = 2^-10 (nearly every Gaussian underflows: rows keep
    root + bias alone); "zero-sigma": sigma[0, 0] = 0 -- the EPS path, 1 / (EPS + 0) = 1e15 -- with attr[e, 0] = mu[0, 0] exactly
    on the first 40 edges; "huge-sigma": sigma = 2^10; "far-mu": mu = +-2^10.  sigma = 0 and the far mu stay apart: their product
    is 0 * inf in any float32 arithmetic."""
    gen = torch.Generator().manual_seed(1000 * seed + 31 * n + 7 * C + K + 11)
    rn = lambda *s: torch.randn(*s, generator=gen)
    o = dict(hf=rn(n, K * C), r=rn(n, C), bias=rn(C), dout=rn(n, C), attr=torch.rand(E, dim, generator=gen),
             mu=torch.rand(K, dim, generator=gen), sigma=0.3 + 0.7 * torch.rand(K, dim, generator=gen))
    if family == "tiny-sigma":
        o["sigma"] = torch.full((K, dim), 2.0 ** -10)
    elif family == "zero-sigma":
        o["sigma"][0, 0] = 0.0
        o["attr"][:40, 0] = o["mu"][0, 0]
    elif family == "huge-sigma":
        o["sigma"] = torch.full((K, dim), 2.0 ** 10)
    elif family == "far-mu":
        o["mu"] = 2.0 ** 10 * (1.0 - 2.0 * (torch.arange(K * dim) % 2).float()).view(K, dim)
    return o


def gmm_reference(o, ei, n, K, dtype, root=True):
    """-> (dict(y, w, dhf, dr, dmu, dsigma, dattr), rows of the coalesced entries, aux); ``root`` False: y without the root term
    (dr is then dropped)."""
    from test_gpu_gmm import entry_map as gmm_entry_map, kernel_reference
    _, rows, ent = gmm_entry_map(ei, n)
    r = o["r"] if root else torch.zeros_like(o["r"])
    ref, aux = kernel_reference(o["hf"], r, o["attr"], o["mu"], o["sigma"], o["bias"], o["dout"], ei, n, K, dtype, ent, len(rows))
    if not root:
        del ref["dr"]
    return ref, rows, aux


def check_gmm_condition(family, o, gamma, dst, n):
    """``gamma``: the reference's own Gaussians [E, K] in float64."""
    live = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, gamma.sum(1))
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(len(dst), dtype=torch.float64))
    if family == "tiny-sigma":                                   # rows that lose every Gaussian beside rows that keep one
        dead = float(((live == 0) & (deg > 0)).double().sum() / (deg > 0).double().sum())
        assert 0.05 < dead < 1.0, dead
    elif family == "zero-sigma":
        assert float(o["sigma"][0, 0]) == 0.0 and bool((o["attr"][:40, 0] == o["mu"][0, 0]).all())
        assert float(gamma[:40, 0].min()) > 1e-3 and float(gamma[40:, 0].max()) == 0.0
    elif family == "huge-sigma":
        assert float(gamma.min()) > 0.999999
    else:
        assert not gamma.any()

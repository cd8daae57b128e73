"""Cases, references and bounds for the BatchNorm + LeakyReLU kernels (csrc/bn.hip, csrc/finalize.h) at hard columns.
Plain module, no GPU: tests/test_bn_cases_cpu.py holds the cases and bounds themselves to account, tests/test_gpu_bn.py runs
the kernels against them.

A case is an [n, C] float32 matrix y, a gradient dz, and gamma / beta.  Column c belongs to family
(c + shift) % len(families), so one launch covers every family; every column draws from a generator of its own (seeded by the
case's seed and the column), so a block of columns can be made without the rest.  All scalings are powers of two and the operands
are rounded to float32 (or bfloat16) BEFORE anything is computed from them: the float64 reference sees exactly the values the
kernels see.

    family      y                                  gamma         what it is for
    ordinary    3 + 2 N(0,1)                       [0.5, 1.5]    the operands every earlier test used
    offset32    32 + N(0,1)                        positive      |mean| >> sigma: y*a + shift and c1*y + c0 cancel
    offset1k    1024 + N(0,1)                      positive      ... by three more digits; the float32 `mean` row costs accuracy
    tiny        0.5 + 2^-10 N(0,1)                 positive      variance ~1e-6 < eps: rstd is eps-limited (~316)
    const       1.5 on every row                   positive      variance exactly 0 (see below)
    neg_gamma   1 + 2 N(0,1)                       [-1.5, -0.5]  lrelu'(fma(y, a, b)) with a < 0
    zero_gamma  1 + 2 N(0,1)                       exactly 0     z = beta, dY = 0
    big         2^40 (3 + 2 N(0,1))                positive      y^2 ~ 2^85: float64 sums, float32 coefficients ~2^-41 .. 2^-82
    small       2^-40 (3 + 2 N(0,1))               positive      variance ~ 2^-78 << eps, values far below eps

beta = +-(0.25 + |N(0,1)|) in every column: z = beta on the const and zero_gamma columns (and on every column at n = 1), which
must stay clear of the LeakyReLU's kink.

The const family is valid against eps only for small |y|.  The kernels take the variance as s1/n - (s0/n)^2 from float64 sums;
at y = 1.5 every term is exact and the variance is exactly 0, but for a general constant v the sums round and leave a residue of
either sign of about n^(1/2) .. n times 2^-53 v^2.  The negative one is clamped (`var < 0`), the positive one adds to eps: it
moves rstd by residue / (2 eps) of itself, which stays below a quarter of eps32 = 2^-24 while v^2 <~ 2^-26 eps 2^53 / n, i.e.
|v| <= 32 at n <= 1000 and |v| <= 4 at n = 65541.  The family stays at 1.5; the clamp itself is tested on sums made by hand.

At n = 1 every column is a constant column of value y, z = beta analytically, and float32 computes it as the difference of
two numbers of size |y| gamma / sqrt(eps): the pre-activation is ambiguous (below) as soon as KZ eps32 2 |y| 1.5 / sqrt(eps)
reaches |beta| >= 0.25, i.e. from |y| ~ 270.  The n = 1 cases therefore leave out offset1k and big (N1_FAMILIES).

Gradient kinds: `random` dz = N(0,1); `correlated` dz = N(0,1) + 0.75 yhat + 0.5 with yhat the float64 normalised column
(0 where the column is constant), which makes dgamma/n and dbeta/n O(1), so that the c1*y + c0 half of dY carries weight.

References.  reference(): float64 closed form (two-pass variance), equal to torch autograd through BatchNorm1d(train).double()
and leaky_relu (reference_autograd(); tests/test_bn_cases_cpu.py shows the two equal).  oracle32(): numpy restatement of the
kernels' own arithmetic -- float64 sums of float32 values, mean / rstd / scale / shift / c1 / c0 rounded to float32 exactly
where finalize_column rounds them, shift = fma(-mean32, scale, beta), yhat = (y - mean32) * rstd32 in float32.  It calibrates the
bounds; it is not a second reference.

Bounds, elementwise or per column, in units of eps32 = 2^-24 against scales made of the formula's own terms (reference
coefficients):

    z       |z - ref|   <= KZ eps32 Sz_c,   Sz_c = max_r |y scale| + |shift|
    dY      |dY - ref|  <= KD eps32 Sd_c,   Sd_c = |scale| max_r |dz| + |c1| max_r |y| + |c0|
    dY      |dY - ref|  <= KDT eps32 (Sd_c + Sm_c),   Sm_c = |scale| max_r |yhat| |mean| rstd sum_r |g| / n
    dbeta   |.. - ref|  <= KB eps32 sum_r |g|
    dgamma  |.. - ref|  <= KG eps32 (sum_r |g yhat| + |mean| rstd sum_r |g|)
    running |.. - ref|  <= KR eps32 ((1 - m) |running| + m |statistic|) per call
    sums of bn_stats (and the column sums of the stored dY): relative 1e-12 against float64 sums of the same values

The second term of the dgamma bound is the cost of the float32 `mean` row: yhat = (y - mean32) rstd is off by up to
eps32/2 |mean| rstd in every row, with one sign down the column.  PyTorch's float32 BatchNorm pays the same.  It is stated here,
not fixed.  The same cost reaches dY through c1 = -scale rstd dgamma / n: that is Sm_c.  With Sd_c alone, as the first dY
bound has it, a column with |mean| >> sigma and a gradient uncorrelated with y (dgamma/n ~ n^-1/2, so c1 is small and Sd_c
with it) is off by a large multiple of eps32 Sd_c in the oracle already: 112 on an offset1k column at n = 33, random gradient.
KD follows the rule below from that figure, which leaves the first bound loose on every other column; the second bound, with
the term that explains the figure, is the sharp one (the oracle's worst is 2.5), and both are asserted.

KR is not measured but counted: (1 - m) in float32, two products, one sum and the float32 statistic are five
roundings of at most eps32 of the larger side each, and momentum 0.1f is 1.5e-8 from 0.1: 8 per call, 8 k after k calls.

Sign ambiguity.  Where |gamma yhat + beta| <= KZ eps32 Sz_c the float32 sign of the pre-activation may differ from the
reference's.  On such elements z and dY pass if they match the reference taken with either LeakyReLU branch, and the column's
dbeta / dgamma / dY bounds grow by what the flipped elements can move: (1 - slope) sum_amb |dz|, (1 - slope) sum_amb |dz yhat|,
and |scale| (the first + max|yhat| the second) / n.  The ambiguous share of a case is capped at AMB_SHARE = 1e-3.

Constants: 4 x the worst value oracle32 reaches against reference over every case of CHAIN_CASES and BF16_CASES, rounded up to
a power of two (the margin covers the device's summation order and fma contraction, which the oracle does not reproduce).

    quantity          oracle32 worst (case, family)              constant    kernels' worst on an MI355X
    z                 2.14  (29x1024 correlated, neg_gamma)      KZ  = 16    2.14
    dY, Sd_c alone    112.2 (33x1024 random, offset1k)           KD  = 512   112.2
    dY, Sd_c + Sm_c   2.52  (32771x1024 random, small)           KDT = 16    2.52
    dbeta             1.61  (2x1024 random, zero_gamma)          KB  = 8     1.61
    dgamma            1.97  (3x1024 random, zero_gamma)          KG  = 8     1.97
    running mean      1.88 after one call                        KR  = 8     3.33 after three calls (limit 24)
    running variance  1.89 after one call                        KR  = 8     3.98 after three calls (limit 24)

The kernels reach the oracle's figures to three digits on every quantity: the oracle states their arithmetic, and neither
the device's summation order nor fma contraction shows at this resolution.  The largest ambiguous share of a case is 3.3e-4
(3x1024 correlated); no n = 1 case has an ambiguous element.  bfloat16: the same bounds behind the store's half ulp
(2^-8 relative), worst z 1.99, dY 2.67 (Sd_c alone) in oracle and kernels alike.
"""
import math

import numpy as np
import torch

EPS32 = 2.0 ** -24
BN_EPS = 1e-5
MOMENTUM = 0.1
SLOPE = float(np.float32(0.01))                # the kernels take the slope as a float32 argument: that number is the operand
AMB_SHARE = 1e-3

KZ, KD, KDT, KB, KG, KR = 16.0, 512.0, 16.0, 8.0, 8.0, 8.0

FAMILIES = ("ordinary", "offset32", "offset1k", "tiny", "const", "neg_gamma", "zero_gamma", "big", "small")
N1_FAMILIES = tuple(f for f in FAMILIES if f not in ("offset1k", "big"))       # n = 1: see the module docstring
BF16_FAMILIES = ("ordinary", "offset32", "neg_gamma", "zero_gamma", "const", "tiny")
KINDS = ("random", "correlated")
# y = offset + spread N(0,1), per family (for the tests that have a kernel PRODUCE a family matrix from a bias and a spread)
FAMILY_AFFINE = {"ordinary": (3.0, 2.0), "offset32": (32.0, 1.0), "offset1k": (1024.0, 1.0), "tiny": (0.5, 2.0 ** -10),
                 "const": (1.5, 0.0), "neg_gamma": (1.0, 2.0), "zero_gamma": (1.0, 2.0), "big": (3.0 * 2.0 ** 40, 2.0 ** 41),
                 "small": (3.0 * 2.0 ** -40, 2.0 ** -39)}


class Case:
    def __init__(self, n, C, kind="correlated", shift=0, families=FAMILIES, bf16=False, seed=0):
        assert kind in KINDS
        self.n, self.C, self.kind, self.shift, self.families, self.bf16, self.seed = n, C, kind, shift, tuple(families), bf16, seed

    @property
    def id(self):
        return "%s%dx%d-%s%s" % ("bf16-" if self.bf16 else "", self.n, self.C, self.kind, "-s%d" % self.shift if self.shift else "")

    def family(self, c):
        return self.families[(c + self.shift) % len(self.families)]

    def columns_of(self, fam, lo=0, hi=None):
        return [c - lo for c in range(lo, self.C if hi is None else hi) if self.family(c) == fam]

    def blocks(self, width=128):
        return [(lo, min(self.C, lo + width)) for lo in range(0, self.C, width)]

    def make(self, lo=0, hi=None):
        """-> Data of columns [lo, hi): float32 CPU tensors holding the operands (already rounded to bfloat16 for a bf16 case)."""
        hi = self.C if hi is None else hi
        n = self.n
        y, dz = torch.empty(n, hi - lo), torch.empty(n, hi - lo)
        gamma, beta = torch.empty(hi - lo), torch.empty(hi - lo)
        gen = torch.Generator()
        for c in range(lo, hi):
            fam = self.family(c)
            gen.manual_seed(1000003 * self.seed + 7919 * n + 31 * c + (1 if self.kind == "correlated" else 0) + 17 * self.shift)
            v = torch.randn(n, generator=gen)
            u, b, e = torch.rand(1, generator=gen).item(), torch.randn(1, generator=gen).item(), torch.randn(n, generator=gen)
            if fam == "ordinary":
                col = 3.0 + 2.0 * v
            elif fam == "offset32":
                col = 32.0 + v
            elif fam == "offset1k":
                col = 1024.0 + v
            elif fam == "tiny":
                col = 0.5 + 2.0 ** -10 * v
            elif fam == "const":
                col = torch.full((n,), 1.5)
            elif fam in ("neg_gamma", "zero_gamma"):
                col = 1.0 + 2.0 * v
            elif fam == "big":
                col = 2.0 ** 40 * (3.0 + 2.0 * v)
            else:
                col = 2.0 ** -40 * (3.0 + 2.0 * v)
            if self.bf16:
                col = col.to(torch.bfloat16).float()
            g = 0.0 if fam == "zero_gamma" else (-(0.5 + u) if fam == "neg_gamma" else 0.5 + u)
            d = e
            if self.kind == "correlated":
                cd = col.double()
                dev = cd - cd.mean()
                var = float((dev * dev).mean())
                yhat = dev / math.sqrt(var + BN_EPS) if var > 0 else torch.zeros(n, dtype=torch.float64)
                d = (e.double() + 0.75 * yhat + 0.5).float()
            if self.bf16:
                d = d.to(torch.bfloat16).float()
            y[:, c - lo], dz[:, c - lo] = col, d
            gamma[c - lo], beta[c - lo] = g, math.copysign(0.25 + abs(b), b)
        return Data(self, lo, hi, y, dz, gamma, beta)


class Data:
    def __init__(self, case, lo, hi, y, dz, gamma, beta):
        self.case, self.lo, self.hi, self.y, self.dz, self.gamma, self.beta = case, lo, hi, y, dz, gamma, beta
        self.n, self.C = y.shape

    def families(self):
        return [self.case.family(c) for c in range(self.lo, self.hi)]

    def running_start(self):
        """A non-trivial start of the running statistics (float32, exact in float64)."""
        c = torch.arange(self.lo, self.hi, dtype=torch.float32)
        return 0.25 + (c % 5) * 0.125, 2.0 - (c % 3) * 0.5


# ------------------------------------------------------------------------------------------------- float64 references
MUTANTS = ("unbiased_forward", "no_eps", "c0_plus", "lrelu_from_y", "abs_gamma", "running_biased", "momentum_swapped")


def reference(d, device="cpu", running=None, calls=1, mutant=None):
    """Float64 closed form of BatchNorm1d(train) + LeakyReLU forward and backward on `d` (Data or any object with y, dz,
    gamma, beta); every tensor of the result is float64 on `device`.  `running` = (mean, var) start, default
    d.running_start(); `calls`: how many successive forward calls update them.  `mutant`: one of MUTANTS, a deliberately
    wrong variant (tests/test_bn_cases_cpu.py: the bounds reject each)."""
    y, dz = d.y.to(device).double(), d.dz.to(device).double()
    gamma, beta = d.gamma.to(device).double(), d.beta.to(device).double()
    n = y.shape[0]
    mean = y.sum(0) / n
    dev = y - mean
    var = (dev * dev).sum(0) / n
    var_fwd = var * n / (n - 1) if mutant == "unbiased_forward" and n > 1 else var
    rstd = 1.0 / torch.sqrt(var_fwd + (0.0 if mutant == "no_eps" else BN_EPS))
    yhat = dev * rstd
    gm = gamma.abs() if mutant == "abs_gamma" else gamma
    scale = gm * rstd
    shift = beta - mean * scale
    pre = gm * yhat + beta
    z = torch.where(pre > 0, pre, SLOPE * pre)
    on = y if mutant == "lrelu_from_y" else pre
    slope_of = torch.where(on > 0, 1.0, SLOPE)
    g = dz * slope_of
    dbeta, dgamma = g.sum(0), (g * yhat).sum(0)
    c1 = -scale * rstd * dgamma / n
    c0 = -scale * dbeta / n + (c1 * mean if mutant == "c0_plus" else -c1 * mean)
    if mutant == "c0_plus":
        dy = scale * g + c1 * y + c0
    else:
        dy = scale * (g - dbeta / n - yhat * (dgamma / n))          # the same function without the cancellation at |mean| >> sigma
    rm, rv = (t.to(device).double() for t in (running if running is not None else d.running_start()))
    unb = var if (n == 1 or mutant == "running_biased") else var * n / (n - 1)
    m = 1.0 - MOMENTUM if mutant == "momentum_swapped" else MOMENTUM
    for _ in range(calls):
        rm, rv = (1.0 - m) * rm + m * mean, (1.0 - m) * rv + m * unb
    return dict(z=z, dy=dy, dgamma=dgamma, dbeta=dbeta, run_mean=rm, run_var=rv,
                sums=torch.cat([y.sum(0), (y * y).sum(0)]), sums2=torch.cat([dbeta, dgamma]),
                mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, c1=c1, c0=c0, pre=pre, yhat=yhat, g=g)


def reference_autograd(d, running=None, calls=1):
    """The same through torch autograd: BatchNorm1d(train).double() then leaky_relu (n >= 2: torch refuses n = 1)."""
    C = d.y.shape[1]
    bn = torch.nn.BatchNorm1d(C, eps=BN_EPS, momentum=MOMENTUM).double()
    rm, rv = running if running is not None else d.running_start()
    with torch.no_grad():
        bn.weight.copy_(d.gamma)
        bn.bias.copy_(d.beta)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    bn.train()
    y = d.y.double().requires_grad_(True)
    for _ in range(calls - 1):
        bn(y.detach())
    z = torch.nn.functional.leaky_relu(bn(y), SLOPE)
    z.backward(d.dz.double())
    return dict(z=z.detach(), dy=y.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, run_mean=bn.running_mean.detach(),
                run_var=bn.running_var.detach())


# ------------------------------------------------------------------------------------------------- the kernels' arithmetic
def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _fma32(a, b, c):
    """float32 fma of float32 operands: the product is exact in float64; one float64 rounding under the float32 one."""
    return _f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def oracle32(d, running=None, calls=1):
    """numpy restatement of bn_stats -> bn_prepare -> bn_lrelu_apply -> bn_bwd_reduce -> bn_bwd_prepare -> bn_bwd_apply as
    the kernels compute them (see the module docstring); float64 numpy arrays out, keyed like reference()."""
    y, dz = d.y.numpy(), d.dz.numpy()
    gamma, beta = d.gamma.numpy(), d.beta.numpy()
    n = y.shape[0]
    yd = y.astype(np.float64)
    s0, s1 = yd.sum(0), (yd * yd).sum(0)
    mu = s0 / n
    var = np.maximum(s1 / n - mu * mu, 0.0)
    muf = _f32(mu)
    rs = _f32(1.0 / np.sqrt(var + np.float64(np.float32(BN_EPS))))
    a = gamma * rs                                                  # float32 product
    b = _fma32(-muf, a, beta)
    rm, rv = (t.numpy().astype(np.float32) for t in (running if running is not None else d.running_start()))
    unb = var * n / (n - 1.0) if n > 1 else var
    m = np.float32(MOMENTUM)
    for _ in range(calls):
        rm = (np.float32(1) - m) * rm + m * muf
        rv = (np.float32(1) - m) * rv + m * _f32(unb)
    pre = _fma32(y, a[None, :], b[None, :])
    z = np.maximum(pre, np.float32(SLOPE) * pre)
    g = dz * np.where(pre > 0, np.float32(1), np.float32(SLOPE))     # float32 product
    yhat = (y - muf[None, :]) * rs[None, :]                          # two float32 roundings
    db, dg = g.astype(np.float64).sum(0), (g.astype(np.float64) * yhat.astype(np.float64)).sum(0)
    a64, r64, mu64 = a.astype(np.float64), rs.astype(np.float64), muf.astype(np.float64)
    k1 = -a64 * r64 * dg / n
    c1, c0 = _f32(k1), _f32(-a64 * db / n - k1 * mu64)
    dy = _fma32(a[None, :], g, _fma32(c1[None, :], y, c0[None, :]))
    f = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float64))
    return dict(z=f(z), dy=f(dy), dgamma=f(_f32(dg)), dbeta=f(_f32(db)), run_mean=f(rm), run_var=f(rv),
                sums=f(np.concatenate([s0, s1])), sums2=f(np.concatenate([db, dg])),
                bn4=f(np.stack([a, b, muf, rs])), c10=f(np.stack([c1, c0])))


# ------------------------------------------------------------------------------------------------- the comparison
def scales(d, ref):
    """Per-column scales of the bounds and the ambiguous elements, from the reference's own terms (float64, ref's device)."""
    dev = ref["z"].device
    y, dz = d.y.to(dev).double(), d.dz.to(dev).double()
    n = y.shape[0]
    sz = (y * ref["scale"]).abs().amax(0) + ref["shift"].abs()
    sd = ref["scale"].abs() * dz.abs().amax(0) + ref["c1"].abs() * y.abs().amax(0) + ref["c0"].abs()
    amb = ref["pre"].abs() <= KZ * EPS32 * sz
    flip = (1.0 - SLOPE) * (dz.abs() * amb)
    amb_db, amb_dg = flip.sum(0), (flip * ref["yhat"].abs()).sum(0)
    sb = ref["g"].abs().sum(0)
    sg = (ref["g"] * ref["yhat"]).abs().sum(0) + ref["mean"].abs() * ref["rstd"] * sb
    amb_dy = ref["scale"].abs() * (amb_db + ref["yhat"].abs().amax(0) * amb_dg) / n
    sm = ref["scale"].abs() * ref["yhat"].abs().amax(0) * ref["mean"].abs() * ref["rstd"] * sb / n
    return dict(sz=sz, sd=sd, sdt=sd + sm, sb=sb, sg=sg, amb=amb, amb_db=amb_db, amb_dg=amb_dg, amb_dy=amb_dy,
                amb_share=float(amb.double().mean()))


def _ratio(err, bound):
    """err / bound with 0 / 0 = 0 (a zero_gamma column has dY = 0 against a bound of 0) and x / 0 = inf."""
    r = err / bound
    r = torch.where((bound == 0) & (err == 0), torch.zeros_like(r), r)
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)


def ratios(got, d, ref, sc=None, rel=0.0):
    """-> {quantity: float64 [C] on the CPU}: the worst error of each column in units of eps32 x its scale (to be held
    against KZ, KD, KB, KG, calls x KR), with the either-branch rule on ambiguous elements and their allowance taken off
    first.  `got` holds any of z, dy, dbeta, dgamma, run_mean, run_var (anything castable to float64).  `rel`: a relative
    error of the reference taken off the errors of z and dY first (2^-8 for tensors stored in bfloat16)."""
    sc = sc or scales(d, ref)
    dev = ref["z"].device
    out = {}
    G = {k: v.to(dev).double() for k, v in got.items() if k in ("z", "dy", "dbeta", "dgamma", "run_mean", "run_var")}
    amb = sc["amb"]
    if "z" in G:
        e = ((G["z"] - ref["z"]).abs() - rel * ref["z"].abs()).clamp_min(0)
        if amb.any():
            other = torch.where(ref["pre"] > 0, SLOPE * ref["pre"], ref["pre"])
            e = torch.where(amb, torch.minimum(e, ((G["z"] - other).abs() - rel * other.abs()).clamp_min(0)), e)
        out["z"] = _ratio(e.amax(0), EPS32 * sc["sz"])
    if "dy" in G:
        e = ((G["dy"] - ref["dy"]).abs() - rel * ref["dy"].abs()).clamp_min(0)
        if amb.any():
            dz = d.dz.to(dev).double()
            other = ref["dy"] + ref["scale"] * dz * torch.where(ref["pre"] > 0, SLOPE - 1.0, 1.0 - SLOPE)
            e = torch.where(amb, torch.minimum(e, ((G["dy"] - other).abs() - rel * other.abs()).clamp_min(0)), e)
            e = (e - sc["amb_dy"]).clamp_min(0)
        out["dy"] = _ratio(e.amax(0), EPS32 * sc["sd"])
        out["dyt"] = _ratio(e.amax(0), EPS32 * sc["sdt"])
    if "dbeta" in G:
        out["dbeta"] = _ratio(((G["dbeta"] - ref["dbeta"]).abs() - sc["amb_db"]).clamp_min(0), EPS32 * sc["sb"])
    if "dgamma" in G:
        out["dgamma"] = _ratio(((G["dgamma"] - ref["dgamma"]).abs() - sc["amb_dg"]).clamp_min(0), EPS32 * sc["sg"])
    if "run_mean" in G:
        m = MOMENTUM
        out["run_mean"] = _ratio((G["run_mean"] - ref["run_mean"]).abs(), EPS32 * (ref["run_mean"].abs() + m * ref["mean"].abs()))
        unb = ref["var"] * (d.y.shape[0] / max(1.0, d.y.shape[0] - 1.0))
        out["run_var"] = _ratio((G["run_var"] - ref["run_var"]).abs(), EPS32 * (ref["run_var"].abs() + m * unb))
    return {k: v.cpu() for k, v in out.items()}


LIMITS = {"z": KZ, "dy": KD, "dyt": KDT, "dbeta": KB, "dgamma": KG, "run_mean": KR, "run_var": KR}


def misses(rat, fams, calls=1, part=1.0):
    """-> list of (quantity, family, worst ratio, limit) over the columns whose ratio exceeds part x the limit."""
    bad = []
    for q, r in rat.items():
        lim = LIMITS[q] * (calls if q.startswith("run_") else 1) * part
        for c in torch.nonzero(~(r <= lim)).flatten().tolist():
            bad.append((q, fams[c], float(r[c]), lim))
    return bad


def worst(rat):
    return {q: float(r.max()) for q, r in rat.items()}


def sum_misses(got, vals, rel=1e-12):
    """Column sums `got` [C] against the float64 column sums of `vals` [n, C]: |err| <= rel x sum |terms|, per column.
    -> the worst err / (sum |terms|)."""
    v = vals.double()
    err = (got.to(v.device).double() - v.sum(0)).abs()
    return float(_ratio(err, v.abs().sum(0)).max())


def run_chain(ops, y, dz, gamma, beta, running, calls=1):
    """bn_stats -> bn_prepare (`calls` times: the running statistics move each time) -> bn_lrelu_apply (where `ops` has it)
    -> bn_bwd_reduce -> bn_bwd_prepare -> bn_bwd_apply through `ops` (the product's ops module, or tests/cpu_ops_stub.py) on
    tensors of the caller's device and dtype; `running` = (mean, var) is updated in place."""
    n, C = y.shape
    f32 = dict(dtype=torch.float32, device=y.device)
    bn4, c10 = torch.empty(4, C, **f32), torch.empty(2, C, **f32)
    dgamma, dbeta = torch.empty(C, **f32), torch.empty(C, **f32)
    for _ in range(calls):
        sums = ops.bn_stats(y)
        ops.bn_prepare(sums, n, gamma, beta, bn4, running=running)
    out = dict(sums=sums, bn4=bn4, run_mean=running[0], run_var=running[1])
    if hasattr(ops, "bn_lrelu_apply"):
        out["z"] = ops.bn_lrelu_apply(y, bn4[0], bn4[1])
    sums2 = ops.bn_bwd_reduce(dz, y, bn4)
    ops.bn_bwd_prepare(sums2, n, bn4, dgamma, dbeta, c10)
    dy = torch.empty_like(y)
    dbs = torch.zeros(2 * C, dtype=torch.float64, device=y.device)
    ops.bn_bwd_apply(dz, y, bn4, c10, dy, dbs)
    out.update(sums2=sums2, dgamma=dgamma, dbeta=dbeta, c10=c10, dy=dy, dbias=dbs[:C])
    return out


# ------------------------------------------------------------------------------------------------- the cases of both files
WIDTHS = (8, 16, 32, 64, 128, 256, 512, 1024)
# row counts at C = 1024 (one row per 256-lane step) -> workgroup counts of the column reduction's first stage
NBLK_AT_1024 = {1: 1, 25: 7, 29: 8, 33: 9, 225: 57, 253: 64, 257: 65, 2000: 256, 32771: 1024}
LARGE = ((32771, 1024), (65541, 512))          # past one grid pass of bn_lrelu_apply (2048 x 256 float4s); cap at rpi = 2


def _chain_cases():
    out, seen = [], set()

    def add(n, C, shift=0):
        for kind in KINDS:
            if (n, C, kind, shift) not in seen:
                seen.add((n, C, kind, shift))
                # (2, 1024): yhat = +-1 in both rows, so a column whose |gamma| is within KZ eps32 Sz of |beta| has a row on the
                # kink, and among 1024 columns most seeds have one (seed 0: 2 of 2048 elements, right at the cap on ambiguous
                # elements).  Another seed, not another cap: these two have none.
                # (257, 8) at shift 1, correlated: seed 0 has 2 of 2056 elements on the kink, again at the cap; seed 1 has none.
                seed = {"random": 5, "correlated": 3}[kind] if (n, C) == (2, 1024) else 1 if (n, C, shift) == (257, 8, 1) else 0
                out.append(Case(n, C, kind, shift, families=N1_FAMILIES if n == 1 else FAMILIES, seed=seed))
    for C in WIDTHS:
        add(257, C)
    add(257, 8, 1)                             # C = 8: a second shift, so that every family appears
    for n in (1, 2, 3):
        add(n, 8)
        add(n, 8, 1)
        add(n, 1024)
    for n in NBLK_AT_1024:
        add(n, 1024)
    add(65541, 512)
    return out


CHAIN_CASES = _chain_cases()
BF16_CASES = [Case(n, C, "correlated", families=BF16_FAMILIES, bf16=True) for C in (16, 128, 1024) for n in (3, 257, 16391)]


def is_large(case):
    return case.n * case.C > 4 * 1024 * 1024

"""tests/bn_cases.py without a GPU: (1) every column family holds the condition it is named for; (2) the float32 oracle (the
kernels' own arithmetic in numpy) stays within a quarter of every bound against the float64 reference, and within the cap on
sign-ambiguous elements, on every case tests/test_gpu_bn.py runs, figures printed; (3) the closed-form reference equals torch
autograd; (4) the bounds have teeth: seven wrong variants of the reference each exceed a bound on a family named here; (5) the
CPU stub of the BatchNorm passes (tests/cpu_ops_stub.py) is held to the same bounds."""
import pytest
import torch

import bn_cases as bc


def _ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("case", [bc.Case(257, 32), bc.Case(2000, 1024, "random"), bc.Case(257, 128, families=bc.BF16_FAMILIES, bf16=True)],
                         ids=lambda c: c.id)
def test_families_hold_their_conditions(case):
    d = case.make(0, min(case.C, 36))
    y = d.y.double()
    mean, sd = y.mean(0), y.var(0, unbiased=False).sqrt()
    seen = set()
    for c, fam in enumerate(d.families()):
        seen.add(fam)
        r = float(mean[c].abs() / sd[c]) if sd[c] > 0 else float("inf")
        g, b = float(d.gamma[c]), float(d.beta[c])
        assert abs(b) >= 0.25
        assert (-1.5 <= g <= -0.5) if fam == "neg_gamma" else (g == 0.0) if fam == "zero_gamma" else (0.5 <= g <= 1.5)
        if fam == "ordinary":
            assert r < 3
        elif fam == "offset32":
            assert r > 16
        elif fam == "offset1k":
            assert r > 512
        elif fam == "tiny":
            assert 0 < float(sd[c]) ** 2 < bc.BN_EPS / 2
        elif fam == "const":
            assert float(y[:, c].min()) == float(y[:, c].max()) == 1.5 and float(sd[c]) == 0.0
        elif fam == "big":
            assert float(y[:, c].abs().max()) > 2.0 ** 41 and r < 3
        elif fam == "small":
            assert float(y[:, c].abs().max()) < 2.0 ** -36 and float(sd[c]) ** 2 < 1e-12 * bc.BN_EPS
    assert seen == set(case.families)
    if case.bf16:
        assert torch.equal(d.y.to(torch.bfloat16).float(), d.y) and torch.equal(d.dz.to(torch.bfloat16).float(), d.dz)
    # dgamma / n and dbeta / n: O(1) at the correlated gradient, O(n^-1/2) at the random one (on the columns whose yhat is O(1);
    # a column that sits on the LeakyReLU's 0.01 branch scales both down, hence the median)
    ref = bc.reference(d)
    live = [c for c, f in enumerate(d.families()) if f in ("ordinary", "offset32", "offset1k", "big", "neg_gamma")]
    db, dg = (ref["dbeta"].abs() / case.n)[live].median(), (ref["dgamma"].abs() / case.n)[live].median()
    assert (float(db) > 0.1 and float(dg) > 0.1) if case.kind == "correlated" else (float(db) < 0.1 and float(dg) < 0.1)


def test_c8_takes_two_shifts_to_show_every_family():
    fams = {c.family(k) for c in bc.CHAIN_CASES if (c.n, c.C) == (257, 8) for k in range(8)}
    assert fams == set(bc.FAMILIES)
    fams = {c.family(k) for c in bc.CHAIN_CASES if (c.n, c.C) == (1, 8) for k in range(8)}
    assert fams == set(bc.N1_FAMILIES)


@pytest.mark.parametrize("case", bc.CHAIN_CASES + bc.BF16_CASES, ids=_ids(bc.CHAIN_CASES + bc.BF16_CASES))
def test_float32_oracle_is_within_a_quarter_of_every_bound(case):
    amb, fig = 0.0, {}
    for lo, hi in case.blocks(128):
        d = case.make(lo, hi)
        ref = bc.reference(d)
        sc = bc.scales(d, ref)
        got = bc.oracle32(d)
        rat = bc.ratios(got, d, ref, sc)
        amb += sc["amb_share"] * (hi - lo) / case.C
        for q, v in bc.worst(rat).items():
            fig[q] = max(fig.get(q, 0.0), v)
        assert not bc.misses(rat, d.families(), part=0.25), bc.misses(rat, d.families(), part=0.25)
        assert bc.sum_misses(got["sums"][:hi - lo], d.y) <= 1e-12 and bc.sum_misses(got["sums"][hi - lo:], d.y.double() ** 2) <= 1e-12
    print("oracle32", case.id, "ambiguous %.1e" % amb, {q: round(v, 2) for q, v in fig.items()})
    assert amb <= bc.AMB_SHARE


@pytest.mark.parametrize("case", [bc.Case(n, C, kind, s) for n, C, s in ((2, 8, 0), (2, 8, 1), (3, 8, 0), (3, 8, 1), (257, 8, 1), (257, 32, 0))
                                  for kind in bc.KINDS], ids=lambda c: c.id)
def test_closed_form_equals_autograd(case):
    d = case.make()
    ref, auto = bc.reference(d, calls=3), bc.reference_autograd(d, calls=3)
    rat = bc.ratios(auto, d, ref)
    # two float64 evaluations of one function: 1e-4 eps32 = 6e-12 of each scale (float64 rounding is 1e-16 of it, times the
    # condition of c1 y + c0 at |mean| / sigma = 1024 and a few hundred terms)
    assert all(float(r.max()) <= 1e-4 for r in rat.values()), bc.worst(rat)


MUTANT_TRIPS = {                                                    # mutant -> (quantity, family) that must exceed its bound
    "unbiased_forward": ("z", "ordinary"),
    "no_eps": ("z", "tiny"),
    "c0_plus": ("dy", "offset1k"),
    "lrelu_from_y": ("dy", "neg_gamma"),
    "abs_gamma": ("z", "neg_gamma"),
    "running_biased": ("run_var", "ordinary"),
    "momentum_swapped": ("run_mean", "ordinary"),
}


def test_every_mutant_is_listed():
    assert set(MUTANT_TRIPS) == set(bc.MUTANTS)


@pytest.mark.parametrize("mutant", bc.MUTANTS)
def test_bounds_reject_a_wrong_reference(mutant):
    case = bc.Case(257, 32, "correlated")
    d = case.make()
    ref = bc.reference(d)
    assert not bc.misses(bc.ratios(ref, d, ref), d.families())
    bad = bc.misses(bc.ratios(bc.reference(d, mutant=mutant), d, ref), d.families())
    q, fam = MUTANT_TRIPS[mutant]
    assert any(b[0] == q and b[1] == fam for b in bad), (mutant, bad)
    if q == "dy":                                                   # the sharp dY bound sees it too
        assert any(b[0] == "dyt" and b[1] == fam for b in bad), (mutant, bad)


@pytest.mark.parametrize("case", [bc.Case(257, 32, "correlated"), bc.Case(3, 8, "random", 1)], ids=lambda c: c.id)
def test_cpu_stub_chain_is_within_the_bounds(case):
    import cpu_ops_stub as stub
    d = case.make()
    ref = bc.reference(d, calls=3)
    run = [t.clone() for t in d.running_start()]
    got = bc.run_chain(stub, d.y, d.dz, d.gamma, d.beta, (run[0], run[1]), calls=3)
    rat = bc.ratios(got, d, ref)
    assert "z" not in rat and "dy" in rat                            # the stub has no bn_lrelu_apply
    assert not bc.misses(rat, d.families(), calls=3), bc.misses(rat, d.families(), calls=3)
    assert bc.sum_misses(got["sums"][:case.C], d.y) <= 1e-12
    assert bc.sum_misses(got["dbias"], got["dy"]) <= 1e-12

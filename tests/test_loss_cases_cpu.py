"""tests/loss_cases.py without a GPU: (1) the float32 oracle through the comparison rule against the float64 oracle for every
case tests/test_gpu_losses.py runs -- the reference alone stays below every cap and floor, with the figures printed; (2) the
rule rejects a gradient whose rows past the 2,048-block kernels' first trip are shifted by one row, and one whose elements past
524,288 are missing; (3) the numpy float64 restatements (sigma_c through the one-pass bilateral filter, face normals, vertex
update) against the vectors captured from the reference (tests/golden); (4) what the exact-tie and `bnfloop = 0` cases expect
holds for the oracle in float32 and in float64."""
import os

import numpy as np
import pytest
import torch

import loss_cases as lc

NAMES = ["ico2", "grid4", "cube3", "grid7x5"]


@pytest.mark.parametrize("run", lc.ENGINE_RUNS, ids=lc.run_id)
def test_float32_oracle_is_within_the_rule(run):
    name, loop, k, gate4 = run
    c = lc.case(name)
    r32, r64 = c.ref(torch.float32, loop, k, gate4), c.ref(torch.float64, loop, k, gate4)
    fig = lc.check_run(r32.scalars, r32.dpos, r32.dnorm, c, loop, k, gate4, lc.run_id(run))
    # the condition sits well above the reference's own share of knife-edge rows: a cap, not a measurement
    assert all(f.get("off", 0.0) <= lc.OFF_SHARE / 4 for f in fig.values()), fig
    assert np.isfinite(r64.scalars).all() and np.isfinite(r64.dpos).all() and np.isfinite(r64.dnorm).all()


def test_blocks_merge_a_short_tail():
    assert lc.blocks(1) == [(0, 1)] and lc.blocks(65536) == [(0, 65536)]
    assert lc.blocks(65536 + 16383) == [(0, 65536 + 16383)]
    assert lc.blocks(65536 + 16384) == [(0, 65536), (65536, 65536 + 16384)]
    assert lc.blocks(526350)[-1] == (7 * 65536, 526350) and len(lc.blocks(526350)) == 8


@pytest.mark.parametrize("which", ["dpos", "dnorm"])
def test_rule_rejects_rows_shifted_past_the_first_trip(which):
    """A kernel whose second trip starts one row off: rows >= 524,288 of the float64 gradient rolled by one."""
    c = lc.case("x524k")
    r64, r32 = c.ref(torch.float64, 2), c.ref(torch.float32, 2)
    g = np.array(getattr(r64, which))
    assert not lc.gradient_misses(g, getattr(r64, which), getattr(r32, which), lc.FLOOR, "unplanted")[0]
    g[524288:] = np.roll(g[524288:], 1, axis=0)
    miss, _ = lc.gradient_misses(g, getattr(r64, which), getattr(r32, which), lc.FLOOR_BNF, "rolled " + which)
    assert any("are off" in m for m in miss), miss


def test_rule_rejects_elements_missing_past_the_first_trip():
    """bnf_bwd_init / face_bwd index 3F elements: [524,288, 3F) never written."""
    c = lc.case("x524k")
    r64, r32 = c.ref(torch.float64, 2), c.ref(torch.float32, 2)
    g = np.array(r64.dnorm)
    g.reshape(-1)[524288:] = 0.0
    miss, _ = lc.gradient_misses(g, r64.dnorm, r32.dnorm, lc.FLOOR_BNF, "zeroed dnorm")
    assert any("are off" in m for m in miss), miss
    g = np.array(r64.dnorm)
    g[-1, 2] = np.nan                                                     # one bad element in a million rows
    assert any("non-finite" in m for m in lc.gradient_misses(g, r64.dnorm, r32.dnorm, lc.FLOOR_BNF, "nan")[0])


def test_scalar_rule():
    ref = np.array([1.0, 2.0, 3.0, 0.0, 5.0, 6.0])
    assert not lc.scalar_misses(ref * (1 + np.array([5e-10, 5e-6, 5e-10, 0, 5e-6, 5e-6])), ref)
    assert len(lc.scalar_misses(ref * (1 + 2e-9), ref)) == 2                # L1 and L3 are float64 sums
    assert len(lc.scalar_misses(ref + np.array([0, 0, 0, 1e-30, 0, 0]), ref)) == 1   # an exact zero is expected exactly


# ------------------------------------------------------------------------------------ numpy restatements vs the reference's vectors
@pytest.mark.parametrize("name", NAMES)
def test_numpy_references_match_reference_golden(golden_dir, name):
    gl = np.load(os.path.join(golden_dir, "loss_%s.npz" % name))
    gm = np.load(os.path.join(golden_dir, "mesh_%s.npz" % name))
    pos, nrm, faces, f2f = gl["pos"], gl["norm"], gm["faces"], gm["f2f"]
    # sigma_c enters the reference's outputs through the filter weights only: one and five passes of the numpy filter built on
    # sigma_c_np reproduce the reference's filtered normals and L4
    for loop in (1, 5):
        new_fn, l4 = lc.bnf_filter_np(pos, nrm, faces, f2f, loop)
        np.testing.assert_allclose(new_fn, gl["bnf%d_newfn" % loop], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(l4, gl["bnf%d" % loop], rtol=1e-6, atol=1e-7)
    # ... and the weights do depend on it at this resolution
    sc = lc.sigma_c_np(pos, faces, f2f)
    assert 0.1 < sc < 10.0
    fn, fa = lc.face_normals_np(pos, faces)
    np.testing.assert_allclose(fn, gl["cfn_fn"], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(fa, gl["cfn_fa"], rtol=1e-13)
    assert lc.mad_np(fn, gm["fn"]) == pytest.approx(float(gl["mad_pos"]), rel=1e-12)
    for loop in (1, 3):
        np.testing.assert_allclose(lc.vertex_update_np(pos, nrm, faces, loop), gl["vertex_updating_%d" % loop],
                                   rtol=1e-5, atol=2e-6)


def test_sigma_c_of_one_face_is_the_epsilon():
    c = lc.case("tri1")
    assert (c.mesh.f2f == -1).all()
    assert lc.sigma_c_np(c.pos, c.mesh.faces, c.mesh.f2f) == pytest.approx(1.0e-6, rel=1e-12)


# ------------------------------------------------------------------------------------ exact expectations hold for the oracle
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_oracle_at_exact_ties(dtype):
    c = lc.case("ties")
    assert np.array_equal(c.pos.astype(np.float64), c.mesh.vs) and np.array_equal(c.norm.astype(np.float64), c.mesh.fn)
    l1, dpos, _ = lc.oracle_part(c, dtype, 0)
    assert l1 == 1.0e-3 and not dpos.any()                                  # sqrt(0 + 1e-6); (p - real) / (V L1) = 0
    l3, _, dnorm = lc.oracle_part(c, dtype, 2)
    assert l3 == 0.0 and not dnorm.any()                                    # sign(0) = 0
    l5, dpos, dnorm = lc.oracle_part(c, dtype, 4)
    assert l5 == 0.0 and not dpos.any() and not dnorm.any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_oracle_without_filter_passes(dtype):
    l4, dpos, dnorm = lc.oracle_part(lc.case("loops"), dtype, 3, loop=0)
    assert l4 == 0.0 and not dpos.any() and not dnorm.any()


def test_degenerate_cases_are_what_they_say():
    for name, n in (("collapse2", 2), ("collapse3", 3)):
        c = lc.case(name)
        z = lc.zero_area_faces(c)
        assert len(z) == (2 if n == 2 else 4)                                # an interior edge's two faces; a face and its three neighbours
        fn, fa = lc.face_normals_np(c.pos, c.mesh.faces)
        assert not fn[z].any() and not fa[z].any() and np.isfinite(fn).all()  # 0 / 1e-24
    assert 5.0 < lc.weight_exponents(lc.case("gap200")).max() < 22.0          # small weights; sigma_c grows with the gap
    e = lc.weight_exponents(lc.case("spike200"))
    assert (e > 104.0).sum() >= 6 and np.exp(np.float32(-e.max())) == 0.0    # expf underflows past 103.97

"""csrc/loss.hip and csrc/eval.hip against independent float64 references (tests/loss_cases.py) where the golden meshes (a few
hundred faces) cannot reach: past the first trip of every grid-stride loop (65,536 elements for the 256-block reducers, 524,288
for the 2,048-block element-wise kernels), one- and two-face meshes, every parity of `bnfloop` (the G0 / scratch ping-pong of
the BNF backward) and `bnfloop = 0`, exact ties of the sign arguments, zero-area predicted faces, weights that underflow expf,
meshes that are not unit scale, and MAD at the clamp.  The comparison rule and the cases are described in loss_cases.py; every
figure is printed (pytest -s) before anything is asserted.

MEASURED on an MI355X (HIP against float64; in brackets the float32 oracle against float64 on the same host).  "off" is the
worst 65,536-row block's share of rows with a component further than 1e-3 max|ref| from float64 (cap 1e-3), "rel" the rel-L2
over the other rows (bound: max(floor, 4 x the float32 oracle's)).  Scalars: L1 / L3 agree to <= 1e-15, L2 / L4 / L5 / total /
sigma_c to <= 1.0e-7 except offset1000 (L2 8.1e-6 -- the float32 oracle: 8.0e-6 --, L5 1.3e-6, sigma_c and total 2.3e-6: float32
1-ring means and centroids at |p| = 1000; the bound is 1e-5).

  run                 dpos off              dpos rel               dnorm off             dnorm rel
  e65k loop 1         9.1e-5 (9.1e-5)       5.00e-6 (5.00e-6)      1.5e-5 (1.5e-5)       1.21e-6 (1.21e-6)
  e65k loop 4         9.1e-5 (9.1e-5)       5.00e-6 (5.00e-6)      1.5e-5 (1.5e-5)       1.93e-6 (1.93e-6)
  x65k loop 5         0      (0)            6.35e-6 (6.35e-6)      0      (0)            2.88e-6 (2.91e-6)
  e524k loop 2        1.2e-4 (1.2e-4)       1.27e-5 (1.27e-5)      1.7e-4 (1.5e-4)       1.80e-5 (2.38e-5)
  x524k loop 2        1.7e-4 (1.7e-4)       1.86e-5 (1.86e-5)      1.7e-4 (1.7e-4)       2.74e-5 (2.74e-5)
  x524k loop 2, k2=0  1.7e-4 (1.7e-4)       5.2e-8  (5.5e-8)       1.7e-4 (1.7e-4)       2.71e-5 (2.71e-5)
  x524k loop 2, gate0 1.7e-4 (1.7e-4)       1.86e-5 (1.86e-5)      4.6e-5 (4.6e-5)       6.04e-6 (6.04e-6)
  loops loop 0 .. 5   0      (0)            2.3e-7  (2.4e-7)       0      (0)            <= 3.1e-7 (<= 2.0e-7)
  tri1, tri2 loop 1   0      (0)            <= 5.7e-8              0      (0)            <= 5.9e-7 (<= 3.7e-7)
  offset1000          0      (0)            3.99e-5 (3.99e-5)      0      (0)            7.76e-6 (7.75e-6)
  the other inputs    0      (0)            <= 2.4e-7              0      (0)            <= 2.0e-7
The autograd entry points give the same figures.  tri2 at loop 2: L4 1.49e-8 against 1.10e-8 in float64 (the float32 oracle:
1.49e-8), the filter's part of dnorm 0.44 at most (cap 6.9): see loss_cases.filter_returns_input.
Evaluation kernels at 524,288 / 1,049,800 faces: face normals within 1.4e-7 of float64 (allowed 2e-6 + 1e-5 |ref|); MAD equal to
numpy on the same normals to 1e-16 rel and within 4e-9 degrees of MAD on float64 normals; vertex_updating: 0.04 of the
allowance at most after one sweep and after three.  MAD at the clamp: 1.9e-16 rel.
"""
import numpy as np
import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu

AUTOGRAD_CASES = ["e65k", "x65k", "tri1", "tri2", "loops"] + list(lc.DEGENERATE)
EVAL_CASES = ["e524k", "x524k"]
EVAL_RTOL, EVAL_ATOL = 1.0e-5, 2.0e-6           # test_vertex_updating_matches_reference_golden's; atol x the mean edge for positions


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _poison(scratch):
    """NaN into every float32 buffer the kernels are to write: an element a kernel skips is seen, whatever the allocator handed out."""
    for v in vars(scratch).values():
        if isinstance(v, torch.Tensor) and v.dtype == torch.float32:
            v.fill_(float("nan"))
    scratch.lossbuf.fill_(float("nan"))
    scratch.partials.fill_(float("nan"))


def _engine(case, dev, loop, k=lc.DEFAULT_K, gate4=1.0):
    from dual_dmp_amd import loss as L
    eng = L.LossEngine(case.mesh, dev, bnfloop=loop, k=k)
    _poison(eng.s)
    buf, dpos, dnorm = eng.forward_backward(_dev(case.pos, dev), _dev(case.norm, dev), gate4)
    torch.cuda.synchronize()
    return eng, buf.cpu().numpy(), dpos.cpu().numpy(), dnorm.cpu().numpy()


def _sigma_misses(buf, case, what):
    ref = lc.sigma_c_np(case.pos, case.mesh.faces, case.mesh.f2f)
    return lc.scalar_misses([buf[11]], [ref], what, ("sigma_c",), (1e-5,))


# ------------------------------------------------------------------------------------ the fused engine
@pytest.mark.parametrize("run", lc.ENGINE_RUNS, ids=lc.run_id)
def test_engine_matches_float64_oracle(dev, run):
    """LossEngine.forward_backward: lossbuf[0:6], lossbuf[11], dpos, dnorm."""
    name, loop, k, gate4 = run
    case = lc.case(name)
    _, buf, dpos, dnorm = _engine(case, dev, loop, k, gate4)
    miss, _ = lc.run_misses(buf[:6], dpos, dnorm, case, loop, k, gate4, lc.run_id(run))
    miss += _sigma_misses(buf, case, lc.run_id(run))
    # the gradient coefficients the backward kernels read
    c = np.array(k) / np.array([case.V * buf[0], case.V * buf[1], case.F, case.F, case.V]) * np.array([1, 1, 1, gate4, 1])
    assert np.allclose(buf[6:11], c, rtol=1e-12, atol=0.0), (buf[6:11], c)
    assert not miss, miss


def test_no_filter_pass_means_no_filter_gradient(dev):
    """bnfloop = 0: L4 is exactly 0 and G0 contributes exactly nothing -- dnorm is, bit for bit, that of the closed gate."""
    case = lc.case("loops")
    eng, buf, _, dnorm = _engine(case, dev, 0, gate4=1.0)
    assert buf[3] == 0.0
    assert not eng.s.G0.cpu().numpy().any()
    _, buf0, _, dnorm0 = _engine(case, dev, 0, gate4=0.0)
    assert buf0[3] == 0.0 and np.array_equal(dnorm, dnorm0) and buf[5] == buf0[5]


# ------------------------------------------------------------------------------------ the five autograd entry points
def _autograd(case, dev, loop, k=lc.DEFAULT_K):
    from dual_dmp_amd import loss as L
    m = case.mesh
    pos, nrm = _dev(case.pos, dev).requires_grad_(True), _dev(case.norm, dev).requires_grad_(True)
    t = [L.pos_rec_loss(pos, m.vs), L.mesh_laplacian_loss(pos, m), L.norm_rec_loss(nrm, m.fn),
         L.fn_bnf_loss(pos, nrm, m, loop=loop)[0], L.pos_norm_loss(pos, nrm, m)]
    assert [x.dtype for x in t] == [torch.float64, torch.float32, torch.float64, torch.float32, torch.float32]
    total = k[0] * t[0] + k[1] * t[1] + k[2] * t[2] + k[3] * t[3] + k[4] * t[4]
    gp, gn = torch.autograd.grad(total, [pos, nrm])
    return np.array([x.item() for x in t] + [total.item()]), gp.cpu().numpy(), gn.cpu().numpy()


@pytest.mark.parametrize("run", [(n, l) for n in AUTOGRAD_CASES for l in lc.loops_of(n)], ids=lambda r: "%s-loop%d" % r)
def test_autograd_entry_points_match_float64_oracle(dev, run):
    """pos_rec_loss ... pos_norm_loss (their own scratch per call, torch reductions of the partial sums), weighted as
    main.py:106 and differentiated by autograd."""
    name, loop = run
    case = lc.case(name)
    scalars, gp, gn = _autograd(case, dev, loop)
    lc.check_run(scalars, gp, gn, case, loop, what="autograd %s loop %d" % run)


# ------------------------------------------------------------------------------------ exact ties
def test_exact_ties_give_exact_zeros(dev):
    """real == pred bit for bit on a dyadic planar patch, every normal (0, 0, 1): sign(0) must be 0 as autograd's abs has it."""
    from dual_dmp_amd import loss as L
    case = lc.case("ties")
    m = case.mesh

    def leaves():
        return _dev(case.pos, dev).requires_grad_(True), _dev(case.norm, dev).requires_grad_(True)

    pos, nrm = leaves()
    l1 = L.pos_rec_loss(pos, m.vs)
    assert l1.item() == 1.0e-3
    assert not torch.autograd.grad(l1, pos)[0].cpu().numpy().any()
    l3 = L.norm_rec_loss(nrm, m.fn)
    assert l3.item() == 0.0
    assert not torch.autograd.grad(l3, nrm)[0].cpu().numpy().any()
    l5 = L.pos_norm_loss(pos, nrm, m)
    assert l5.item() == 0.0
    gp, gn = torch.autograd.grad(l5, [pos, nrm])
    assert not gp.cpu().numpy().any() and not gn.cpu().numpy().any()
    # the fused engine with the filter out of the total (closed gate, or k4 = 0: the filtered normal sits within an ulp of its
    # input, so L4 and the sign of n_last - n0 are rounding noise in any float32 arithmetic): only the Laplacian term is left
    # in dpos, nothing in dnorm
    l2, d2, _ = lc.oracle_part(case, torch.float64, 1)
    for k, gate4 in ((lc.DEFAULT_K, 0.0), ((3.0, 4.0, 4.0, 0.0, 1.0), 1.0)):
        _, buf, dpos, dnorm = _engine(case, dev, 1, k, gate4)
        assert buf[0] == 1.0e-3 and buf[2] == 0.0 and buf[4] == 0.0
        assert not dnorm.any()
        assert abs(buf[1] - l2) <= 1e-5 * l2 and abs(buf[5] - (k[0] * 1.0e-3 + k[1] * l2)) <= 1e-5 * buf[5]
        lc.check_gradient(dpos, k[1] * d2, k[1] * lc.oracle_part(case, torch.float32, 1)[1], lc.FLOOR, "ties dpos")


# ------------------------------------------------------------------------------------ evaluation kernels
def _face_normals(pos, faces, dev):
    """ddmp_face_normals_f32 with its optional area output (Evaluator.face_normals passes none)."""
    from dual_dmp_amd import _lib
    from dual_dmp_amd.ops import _p, _stream
    F = len(faces)
    fn = torch.full((F, 3), float("nan"), dtype=torch.float32, device=dev)
    fa = torch.full((F,), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ddmp_face_normals_f32(F, _p(pos), _p(_dev(faces.astype(np.int32), dev)), _p(fn), _p(fa), _stream()),
               "ddmp_face_normals_f32")
    return fn.cpu().numpy(), fa.cpu().numpy()


def _close(got, ref, atol, what):
    """np.testing.assert_allclose's condition with the figures printed first."""
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= atol + EVAL_RTOL * np.abs(ref))
    print("%-30s max |err| %.3e  largest err / (atol + rtol |ref|) %.2f  components outside %d of %d"
          % (what, np.nanmax(err), np.nanmax(err / (atol + EVAL_RTOL * np.abs(ref))), int(bad.sum()), bad.size))
    assert np.isfinite(got).all(), what
    assert not bad.any(), (what, int(bad.sum()), float(err.max()))


@pytest.mark.parametrize("name", ["collapse2", "collapse3"])
def test_zero_area_predicted_faces(dev, name):
    """0 / 1e-24 in face_normals, the 1e-12 under the area's square root in the losses: exact zeros, everything finite."""
    from dual_dmp_amd import models
    from dual_dmp_amd.evaluate import Evaluator
    case = lc.case(name)
    zero = lc.zero_area_faces(case)
    pos = _dev(case.pos, dev)
    fn, fa = _face_normals(pos, case.mesh.faces, dev)
    assert not fn[zero].any() and not fa[zero].any()
    ref_fn, ref_fa = lc.face_normals_np(case.pos, case.mesh.faces)
    _close(fn, ref_fn, EVAL_ATOL, name + " face normals")
    _close(fa, ref_fa, EVAL_ATOL * lc.mean_edge(case.mesh) ** 2, name + " face areas")
    assert np.array_equal(Evaluator(case.mesh, case.mesh.fn, dev).face_normals(pos).cpu().numpy(), fn)
    out = models.vertex_updating(pos, _dev(case.norm, dev), case.mesh, loop=1).cpu().numpy()
    _close(out, lc.vertex_update_np(case.pos, case.norm, case.mesh.faces, 1), EVAL_ATOL * lc.mean_edge(case.mesh),
           name + " vertex_updating")
    # (losses and gradients of these inputs: ENGINE_RUNS / AUTOGRAD_CASES above)


@pytest.mark.parametrize("name", EVAL_CASES)
def test_face_normals_and_mad_past_the_first_trip(dev, name):
    from dual_dmp_amd.evaluate import Evaluator
    case = lc.case(name)
    ev = Evaluator(case.mesh, case.mesh.fn, dev)
    ev.fn.fill_(float("nan"))
    pos = _dev(case.pos, dev)
    fn = ev.face_normals(pos).cpu().numpy()
    ref_fn, _ = lc.face_normals_np(case.pos, case.mesh.faces)
    mad = ev.mad(pos)
    mad_own, mad_ref = lc.mad_np(fn, case.mesh.fn), lc.mad_np(ref_fn, case.mesh.fn)
    print("%-30s mad %.12f  numpy on the kernel's normals %.12f  on float64 normals %.12f" % (name, mad, mad_own, mad_ref))
    # the reduction itself: float64 on the very normals it read; and the pair of kernels to the golden test's 1e-3 degrees
    miss = [] if abs(mad - mad_own) <= 1e-9 * mad_own and abs(mad - mad_ref) < 1e-3 else ["mad %r %r %r" % (mad, mad_own, mad_ref)]
    # whole blocks of faces first (a stride error), then every component
    far = np.abs(fn - ref_fn).max(1) > 1e-3
    assert far.sum() <= 1e-3 * 16384 and np.isfinite(fn).all(), (int(far.sum()), np.flatnonzero(far)[:8])
    assert not miss, miss
    _close(fn, ref_fn, EVAL_ATOL, name + " face normals")


@pytest.mark.parametrize("loop", [1, 3])
@pytest.mark.parametrize("name", EVAL_CASES)
def test_vertex_updating_past_the_first_trip(dev, name, loop):
    """models.vertex_updating against float64 numpy, rtol 1e-5 and atol 2e-6 x the mean edge.

    What it took at |p| up to 726.  With the centroid rounded to float32 first, ONE sweep missed at 12,011 (e524k) / 68,416
    (x524k) components: the per-corner offsets are formed from edge vectors now.  With the positions stored as one float32
    between sweeps, THREE sweeps missed at 8,669 / 57,264 components (4.2 / 8.2 times the allowance): x and y in the hundreds
    come back rounded to 6e-5 and the next sweep's (c_f - p_v) . n_f carries that into the small components, where 2.3e-6 is
    allowed; models.vertex_updating keeps them as a float32 pair now (ddmp_vertex_update_pair_f32).  The single-float entry
    point, ddmp_vertex_update_f32, is held to the same bound for the one sweep it can meet it for."""
    from dual_dmp_amd import models
    case = lc.case(name)
    edge = lc.mean_edge(case.mesh)
    out = models.vertex_updating(_dev(case.pos, dev), _dev(case.norm, dev), case.mesh, loop=loop).cpu().numpy()
    ref = lc.vertex_update_np(case.pos, case.norm, case.mesh.faces, loop)
    # whole blocks of vertices first: a vertex a sweep skipped keeps its 0.3-edge noise along the normal
    far = np.abs(out - ref).max(1) > 1e-2
    assert not far.any() and np.isfinite(out).all(), (int(far.sum()), np.flatnonzero(far)[:8])
    _close(out, ref, EVAL_ATOL * edge, "%s vertex_updating loop %d" % (name, loop))
    if loop == 1:
        _close(_vertex_update_single(case, dev, 1), ref, EVAL_ATOL * edge, "%s ddmp_vertex_update_f32 loop 1" % name)


def _vertex_update_single(case, dev, loop):
    """ddmp_vertex_update_f32: the entry point with [F,3] floats of scratch only."""
    from dual_dmp_amd import _lib
    from dual_dmp_amd.loss import tables_for
    from dual_dmp_amd.ops import _p, _stream
    tb = tables_for(case.mesh, dev)
    pos, nrm = _dev(case.pos, dev), _dev(case.norm, dev)
    scratch = torch.full((tb.F, 3), float("nan"), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ddmp_vertex_update_f32(tb.V, tb.F, _p(pos), _p(nrm), _p(tb.faces), _p(tb.vf_ptr), _p(tb.vf_corner),
                                                 _p(scratch), loop, _stream()), "ddmp_vertex_update_f32")
    return pos.cpu().numpy()


# ------------------------------------------------------------------------------------ MAD at the clamp
F_MAD = 131584                                   # the second trip of the 256-block reduction


def _mad(n1, n2, dev):
    from dual_dmp_amd import _lib
    from dual_dmp_amd.ops import Workspace, _p, _stream
    L = _lib.lib()
    a, b = _dev(n1.astype(np.float32), dev), _dev(n2.astype(np.float64), dev)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    ws = Workspace.get(L.ddmp_mad_workspace_bytes(), dev)
    _lib.check(L.ddmp_mad_f64(len(n1), _p(a), _p(b), _p(out), _p(ws), ws.numel(), _stream()), "ddmp_mad_f64")
    return float(out.item())


def test_mad_at_the_clamp(dev):
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    n1 = axes[np.arange(F_MAD) % 6]
    assert _mad(n1, n1, dev) == 0.0                                    # inner == 1 exactly
    assert _mad(n1, -n1, dev) == 180.0                                 # inner == -1 exactly
    rng = np.random.default_rng(17)
    r = rng.standard_normal((F_MAD, 3)).astype(np.float32)
    r = (r / np.sqrt((r * r).sum(1, dtype=np.float32))[:, None]).astype(np.float32)
    inner = (r.astype(np.float64) ** 2).sum(1)
    assert (inner > 1.0).sum() > F_MAD // 10 and (inner < 1.0).sum() > F_MAD // 10      # straddles the clamp
    got, ref = _mad(r, r.astype(np.float64), dev), lc.mad_np(r, r.astype(np.float64))
    print("mad at the clamp: %.17g  numpy %.17g  rel %.2e" % (got, ref, abs(got - ref) / ref))
    assert np.isfinite(got) and abs(got - ref) <= 1e-9 * ref

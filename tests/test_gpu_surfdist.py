"""Point-to-surface distance on the MI355X (csrc/surfdist.hip through evaluate.SurfaceDistance / hausdorff) against a
float64 brute force (tests/surfdist_ref.py).

Tolerances.  The kernel reads float32 coordinates; the brute force gets the same float32 values widened to float64, so only
the kernel's arithmetic is measured.  Every difference with the query point is formed against one vertex (one rounding:
<= 2^-24 |coord|), the dot products and the closest point on the region add a few roundings of the same size, and the
distance is a square root of a sum of squares of those differences.  That bounds the per-sample error by a small multiple
of 2^-24 (max|coord| + d); the test allows 2^-20 (max|coord| + d), i.e. 16 such roundings.  Mean and rms are float64 sums
of the per-sample values, so their relative error is that of the samples averaged: <= 1e-5 relative is asked.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from surfdist_ref import brute_force

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
TOL = 2.0 ** -20


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _queries(vs, faces, seed=0):
    """vertices (on the surface), jittered vertices, random points in and around the bbox, far points, duplicates."""
    rng = np.random.default_rng(seed)
    vs = np.asarray(vs, dtype=np.float64)
    lo, hi = vs.min(0), vs.max(0)
    ext = float(np.linalg.norm(hi - lo))
    cen = vs[faces].mean(1)
    near = vs[rng.integers(0, len(vs), 300)] + rng.normal(scale=0.02 * ext, size=(300, 3))
    box = lo - 0.25 * (hi - lo) + rng.random((300, 3)) * 1.5 * (hi - lo)
    far = 0.5 * (lo + hi) + rng.normal(size=(16, 3)) * 10.0 * ext
    pts = np.concatenate([vs, cen[:200], near, box, far])
    return np.concatenate([pts, pts[rng.integers(0, len(pts), 50)]])


def _check(vs, faces, pts, max_dist=0.0, sort=None):
    from dual_dmp_amd.evaluate import SurfaceDistance
    sd = SurfaceDistance(vs, faces, DEV)
    r = sd.query(pts, max_dist=max_dist, per_sample=True, sort=sort)
    d = r["dist"].cpu().numpy().astype(np.float64)
    ref = brute_force(_f32(pts), _f32(vs), faces)
    M = max(np.abs(_f32(pts)).max(), np.abs(_f32(vs)).max())
    if max_dist > 0:
        keep = ref <= max_dist
        assert np.array_equal(np.isinf(d), ~keep)
        assert r["n_dropped"] == int((~keep).sum()) and r["n"] == int(keep.sum())
        d, ref = d[keep], ref[keep]
    err = np.abs(d - ref)
    bound = TOL * (M + ref)
    assert (err <= bound).all(), (err.max(), np.argmax(err / bound), float((err / bound).max()))
    if len(ref):
        assert abs(r["mean"] - ref.mean()) <= 1e-5 * ref.mean() + 1e-12
        assert abs(r["rms"] - math.sqrt((ref ** 2).mean())) <= 1e-5 * math.sqrt((ref ** 2).mean()) + 1e-12
        assert r["min"] == d.min() and r["max"] == d.max()
    return r, d, ref


def _soup(n=2000, seed=1):
    rng = np.random.default_rng(seed)
    vs = rng.random((3 * n, 3))
    return vs, np.arange(3 * n).reshape(n, 3)


def _hub_torus():
    from dual_dmp_amd import synth
    vs, f = synth.torus(24, 16)
    f = synth.flip_edges(vs, f, rounds=6, seed=3)
    return vs, synth.add_hub(vs, f, vertex=0, valence=24)


def _degenerate():
    from dual_dmp_amd import synth
    vs, f = synth.icosphere(2)
    n = len(vs)
    extra_v = np.array([[2.0, 0.0, 0.0], [2.5, 0.5, 0.0], [3.0, 1.0, 0.0], [2.0, 2.0, 2.0]])   # three collinear, one lone
    vs = np.concatenate([vs, extra_v])
    extra_f = np.array([[n, n + 1, n + 2], [n + 3, n + 3, n + 3], [n, n, n + 3], [n + 2, n + 1, n], [0, 0, 1]])
    return vs, np.concatenate([f, extra_f])


def _meshes():
    from dual_dmp_amd import synth
    return {
        "soup": _soup(),
        "icosphere3": synth.icosphere(3),
        "hub_torus": _hub_torus(),
        "open_grid": synth.open_grid(30, 20),
        "cube_cad": synth.cube_cad(10),
        "permuted": synth.permute_vertices(*synth.icosphere(3), seed=5),
        "degenerate": _degenerate(),
    }


@pytest.mark.parametrize("name", ["soup", "icosphere3", "hub_torus", "open_grid", "cube_cad", "permuted", "degenerate"])
@pytest.mark.parametrize("sort", [False, True])
def test_kernel_matches_brute_force(name, sort):
    vs, f = _meshes()[name]
    _check(vs, f, _queries(vs, f), sort=sort)


def test_mesh_against_itself_is_zero():
    from dual_dmp_amd import synth
    from dual_dmp_amd.evaluate import hausdorff
    vs, f = synth.icosphere(3)
    r = hausdorff((vs, f), (vs, f), DEV)
    assert r["hd"] == 0.0 and r["ab"]["max"] == 0.0 and r["ba"]["max"] == 0.0 and r["ab"]["n"] == len(vs)


def test_shifted_plane_gives_the_shift():
    from dual_dmp_amd import synth
    from dual_dmp_amd.evaluate import SurfaceDistance
    vs, f = synth.open_grid(40, 30)
    vs = vs.copy()
    vs[:, 2] = 0.0
    t = 0.3125
    up = vs + np.array([0.0, 0.0, t])
    for a, b in ((vs, up), (up, vs)):
        d = SurfaceDistance(b, f, DEV).query(a, per_sample=True)["dist"].cpu().numpy()
        M = np.abs(a).max()
        assert np.abs(d - t).max() <= TOL * (M + t)


def test_concentric_icospheres_within_analytic_bounds():
    from dual_dmp_amd import synth
    from dual_dmp_amd.evaluate import SurfaceDistance
    vs, f = synth.icosphere(3, modulate=0.0)
    a, b, c = vs[f[:, 0]], vs[f[:, 1]], vs[f[:, 2]]
    n = np.cross(b - a, c - a)
    r_in = float(np.min(np.abs((n * a).sum(1)) / np.linalg.norm(n, axis=1)))   # inscribed radius of the polyhedron
    s = 1.5
    eps = TOL * 2 * s
    d = SurfaceDistance(vs, f, DEV).query(s * vs, per_sample=True)["dist"].cpu().numpy()
    assert d.min() >= s - 1.0 - eps and d.max() <= s - r_in + eps
    d = SurfaceDistance(s * vs, f, DEV).query(vs, per_sample=True)["dist"].cpu().numpy()
    assert d.min() >= s * r_in - 1.0 - eps and d.max() <= s - 1.0 + eps


def test_max_dist_drops_and_truncates_like_brute_force():
    vs, f = _soup(1500, seed=7)
    pts = _queries(vs, f, seed=7)[len(vs):]                      # (not the vertices: their distance is 0)
    ref = np.sort(brute_force(_f32(pts), _f32(vs), f))
    gaps = np.diff(ref)
    lo = len(ref) // 3
    k = lo + int(np.argmax(gaps[lo:2 * len(ref) // 3]))          # a threshold in the widest gap of the middle third
    md = float(0.5 * (ref[k] + ref[k + 1]))
    r, _, _ = _check(vs, f, pts, max_dist=md)
    assert r["n_dropped"] == len(ref) - (k + 1)


def test_far_outlier_vertex_stays_exact_within_the_cell_cap():
    from dual_dmp_amd import synth
    from dual_dmp_amd.evaluate import SurfaceDistance
    vs, f = synth.icosphere(3)
    edge = float(np.mean(np.linalg.norm(vs[f[:, 0]] - vs[f[:, 1]], axis=1)))
    vs = vs.copy()
    vs[7] += np.array([1.0, 0.6, -0.3]) * 1e4 * edge
    _check(vs, f, _queries(vs, f, seed=3))
    sd = SurfaceDistance(vs, f, DEV)
    hdr = sd._grid[:48].cpu().numpy()
    dims = hdr[24:36].view(np.int32)
    ncells = int(hdr[36:40].view(np.int32)[0])
    assert ncells == int(np.prod(dims.astype(np.int64))) and ncells <= 4 * len(f)


def test_two_runs_are_bitwise_identical():
    from dual_dmp_amd import synth
    from dual_dmp_amd.evaluate import SurfaceDistance
    vs, f = synth.permute_vertices(*synth.torus(60, 40), seed=2)
    pts = _queries(vs, f, seed=9)
    outs = []
    for sort in (True, True, False):
        r = SurfaceDistance(vs, f, DEV).query(pts, per_sample=True, sort=sort)
        outs.append((r.pop("dist").cpu().numpy(), r))
    for d, r in outs[1:]:
        assert np.array_equal(d, outs[0][0]) and r == outs[0][1]


def test_one_million_faces_both_directions():
    from dual_dmp_amd import synth
    from dual_dmp_amd.evaluate import SurfaceDistance
    vs, f = synth.torus(1000, 500)
    gt, noisy, _ = synth.make_triplet(vs, f, steps=1)
    assert len(f) == 1000000
    rng = np.random.default_rng(0)
    for a, b in ((noisy, gt), (gt, noisy)):
        r = SurfaceDistance(b.vs, b.faces, DEV).query(a.vs, per_sample=True)
        d = r.pop("dist").cpu().numpy().astype(np.float64)
        idx = rng.choice(len(a.vs), 4096, replace=False)
        ref = brute_force(_f32(a.vs[idx]), _f32(b.vs), b.faces, chunk=16, device=DEV)
        M = max(np.abs(_f32(a.vs)).max(), np.abs(_f32(b.vs)).max())
        assert (np.abs(d[idx] - ref) <= TOL * (M + ref)).all()
        assert r["n"] == len(a.vs) and abs(r["mean"] - d.mean()) <= 1e-6 * d.mean()


def test_evaluator_hausdorff_equals_standalone_after_training_steps():
    from dual_dmp_amd import synth
    from dual_dmp_amd.datamaker import dataset_from_meshes
    from dual_dmp_amd.evaluate import Evaluator, hausdorff
    from dual_dmp_amd.networks import PosNet, NormalNet
    from dual_dmp_amd.trainer import FusedTrainer
    v, f = synth.icosphere(3)
    gt, noisy, smooth = synth.make_triplet(v, f)
    data = dataset_from_meshes(noisy, smooth)
    data.to(DEV)
    torch.manual_seed(0)
    tr = FusedTrainer(PosNet(DEV), NormalNet(DEV), data, noisy)
    ev = Evaluator(noisy, gt.fn, DEV, gt_mesh=gt)
    for _ in range(3):
        tr.step()
        pos = tr.pos.detach()
        got = ev.hausdorff(pos)
        want = hausdorff((pos.cpu().numpy(), f), gt, DEV)
        assert got["hd"] == want["hd"] and got["ab"] == want["ab"] and got["ba"] == want["ba"]
        assert got["hd"] > 0.0


def _run(cmd, timeout):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)


def test_check_cli_end_to_end(tmp_path):
    from dual_dmp_amd import synth
    from dual_dmp_amd import loss as Loss
    from dual_dmp_amd.evaluate import hausdorff
    from dual_dmp_amd.mesh import Mesh
    v, f = synth.icosphere(3)
    gt, noisy, smooth = synth.make_triplet(v, f)
    d = synth.write_dataset_dir(str(tmp_path), "ico", gt, noisy, smooth)
    p = _run([sys.executable, "-m", "dual_dmp_amd.check", "-i", d, "--json", str(tmp_path / "out.json")], 300)
    assert p.returncode == 0, p.stdout
    import json
    res = json.load(open(tmp_path / "out.json"))
    g = Mesh(os.path.join(d, "ico_gt.obj"))
    for stem in ("ico_noise", "ico_smooth"):
        m = Mesh(os.path.join(d, stem + ".obj"))
        mad = Loss.mad(m.fn, g.fn)
        hd = hausdorff(m, g, DEV)
        assert "{:20s}: {:.3f}".format(stem + ".obj", mad) in p.stdout
        assert "{:20s}: {:.7f}".format(stem + ".obj", hd["hd"]) in p.stdout
        assert res[stem + ".obj"]["mad"] == mad and res[stem + ".obj"]["hd"] == hd["hd"]
        for sub, key in (("mad", "{:.3f}".format(mad)), ("hd", "{:.6f}".format(hd["ab"]["mean"] / hd["ab"]["diag"]))):
            ply = os.path.join(d, sub, "%s=%s.ply" % (stem, key))
            head = open(ply).read().split("end_header\n")[0]
            assert "element vertex %d\n" % len(m.vs) in head and "element face %d\n" % len(m.faces) in head


def test_main_hd_flag_prints_hd(tmp_path):
    from dual_dmp_amd import synth
    v, f = synth.icosphere(2)
    gt, noisy, smooth = synth.make_triplet(v, f)
    d = synth.write_dataset_dir(str(tmp_path / "datasets"), "ico", gt, noisy, smooth)
    env_cwd = str(tmp_path)
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "-i", d, "--iter", "100", "--hd", "--seed", "0"]
    p = subprocess.run(cmd, cwd=env_cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("hd=")]
    assert len(lines) == 2, p.stdout[-3000:]                     # the OBJ at iteration 100, then the end
    assert all(0.0 < float(l[3:]) < 1.0 for l in lines)


def _cap_soup():
    """512 right triangles (legs 1) scattered in the plane z = 0 over [0, 31.5 h] x [0, 63.5 h], h = the mean edge length:
    the grid is exactly 32 x 64 x 1 = 2048 cells = the cap (4 F) = one whole scan tile, so the end offset of the last cell
    lies past the last tile."""
    rng = np.random.default_rng(11)
    h = (2.0 + 2.0 ** 0.5) / 3.0
    X, Y = 31.5 * h, 63.5 * h
    base = np.stack([rng.random(512) * (X - 1.0), rng.random(512) * (Y - 1.0)], 1)
    base[0] = (0.0, 0.0)
    base[1] = (X - 1.0, Y - 1.0)                                 # the far corner of the box
    base[2:40] = (X - 1.0, Y - 1.0) - rng.random((38, 2)) * 1.5  # and the last cell's neighbourhood
    vs = np.zeros((3 * 512, 3))
    vs[0::3, :2] = base
    vs[1::3, :2] = base + (1.0, 0.0)
    vs[2::3, :2] = base + (0.0, 1.0)
    return vs, np.arange(3 * 512).reshape(512, 3), (X, Y)


def test_grid_whose_cell_count_is_the_cap_and_a_whole_tile():
    from dual_dmp_amd.evaluate import SurfaceDistance
    vs, f, (X, Y) = _cap_soup()
    sd = SurfaceDistance(vs, f, DEV)
    sd._grid.fill_(255)                                          # a stale buffer: every word the build leaves alone is -1
    sd.update(vs)
    hdr = sd._grid[:48].cpu().numpy()
    assert list(hdr[24:36].view(np.int32)) == [32, 64, 1] and int(hdr[36:40].view(np.int32)[0]) == 4 * len(f) == 2048
    rng = np.random.default_rng(12)
    corner = np.array([X, Y, 0.0]) - rng.random((400, 3)) * (3.0, 3.0, -1.0) - (0.0, 0.0, 0.5)
    spread = rng.random((400, 3)) * (X, Y, 4.0) - (0.0, 0.0, 2.0)
    pts = np.concatenate([vs, corner, spread])
    r = sd.query(pts, per_sample=True)
    d = r["dist"].cpu().numpy().astype(np.float64)
    ref = brute_force(_f32(pts), _f32(vs), f)
    M = max(np.abs(pts).max(), np.abs(vs).max())
    assert (np.abs(d - ref) <= TOL * (M + ref)).all()


def test_non_finite_input_is_refused():
    import ctypes
    from dual_dmp_amd import _lib, synth
    from dual_dmp_amd.evaluate import SurfaceDistance
    from dual_dmp_amd.ops import _p, _stream
    vs, f = synth.icosphere(2)
    sd = SurfaceDistance(vs, f, DEV)
    for bad in (np.inf, -np.inf, np.nan):
        v = vs.copy()
        v[5, 1] = bad
        with pytest.raises(ValueError):
            SurfaceDistance(v, f, DEV)
        with pytest.raises(ValueError):
            sd.query(v)
    # the library refuses such a grid by itself (no Python check in between): EINVAL, nothing built, queries give NaN
    L = _lib.lib()
    faces = torch.from_numpy(f.astype(np.int32)).to(DEV)
    grid = torch.empty(L.ddmp_surfdist_grid_bytes(len(f), 16 * len(f)), dtype=torch.uint8, device=DEV)
    out = torch.empty(12, dtype=torch.float64, device=DEV)
    dist = torch.empty(len(vs), dtype=torch.float32, device=DEV)
    pts = torch.from_numpy(vs.astype(np.float32)).to(DEV)
    ws = torch.empty(L.ddmp_surfdist_query_workspace_bytes(len(vs), len(f)), dtype=torch.uint8, device=DEV)
    for bad in (np.inf, -np.inf, np.nan, 3e38):
        v = vs.astype(np.float32)
        v[f[7, 2]] = (bad, 1.0, 0.0) if bad == 3e38 else (0.0, bad, 0.0)
        if bad == 3e38:
            v[f[300, 0]] = (-bad, 1.0, 0.0)                      # an x extent of 6e38: beyond the float32 range
        pos = torch.from_numpy(v).to(DEV)
        need = ctypes.c_int64(0)
        st = L.ddmp_surfdist_build(len(vs), len(f), _p(pos), _p(faces), _p(grid), grid.numel(), ctypes.addressof(need), _stream())
        assert st == -1, (bad, st)                               # (3e38: finite, but the extent overflows float32)
        assert L.ddmp_surfdist_query(len(f), _p(grid), grid.numel(), len(vs), _p(pts), 0.0, 1, _p(dist), _p(out), _p(ws),
                                     ws.numel(), _stream()) == 0
        assert torch.isnan(dist).all()
    # a non-finite query point: NaN for it (never a silent drop), the others exact
    q = pts.clone()
    q[3, 0] = float("nan")
    assert L.ddmp_surfdist_query(len(f), _p(sd._grid), sd._grid.numel(), len(vs), _p(q), 0.0, 1, _p(dist), _p(out), _p(ws),
                                 ws.numel(), _stream()) == 0
    d = dist.cpu().numpy()
    s = out.cpu().numpy()
    assert np.isnan(d[3]) and (d[np.arange(len(d)) != 3] == 0.0).all() and np.isnan(s[1]) and s[5] == 0.0


def test_points_far_outside_the_grid_are_exact():
    from dual_dmp_amd import synth
    vs, f = synth.cube_cad(12)
    rng = np.random.default_rng(4)
    pts = np.concatenate([vs + (40.0, 0.0, 0.0), vs * 3.0 + (0.0, -25.0, 60.0), rng.normal(size=(200, 3)) * 500.0])
    _check(vs, f, pts)

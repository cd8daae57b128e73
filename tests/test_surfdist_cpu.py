"""Host side of the surface-distance / mesh-check feature (no GPU): the float64 brute-force reference the GPU tests use,
the numpy jet colormap, Mesh.save_as_ply, the check CLI's host logic (distance call replaced) and main.py's --hd flag."""
import json
import os

import numpy as np
import pytest
import torch

from surfdist_ref import brute_force, point_tri_d2

A, B, C = np.array([0.0, 0.0, 0.0]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 2.0, 0.0])


def _d(p, a=A, b=B, c=C):
    t = lambda x: torch.tensor(np.asarray(x, dtype=np.float64))
    return float(point_tri_d2(t(p), t(a), t(b), t(c)).sqrt())


@pytest.mark.parametrize("p,want", [
    ((0.5, 0.5, 0.75), 0.75),                  # face (above the interior)
    ((-1.0, -1.0, 0.0), 2 ** 0.5),             # vertex A
    ((3.0, -1.0, 0.0), 2 ** 0.5),              # vertex B
    ((-1.0, 3.0, 0.0), 2 ** 0.5),              # vertex C
    ((1.0, -2.0, 0.0), 2.0),                   # edge AB
    ((-3.0, 1.0, 4.0), 5.0),                   # edge AC
    ((2.0, 2.0, 0.0), 2 ** 0.5),               # edge BC
    ((1.0, 1.0, 0.0), 0.0),                    # on the hypotenuse
    ((0.5, 0.25, -2.0), 2.0),                  # face, below
])
def test_reference_in_every_voronoi_region(p, want):
    assert abs(_d(p) - want) <= 1e-12


def test_reference_on_degenerate_triangles():
    # repeated vertex: a segment
    assert abs(_d((1.0, 1.0, 0.0), A, A, B) - 1.0) <= 1e-12
    assert abs(_d((3.0, 0.0, 4.0), A, B, B) - (1.0 + 16.0) ** 0.5) <= 1e-12
    # all three equal: a point
    assert abs(_d((3.0, 4.0, 0.0), A, A, A) - 5.0) <= 1e-12
    # collinear: the hull segment from (0,0,0) to (4,0,0)
    assert abs(_d((2.0, 3.0, 0.0), A, np.array([4.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])) - 3.0) <= 1e-12
    assert abs(_d((6.0, 0.0, 0.0), A, np.array([4.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])) - 2.0) <= 1e-12
    d = brute_force(np.array([[0.0, 0.0, 1.0]]), np.array([A, A, A]), np.array([[0, 1, 2]]))
    assert np.isfinite(d).all() and abs(d[0] - 1.0) <= 1e-12


def test_reference_brute_force_picks_the_nearest_triangle():
    vs = np.array([A, B, C, [10.0, 0.0, 0.0], [12.0, 0.0, 0.0], [10.0, 2.0, 0.0]])
    f = np.array([[0, 1, 2], [3, 4, 5]])
    d = brute_force(np.array([[0.5, 0.5, 1.0], [10.5, 0.5, -2.0], [6.0, 0.0, 0.0]]), vs, f)
    assert np.allclose(d, [1.0, 2.0, 4.0], atol=1e-12)


def test_jet_matches_matplotlib():
    cm = pytest.importorskip("matplotlib.cm")
    from dual_dmp_amd.check import jet
    x = np.linspace(0.0, 1.0, 1001)
    assert np.allclose(jet(x), cm.jet(x)[:, :3], atol=1e-12, rtol=0)
    y = np.array([-0.5, 1.5])
    assert np.allclose(jet(y), cm.jet(y)[:, :3], atol=1e-12, rtol=0)


def test_jet_endpoints_without_matplotlib():
    from dual_dmp_amd.check import jet
    c = jet([0.0, 0.5, 1.0, -1.0, 2.0])
    assert np.allclose(c[0], [0.0, 0.0, 0.5]) and np.allclose(c[2], [0.5, 0.0, 0.0])
    assert np.array_equal(c[3], c[0]) and np.array_equal(c[4], c[2]) and c.shape == (5, 3)


def _two_triangles():
    from dual_dmp_amd.mesh import Mesh
    return Mesh(vs=[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.5]], faces=[[0, 1, 2], [1, 3, 2]])


PLY_FACE = """ply
format ascii 1.0
element vertex 4
property float x
property float y
property float z
element face 2
property list uchar int vertex_indices
property uchar red
property uchar green
property uchar blue
property uchar alpha
end_header
0.000000 0.000000 0.000000
1.000000 0.000000 0.000000
0.000000 1.000000 0.000000
1.000000 1.000000 0.500000
3 0 1 2 25 127 255 255
3 1 3 2 0 254 1 255
"""

PLY_VERTEX = """ply
format ascii 1.0
element vertex 4
property float x
property float y
property float z
property uchar red
property uchar green
property uchar blue
property uchar alpha
element face 2
property list uchar int vertex_indices
end_header
0.000000 0.000000 0.000000 25 127 255 255
1.000000 0.000000 0.000000 0 254 1 255
0.000000 1.000000 0.000000 0 0 0 255
1.000000 1.000000 0.500000 255 255 255 255
3 0 1 2
3 1 3 2
"""


def test_save_as_ply_face_colours(tmp_path):
    m = _two_triangles()
    m.save_as_ply(str(tmp_path / "f.ply"), face_colors=np.array([[0.1, 0.5, 1.2], [-0.2, 0.999, 0.004]]))
    assert open(tmp_path / "f.ply").read() == PLY_FACE


def test_save_as_ply_vertex_colours(tmp_path):
    m = _two_triangles()
    m.save_as_ply(str(tmp_path / "v.ply"),
                  vertex_colors=np.array([[0.1, 0.5, 1.2], [-0.2, 0.999, 0.004], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]))
    assert open(tmp_path / "v.ply").read() == PLY_VERTEX


def _dataset(tmp_path):
    from dual_dmp_amd import synth
    v, f = synth.icosphere(1)
    gt, noisy, smooth = synth.make_triplet(v, f)
    d = synth.write_dataset_dir(str(tmp_path), "ico", gt, noisy, smooth)
    open(os.path.join(d, "notes.txt"), "w").write("not a mesh")
    return d


def _fake_distances(monkeypatch):
    from dual_dmp_amd import check

    class Fake:
        def __init__(self, gt_mesh, max_dist):
            self.max_dist = max_dist

        def __call__(self, mesh):
            d = np.linspace(0.0, 1.0, len(mesh.vs))
            one = {"mean": 0.25, "rms": 0.5, "min": 0.0, "max": 1.0, "n": len(mesh.vs), "n_dropped": 0, "diag": 2.0}
            return {"hd": 0.125, "ab": one, "ba": dict(one), "diag_a": 2.0, "diag_b": 2.0}, d
    monkeypatch.setattr(check, "_Distances", Fake)


def test_check_finds_inputs_and_skips_the_gt(tmp_path):
    from dual_dmp_amd.check import find_inputs
    d = _dataset(tmp_path)
    gt, files = find_inputs(d)
    assert os.path.basename(gt) == "ico_gt.obj"
    assert [os.path.basename(p) for p in files] == ["ico_noise.obj", "ico_smooth.obj"]
    gt, files = find_inputs(d, gt=os.path.join(d, "ico_smooth.obj"))
    assert os.path.basename(gt) == "ico_smooth.obj"
    assert [os.path.basename(p) for p in files] == ["ico_gt.obj", "ico_noise.obj"]
    out = os.path.join(d, "output")
    os.makedirs(out)
    gt, files = find_inputs(out, gt=os.path.join(d, "ico_gt.obj"))          # training's output folder, GT one level up
    assert files == [] and gt.endswith("ico_gt.obj")


def test_check_outputs_names_and_max_val(tmp_path, monkeypatch):
    from dual_dmp_amd import check, loss as Loss
    from dual_dmp_amd.mesh import Mesh
    _fake_distances(monkeypatch)
    d = _dataset(tmp_path)
    lines = []
    assert check.run(["-i", d, "--json", str(tmp_path / "r.json")], log=lines.append) == 0
    g = Mesh(os.path.join(d, "ico_gt.obj"))
    mx = open(os.path.join(d, "hd", "max_val.txt")).read()
    assert mx == "{:.7f}".format(0.002 * np.linalg.norm(g.vs.max(0) - g.vs.min(0)))
    res = json.load(open(tmp_path / "r.json"))
    for stem in ("ico_noise", "ico_smooth"):
        mad = Loss.mad(Mesh(os.path.join(d, stem + ".obj")).fn, g.fn)
        assert os.path.exists(os.path.join(d, "mad", "{}={:.3f}.ply".format(stem, mad)))
        assert os.path.exists(os.path.join(d, "hd", "{}=0.125000.ply".format(stem)))
        assert "{:20s}: {:.3f}".format(stem + ".obj", mad) in lines
        assert "{:20s}: {:.7f}".format(stem + ".obj", 0.125) in lines
        assert res[stem + ".obj"]["mad"] == mad and res[stem + ".obj"]["hd"] == 0.125
        assert res[stem + ".obj"]["ab"]["mean"] == 0.25 and res[stem + ".obj"]["ba"]["n"] > 0
    assert sorted(os.listdir(os.path.join(d, "hd"))) == ["ico_noise=0.125000.ply", "ico_smooth=0.125000.ply", "max_val.txt"]
    lines.clear()
    assert check.run(["-i", d, "--no_mad", "--no_hd"], log=lines.append) == 0
    assert not any(l.startswith("ico_") for l in lines)


def test_check_without_gt_exits_nonzero(tmp_path):
    from dual_dmp_amd import check
    from dual_dmp_amd.mesh import Mesh
    Mesh(vs=np.eye(3), faces=[[0, 1, 2]]).save(str(tmp_path / "a.obj"))
    lines = []
    assert check.run(["-i", str(tmp_path)], log=lines.append) == 1
    assert lines[-1] == "No ground-truth mesh was detected!"
    with pytest.raises(SystemExit) as e:
        import sys
        argv, sys.argv = sys.argv, ["check", "-i", str(tmp_path)]
        try:
            check.main()
        finally:
            sys.argv = argv
    assert e.value.code == 1


def test_hd_flag_parses_and_defaults_off():
    from dual_dmp_amd.cli import get_parser
    base = vars(get_parser(False).parse_args(["-i", "x"]))
    assert base.pop("hd") is False
    on = vars(get_parser(False).parse_args(["-i", "x", "--hd"]))
    assert on.pop("hd") is True and on == base
    assert base["iter"] == 1000 and base["k1"] == 3.0 and base["bnfloop"] == 1 and base["gpu"] == 0
    assert "hd" not in vars(get_parser(True).parse_args(["-i", "x"]))     # main4real.py: unchanged


def test_non_finite_points_are_refused_before_any_device_work():
    from dual_dmp_amd.evaluate import _points
    assert _points(np.ones((2, 3)), "cpu").dtype == torch.float32
    for bad in (np.inf, -np.inf, np.nan, 1e39):                   # (1e39 is inf in float32)
        x = np.zeros((4, 3))
        x[2, 1] = bad
        with pytest.raises(ValueError):
            _points(x, "cpu")

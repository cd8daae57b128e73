"""``python -m dual_dmp_amd.check -i DIR [--gt PATH] [--no_mad] [--no_hd] [--max_dist F] [--json OUT]``

The reference's two result checkers in one command (``check/mad_checker.py`` and ``check/hausdorff_checker.py``): for every
``*.obj`` in DIR except the ground truth (``DIR/*_gt.obj``, or ``--gt``; training writes its outputs to
``datasets/<name>/output/`` while the GT sits one directory up),

* MAD: mean angular difference of the float64 face normals to the GT's (``loss.mad``), and ``DIR/mad/<stem>=<mad>.ply``
  coloured per face by the angular error, jet over [0, 50] degrees;
* Hausdorff: the two-sided mean surface distance over the bounding-box diagonals, ``0.5 * (mean_ab / diag_a + mean_ba /
  diag_b)`` with a = the output, b = the GT (``evaluate.hausdorff``, on the GPU), and ``DIR/hd/<stem>=<mean_ab / diag_a>.ply``
  coloured per vertex by its distance to the GT, jet over [0, max_val], max_val = 0.002 * diag(GT) (``DIR/hd/max_val.txt``).

The tables are printed in the reference's formats; ``--json`` also keeps both one-sided results of every file.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys

import numpy as np

# matplotlib's "jet" (_cm.py segment data: (x, y) knots per channel), sampled the way a 256-entry
# LinearSegmentedColormap is: a lookup table at i / 255, indexed by int(256 x) clipped to 0 .. 255
_JET = {
    "red": ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
    "green": ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
    "blue": ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)),
}
_N = 256


def _jet_lut():
    xs = np.linspace(0.0, 1.0, _N)
    return np.stack([np.interp(xs, [k[0] for k in _JET[c]], [k[1] for k in _JET[c]]) for c in ("red", "green", "blue")], 1)


def jet(x):
    """RGB [n, 3] in [0, 1] of matplotlib's ``cm.jet(x)[:, :3]`` for values ``x`` (below 0: the first colour, above 1: the
    last; NaN: black)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    idx = np.clip(np.nan_to_num(x * _N, nan=0.0, posinf=_N, neginf=-1.0), -1, _N).astype(np.int64)
    idx = np.clip(idx, 0, _N - 1)
    out = _jet_lut()[idx]
    out[np.isnan(x)] = 0.0
    return out


def find_inputs(folder, gt=None):
    """-> (gt path or None, sorted list of the other ``*.obj`` files of ``folder``)."""
    if gt is None:
        g = sorted(glob.glob(os.path.join(folder, "*_gt.obj")))
        gt = g[0] if g else None
    skip = os.path.abspath(gt) if gt is not None else None
    files = [p for p in sorted(glob.glob(os.path.join(folder, "*.obj"))) if os.path.abspath(p) != skip]
    return gt, files


def bbox_diag(vs):
    vs = np.asarray(vs, dtype=np.float64)
    return float(np.linalg.norm(vs.max(0) - vs.min(0)))


class _Distances:
    """The GT's grid, built once; per output: both one-sided queries (``evaluate._combine`` of them is exactly
    ``evaluate.hausdorff(out, gt)``) plus the per-vertex distances of the output for its colours."""

    def __init__(self, gt_mesh, max_dist):
        import torch
        from .evaluate import SurfaceDistance
        if not torch.cuda.is_available():
            raise RuntimeError("the Hausdorff distance runs on the GPU (HIP): no device found; --no_hd skips it")
        self.dev = torch.device("cuda:0")
        self.gt = gt_mesh
        self.max_dist = max_dist
        self.grid = SurfaceDistance(gt_mesh.vs, gt_mesh.faces, self.dev)

    def __call__(self, mesh):
        from .evaluate import SurfaceDistance, _combine
        ab = self.grid.query(mesh.vs, max_dist=self.max_dist, per_sample=True)
        d = ab.pop("dist").cpu().numpy()
        ba = SurfaceDistance(mesh.vs, mesh.faces, self.dev).query(self.gt.vs, max_dist=self.max_dist)
        return _combine(ab, ba), d


def get_parser():
    p = argparse.ArgumentParser(
        prog="python -m dual_dmp_amd.check",
        description="MAD and Hausdorff distance of every *.obj in a folder against its ground truth (the reference's "
                    "check/mad_checker.py and check/hausdorff_checker.py).  The distance samples every vertex of the "
                    "sampled mesh (MeshLab's vertex sampling) and normalises by that mesh's bounding-box diagonal.  "
                    "The hd/*.ply files are coloured with jet over [0, max_val], NOT with MeshLab's own colour ramp.")
    p.add_argument("-i", "--input", type=str, required=True, help="folder of *.obj outputs")
    p.add_argument("--gt", type=str, default=None, help="ground-truth OBJ (default: the folder's *_gt.obj)")
    p.add_argument("--no_mad", action="store_true", help="skip the MAD and the mad/*.ply files")
    p.add_argument("--no_hd", action="store_true", help="skip the Hausdorff distance and the hd/*.ply files")
    p.add_argument("--max_dist", type=float, default=0.0,
                   help="leave samples farther than this out of the mean (MeshLab's maxdist); 0: every sample counts")
    p.add_argument("--json", type=str, default=None, help="write every figure (both one-sided results too) to this file")
    return p


def run(argv=None, log=print):
    from .mesh import Mesh
    from . import loss as Loss
    args = get_parser().parse_args(argv)
    for k, v in vars(args).items():
        log("{:12s}: {}".format(k, v))
    folder = args.input
    gt_path, files = find_inputs(folder, args.gt)
    if gt_path is None:
        log("No ground-truth mesh was detected!")
        return 1
    g_mesh = Mesh(gt_path)
    results = {}
    dist = None
    if not args.no_hd:
        os.makedirs(os.path.join(folder, "hd"), exist_ok=True)
        max_val = 0.002 * bbox_diag(g_mesh.vs)
        with open(os.path.join(folder, "hd", "max_val.txt"), "w") as f:
            f.write("{:.7f}".format(max_val))
        dist = _Distances(g_mesh, args.max_dist)
    if not args.no_mad:
        os.makedirs(os.path.join(folder, "mad"), exist_ok=True)
    for path in files:
        name = os.path.basename(path)
        stem = name.split(".")[0]
        mesh = Mesh(path)
        r = results.setdefault(name, {})
        if not args.no_mad:
            if len(mesh.faces) != len(g_mesh.faces):
                log("[WARN] %s: %d faces, the ground truth has %d: no MAD" % (name, len(mesh.faces), len(g_mesh.faces)))
            else:
                r["mad"] = float(Loss.mad(mesh.fn, g_mesh.fn))
                sad = Loss.angular_difference(mesh.fn, g_mesh.fn)
                mesh.save_as_ply(os.path.join(folder, "mad", "{}={:.3f}.ply".format(stem, r["mad"])),
                                 face_colors=jet(np.clip(sad, 0.0, 50.0) / 50.0))
        if dist is not None:
            res, d = dist(mesh)
            r.update(res)
            one = res["ab"]["mean"] / res["ab"]["diag"]
            mesh.save_as_ply(os.path.join(folder, "hd", "{}={:.6f}.ply".format(stem, one)),
                             vertex_colors=jet(np.clip(d / max_val, 0.0, 1.0)))
    for name, r in results.items():
        if "mad" in r:
            log("{:20s}: {:.3f}".format(name, r["mad"]))
    for name, r in results.items():
        if "hd" in r:
            log("{:20s}: {:.7f}".format(name, r["hd"]))
    if args.json:
        out = dict(results)
        out["_gt"] = gt_path
        if dist is not None:
            out["_max_val"] = max_val
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


def main():
    sys.exit(run())


if __name__ == "__main__":
    main()

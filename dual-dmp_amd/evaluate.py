"""Evaluation block of the training loop on the device (``main.py:117-127`` of the reference).

Every 10 iterations the reference copies ``pos`` to the host, recomputes face AND vertex normals in numpy
(with a Python list comprehension over faces, ``util/mesh.py:102``) and evaluates MAD; at 1M faces that stalls
the loop for seconds.  Here face normals and the MAD reduction are two small kernels; only the scalar comes
back.  ``Evaluator.mad(pos)`` == ``Loss.mad(o1_mesh.fn, gt_mesh.fn)`` after ``o1_mesh.vs = pos`` (float32).

Point-to-surface distance (the reference's ``check/hausdorff_checker.py``, which asks MeshLab for it): a uniform grid
over the target's triangles and an exact closest-point query per sample, both HIP (``csrc/surfdist.hip``).
:class:`SurfaceDistance` holds the grid of one mesh; :func:`hausdorff` gives both one-sided figures of two meshes and
the checker's ``0.5 * (mean_ab / diag_a + mean_ba / diag_b)``.  Samples are the vertices of the sampled mesh (MeshLab's
vertex sampling: the reference asks for ``3F >= V`` samples, so every vertex is taken); ``diag`` is the bounding-box
diagonal of the sampled mesh.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import check
from .loss import tables_for, _target
from .ops import Workspace, _p, _stream, on_device


# query points are counted-sorted by grid cell before the search (same results; see scripts/microbench.py hd)
SORT_QUERIES = True
_EWORKSPACE = -4                                                 # DDMP_EWORKSPACE (include/ddmp_hip.h)


def _mesh_arrays(m):
    """(vs, faces) of a Mesh or of a (vs, faces) pair."""
    return (m.vs, m.faces) if hasattr(m, "faces") else (m[0], m[1])


def _points(x, device):
    if isinstance(x, torch.Tensor):
        t = x.detach().to(device=device, dtype=torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32))).to(device)
    t = t.reshape(-1, 3).contiguous()
    if t.shape[0] == 0:
        raise ValueError("no points")
    if not bool(torch.isfinite(t).all()):                        # (one synchronisation; the kernels would give NaN / EINVAL)
        raise ValueError("non-finite coordinates (inf / NaN, or beyond the float32 range)")
    return t


class SurfaceDistance:
    """Grid of one target mesh on ``device``: ``query(points)`` -> distances from the points to its surface.

    ``update(pos)`` rebuilds the grid for moved vertices with the same connectivity (one stream synchronisation: the
    build reads its reference count back).  The grid buffer grows when a mesh needs more cell references."""

    def __init__(self, vs, faces, device):
        self.device = torch.device(device)
        f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
        f = np.ascontiguousarray(f.reshape(-1, 3), dtype=np.int64)
        if len(f) == 0:
            raise ValueError("the target mesh has no faces")
        self.F = len(f)
        self.faces = torch.from_numpy(f.astype(np.int32)).to(self.device)
        self._grid = None
        self._out = torch.empty(12, dtype=torch.float64, device=self.device)
        self.update(vs)

    def update(self, pos):
        """Rebuild the grid for vertex positions ``pos`` [V, 3] (tensor or array; float32 on the device)."""
        L = _lib.lib()
        with on_device(self.device):
            self.pos = _points(pos, self.device)
            V = self.pos.shape[0]
            refs = 8 * self.F if self._grid is None else None
            for _ in range(2):
                if refs is not None:
                    nbytes = L.ddmp_surfdist_grid_bytes(self.F, int(refs))
                    if nbytes == 0:
                        raise _lib.DdmpError("surface grid of %d faces with %d references exceeds the int32 index range" % (self.F, refs))
                    self._grid = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                need = ctypes.c_int64(0)
                st = L.ddmp_surfdist_build(V, self.F, _p(self.pos), _p(self.faces), _p(self._grid), self._grid.numel(),
                                           ctypes.addressof(need), _stream())
                if st != _EWORKSPACE:
                    break
                refs = need.value + need.value // 8                  # grow (with headroom for later updates) and rebuild once
            check(st, "ddmp_surfdist_build")
        return self

    def query(self, points, max_dist: float = 0.0, per_sample: bool = False, sort: bool = None):
        """Distances from ``points`` [Q, 3] to the surface.  -> ``{mean, rms, min, max, n, n_dropped, diag}`` (``diag``: the
        points' bounding-box diagonal) and ``dist`` [Q] f32 with ``per_sample``.  ``max_dist > 0``: samples farther than
        that are left out of the statistics and counted in ``n_dropped`` (their ``dist`` is +inf), as MeshLab's maxdist."""
        L = _lib.lib()
        max_dist = float(max_dist)
        if not (max_dist >= 0.0 and math.isfinite(max_dist)):
            raise ValueError("max_dist must be finite and >= 0")
        with on_device(self.device):
            pts = _points(points, self.device)
            Q = pts.shape[0]
            ws = Workspace.get(L.ddmp_surfdist_query_workspace_bytes(Q, self.F), self.device)
            dist = torch.empty(Q, dtype=torch.float32, device=self.device) if per_sample else None
            check(L.ddmp_surfdist_query(self.F, _p(self._grid), self._grid.numel(), Q, _p(pts), max_dist,
                                        int(SORT_QUERIES if sort is None else bool(sort)), _p(dist), _p(self._out), _p(ws),
                                        ws.numel(), _stream()), "ddmp_surfdist_query")
            s = self._out.cpu().numpy()
        n, nan = int(s[0]), float("nan")
        res = {"mean": float(s[1] / n) if n else nan, "rms": math.sqrt(s[2] / n) if n else nan,
               "min": float(s[3]) if n else nan, "max": float(s[4]) if n else nan, "n": n,
               "n_dropped": int(s[5]), "diag": float(np.sqrt(np.sum((s[9:12] - s[6:9]) ** 2)))}
        if per_sample:
            res["dist"] = dist
        return res


def _combine(ab, ba):
    """Both one-sided results -> the figure of check/hausdorff_checker.py."""
    return {"hd": 0.5 * (ab["mean"] / ab["diag"] + ba["mean"] / ba["diag"]), "ab": ab, "ba": ba,
            "diag_a": ab["diag"], "diag_b": ba["diag"]}


def hausdorff(a, b, device, max_dist: float = 0.0):
    """Two-sided mean surface distance of meshes ``a`` and ``b`` (Mesh objects or (vs, faces) pairs).  -> ``{"hd", "ab",
    "ba", "diag_a", "diag_b"}``: ``ab`` samples the vertices of ``a`` against the surface of ``b`` (``ba`` the reverse), each
    a :meth:`SurfaceDistance.query` result; ``hd = 0.5 * (ab.mean / diag_a + ba.mean / diag_b)`` with ``diag_x`` the
    bounding-box diagonal of the sampled mesh x."""
    va, fa = _mesh_arrays(a)
    vb, fb = _mesh_arrays(b)
    ab = SurfaceDistance(vb, fb, device).query(va, max_dist=max_dist)
    ba = SurfaceDistance(va, fa, device).query(vb, max_dist=max_dist)
    return _combine(ab, ba)


class Evaluator:
    def __init__(self, mesh, gt_fn, device, gt_mesh=None):
        self.tb = tables_for(mesh, device)
        self.gt = _target(gt_fn, device)
        self.fn = torch.empty((self.tb.F, 3), dtype=torch.float32, device=device)
        self.out = torch.zeros(1, dtype=torch.float64, device=device)
        self.device = device
        self.gt_mesh = gt_mesh
        self._gt_sd = self._out_sd = None

    def hausdorff(self, pos: torch.Tensor, max_dist: float = 0.0) -> dict:
        """:func:`hausdorff` of the output mesh (``pos`` on this evaluator's connectivity) against ``gt_mesh``: the GT grid is
        built on the first call, the output's grid is rebuilt from ``pos`` on every call."""
        if self.gt_mesh is None:
            raise ValueError("Evaluator.hausdorff needs gt_mesh=")
        if self._gt_sd is None:
            gv, gf = _mesh_arrays(self.gt_mesh)
            self._gt_sd = SurfaceDistance(gv, gf, self.device)
            self._gt_pts = _points(gv, self.device)
            self._out_sd = SurfaceDistance(pos, self.tb.faces, self.device)
        else:
            self._out_sd.update(pos)
        ab = self._gt_sd.query(pos, max_dist=max_dist)
        ba = self._out_sd.query(self._gt_pts, max_dist=max_dist)
        return _combine(ab, ba)

    def face_normals(self, pos: torch.Tensor) -> torch.Tensor:
        pos = pos.detach().to(torch.float32).contiguous()
        check(_lib.lib().ddmp_face_normals_f32(self.tb.F, _p(pos), _p(self.tb.faces), _p(self.fn), None, _stream()),
              "ddmp_face_normals_f32")
        return self.fn

    def mad(self, pos: torch.Tensor) -> float:
        self.face_normals(pos)
        L = _lib.lib()
        ws = Workspace.get(L.ddmp_mad_workspace_bytes(), pos.device)
        check(L.ddmp_mad_f64(self.tb.F, _p(self.fn), _p(self.gt), _p(self.out), _p(ws), ws.numel(), _stream()),
              "ddmp_mad_f64")
        return float(self.out.item())

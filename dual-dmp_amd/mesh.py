"""Triangle-mesh container with vectorised adjacency construction.

Mirrors the attribute names / dtypes of the reference ``Mesh`` object
(``util/mesh.py:8-21`` of astaka-pe/Dual-DMP) for everything the training hot
path consumes:

    vs  [V,3] f64      faces [F,3] i64     fn [F,3] f64   fa [F] f64   fc [F,3] f64
    vn  [V,3] f64      edges [E,2] i32     edges_count
    f2f [F,3] i64 (-1 padded)              f_edges [2,S] i64
    v2v_mat  sparse COO [V,V] f32 (uncoalesced, 2E entries)   v_dims [V] f32
    vf  list[set[int]] (lazy)              v2f_mat sparse COO [V,F] f32 (lazy)

The reference builds these with per-face Python loops (~100 us/face); here they
come from sorts over the 3F half-edges, so a 1M-face mesh builds in seconds.

Ordering conventions:
  * ``edges`` keeps the reference's order: first appearance while walking faces in
    order and, inside a face, the edges (v0,v1), (v1,v2), (v2,v0); each pair stored
    (min, max) (``util/mesh.py:45-85``).
  * ``f2f[i]`` lists the edge-adjacent faces of face ``i`` in the order of the edge
    they are met across, (v0,v1), (v1,v2), (v2,v0), boundary slots compacted to the
    right and padded with -1 (reference: ``util/mesh.py:176-187``, where the order
    inside a row follows CPython ``set`` iteration and only matters for the order of
    floating-point sums).
  * Faces that share all three vertices with ``i`` are not neighbours (the reference
    keeps only faces sharing *exactly* two vertices, ``util/mesh.py:180``).
  * More than three edge neighbours (a non-manifold edge) is an error, as it is in the
    reference where the ragged list cannot become the [F,3] array.

Extra (not in the reference) CSR views used by the HIP path: ``vf_ptr``/``vf_idx``
(vertex -> incident faces) and ``vv_ptr``/``vv_idx`` (vertex -> 1-ring vertices).

Out of scope here (never read by the training step): ``gemm_edges``, ``sides``, ``ve``,
``vei`` (MeshCNN leftovers, ``util/mesh.py:46-85``) and the optional Laplacian matrices
(``util/mesh.py:114-150,199-265``; ``build_mat`` is False everywhere in the reference).
"""
from __future__ import annotations

import numpy as np
import torch


def _csr_from_pairs(rows: np.ndarray, cols: np.ndarray, n: int):
    """rows/cols -> (ptr int64[n+1], idx int64[nnz]) sorted by (row, original order)."""
    order = np.argsort(rows, kind="stable")
    idx = cols[order]
    counts = np.bincount(rows, minlength=n)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    return ptr, idx.astype(np.int64, copy=False)


def _write_rows(fp, row_fmt, cols, chunk=1 << 16):
    """Text rows of the column blocks ``cols`` (float32 / integer arrays, widened to float64 exactly): one %-formatting
    call per chunk of rows, no Python loop per row."""
    for i in range(0, len(cols[0]), chunk):
        rows = np.concatenate([np.asarray(c[i:i + chunk], dtype=np.float64) for c in cols], 1)
        fp.write((row_fmt * len(rows)) % tuple(rows.ravel().tolist()))


class Mesh:
    """``Mesh(path)`` parses an OBJ like the reference (``util/mesh.py:23-43``);
    ``Mesh(vs=..., faces=...)`` wraps in-memory arrays (used for the synthetic
    1M-face inputs, where a text round trip would dominate start-up)."""

    def __init__(self, path=None, build_mat=False, *, vs=None, faces=None):
        if build_mat:
            raise NotImplementedError(
                "build_mat=True (uniform / cotangent Laplacian matrices, util/mesh.py:114,199) "
                "is outside the training hot path and not built")
        self.path = path
        if path is not None:
            self.vs, self.faces = self.fill_from_file(path)
        else:
            if vs is None or faces is None:
                raise ValueError("Mesh needs either a path or vs= and faces=")
            self.vs = np.array(vs, dtype=np.float64)
            self.faces = np.array(faces, dtype=np.int64)
            assert self.faces.ndim == 2 and self.faces.shape[1] == 3
            assert np.logical_and(self.faces >= 0, self.faces < len(self.vs)).all()
        self.device = "cpu"
        self._vf = None
        self._v2f_mat = None
        self.compute_face_normals()
        self.compute_face_center()
        self.build_gemm()
        self.compute_vert_normals()
        self.build_v2v()
        self.build_vf()

    # ------------------------------------------------------------------ IO
    @staticmethod
    def fill_from_file(path):
        """OBJ subset of the reference parser: ``v x y z``; ``f a b c`` with optional
        ``/t/n`` suffixes, 1-based or negative indices, triangles only."""
        vs, faces = [], []
        with open(path) as fh:
            for line in fh:
                tok = line.split()
                if not tok:
                    continue
                if tok[0] == "v":
                    vs.append((float(tok[1]), float(tok[2]), float(tok[3])))
                elif tok[0] == "f":
                    ids = [int(c.split("/")[0]) for c in tok[1:]]
                    assert len(ids) == 3
                    faces.append([(i - 1) if i >= 0 else (len(vs) + i) for i in ids])
        vs = np.asarray(vs, dtype=np.float64).reshape(-1, 3)
        faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        assert np.logical_and(faces >= 0, faces < len(vs)).all()
        return vs, faces

    def save(self, filename):
        """Same text format as ``util/mesh.py:267-285``: float32 positions printed with
        ``%.8f``, 1-based faces."""
        assert len(self.vs) > 0
        v = np.asarray(self.vs, dtype=np.float32)
        f = np.asarray(self.faces, dtype=np.uint32).astype(np.int64) + 1
        with open(filename, "w") as fp:
            fp.write("".join("v {0:.8f} {1:.8f} {2:.8f}\n".format(x, y, z) for x, y, z in v))
            fp.write("".join("f {0} {1} {2}\n".format(a, b, c) for a, b, c in f))

    def save_as_ply(self, filename, face_colors=None, vertex_colors=None):
        """ASCII PLY in the header layout of ``util/mesh.py:287-317``: float32 positions printed with ``%.6f``, faces as
        ``3 i j k`` followed by ``uchar red green blue alpha`` per face (colours in [0, 1]: ``int(255 c)`` truncated, then
        clipped to 0..255; alpha 255).  With ``vertex_colors`` instead, the colour properties belong to the vertices.
        Written with numpy's text formatter, not a Python loop per face."""
        assert len(self.vs) > 0
        if face_colors is not None and vertex_colors is not None:
            raise ValueError("face_colors or vertex_colors, not both")
        v = np.asarray(self.vs, dtype=np.float32)
        f = np.asarray(self.faces, dtype=np.uint32).astype(np.int64)

        def rgba(c, n):
            c = np.asarray(c, dtype=np.float32).reshape(n, -1)[:, :3]
            u = np.clip((255 * c).astype(np.int64), 0, 255)                 # int(): toward zero, as the reference
            return np.concatenate([u, np.full((n, 1), 255, dtype=np.int64)], 1)

        colour = "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
        head = ["ply\nformat ascii 1.0\nelement vertex {}\n".format(len(v)), "property float x\nproperty float y\nproperty float z\n"]
        if vertex_colors is not None:
            head.append(colour)
        head += ["element face {}\n".format(len(f)), "property list uchar int vertex_indices\n"]
        if face_colors is not None:
            head.append(colour)
        head.append("end_header\n")
        with open(filename, "w") as fp:
            fp.write("".join(head))
            if vertex_colors is not None:
                _write_rows(fp, "%.6f %.6f %.6f %d %d %d %d\n", [v, rgba(vertex_colors, len(v))])
            else:
                _write_rows(fp, "%.6f %.6f %.6f\n", [v])
            if face_colors is not None:
                _write_rows(fp, "3 %d %d %d %d %d %d %d\n", [f, rgba(face_colors, len(f))])
            else:
                _write_rows(fp, "3 %d %d %d\n", [f])

    # ------------------------------------------------------- per-face geometry
    def compute_face_normals(self):
        """``util/mesh.py:87-92``: unnormalised cross product; ``fn /= |.| + 1e-24``;
        ``fa = 0.5 |.|``."""
        vs, faces = self.vs, self.faces
        cr = np.cross(vs[faces[:, 1]] - vs[faces[:, 0]], vs[faces[:, 2]] - vs[faces[:, 0]])
        nrm = np.linalg.norm(cr, axis=1, keepdims=True) + 1e-24
        self.fa = 0.5 * np.sqrt((cr ** 2).sum(axis=1))
        self.fn = cr / nrm

    def compute_face_center(self):
        """``util/mesh.py:109-112``."""
        self.fc = np.sum(self.vs[self.faces], 1) / 3.0

    def compute_vert_normals(self):
        """``util/mesh.py:94-107``: sum of incident face normals, L2-normalised per row
        (all-zero rows stay zero, as sklearn's ``normalize`` leaves them)."""
        nv = len(self.vs)
        acc = np.zeros((nv, 3), dtype=np.float64)
        flat = self.faces.reshape(-1)
        rep = np.repeat(self.fn, 3, axis=0)
        for c in range(3):
            acc[:, c] = np.bincount(flat, weights=rep[:, c], minlength=nv)
        nrm = np.sqrt((acc ** 2).sum(axis=1, keepdims=True))
        nrm[nrm == 0.0] = 1.0
        self.vn = acc / nrm

    # ----------------------------------------------------------- connectivity
    def _half_edges(self):
        f = self.faces
        a = f[:, [0, 1, 2]].reshape(-1)
        b = f[:, [1, 2, 0]].reshape(-1)
        lo = np.minimum(a, b)
        hi = np.maximum(a, b)
        return lo, hi

    def build_gemm(self):
        """Unique undirected edges in first-seen order (``util/mesh.py:45-85``)."""
        nv = len(self.vs)
        lo, hi = self._half_edges()
        key = lo * np.int64(nv) + hi
        _, first = np.unique(key, return_index=True)
        first.sort()
        self.edges = np.stack([lo[first], hi[first]], axis=1).astype(np.int32)
        self.edges_count = int(len(first))
        self._he_key = key

    def build_v2v(self):
        """``util/mesh.py:189-197``: COO adjacency (both directions, uncoalesced) and the
        float32 vertex degree."""
        nv = len(self.vs)
        e = self.edges.T.astype(np.int64)
        inds = np.concatenate([e, e[[1, 0]]], axis=1)
        inds_t = torch.from_numpy(inds).long()
        vals = torch.ones(inds_t.shape[1], dtype=torch.float32)
        self.v2v_mat = torch.sparse_coo_tensor(inds_t, vals, size=(nv, nv))
        self.v_dims = torch.from_numpy(
            np.bincount(inds[0], minlength=nv).astype(np.float32))
        self.vv_ptr, self.vv_idx = _csr_from_pairs(inds[0], inds[1], nv)

    def build_vf(self):
        """vertex->face incidence and the edge-adjacent face table
        (``util/mesh.py:152-187``)."""
        nv, nf = len(self.vs), len(self.faces)
        flat = self.faces.reshape(-1)
        fid = np.repeat(np.arange(nf, dtype=np.int64), 3)
        self.vf_ptr, self.vf_idx = _csr_from_pairs(flat, fid, nv)

        # group the 3F half-edges by undirected edge
        key = self._he_key
        order = np.argsort(key, kind="stable")
        ks = key[order]
        start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        sizes = np.diff(np.r_[start, len(ks)])
        he_face = order // 3
        he_slot = order % 3
        nbr = np.full((nf, 3), -1, dtype=np.int64)
        if (sizes > 2).any():
            # non-manifold edge: every face on it sees >= 2 neighbours across one edge
            raise ValueError(
                "non-manifold edge (shared by more than two faces): the face-adjacency "
                "table f2f is [F,3] (util/mesh.py:176-187)")
        two = start[sizes == 2]
        fa_, fb_ = he_face[two], he_face[two + 1]
        sa_, sb_ = he_slot[two], he_slot[two + 1]
        nbr[fa_, sa_] = fb_
        nbr[fb_, sb_] = fa_
        # a face sharing all three vertices (duplicate face) is met across >1 edge: not a
        # neighbour (reference keeps only count == 2)
        dup01 = (nbr[:, 0] >= 0) & (nbr[:, 0] == nbr[:, 1])
        dup02 = (nbr[:, 0] >= 0) & (nbr[:, 0] == nbr[:, 2])
        dup12 = (nbr[:, 1] >= 0) & (nbr[:, 1] == nbr[:, 2])
        bad = np.zeros((nf, 3), dtype=bool)
        bad[:, 0] = dup01 | dup02
        bad[:, 1] = dup01 | dup12
        bad[:, 2] = dup02 | dup12
        nbr[bad] = -1
        # compact valid entries to the left, keep relative order
        valid = nbr >= 0
        rank = np.argsort(~valid, axis=1, kind="stable")
        self.f2f = np.take_along_axis(nbr, rank, axis=1)
        vmask = self.f2f >= 0
        rows = np.repeat(np.arange(nf, dtype=np.int64), 3).reshape(nf, 3)[vmask]
        self.f_edges = np.stack([rows, self.f2f[vmask]], axis=0)

    # ------------------------------------------------ lazy reference-shaped views
    @property
    def vf(self):
        """list of sets, as ``util/mesh.py:153-158`` (built on first use: half a million
        Python sets are not something the hot path should pay for)."""
        if self._vf is None:
            p, i = self.vf_ptr, self.vf_idx
            self._vf = [set(i[p[v]:p[v + 1]].tolist()) for v in range(len(self.vs))]
        return self._vf

    @property
    def v2f_mat(self):
        """sparse [V,F] incidence of ones (``util/mesh.py:171-173``)."""
        if self._v2f_mat is None:
            nv, nf = len(self.vs), len(self.faces)
            rows = np.repeat(np.arange(nv, dtype=np.int64), np.diff(self.vf_ptr))
            inds = torch.from_numpy(np.stack([rows, self.vf_idx]))
            self._v2f_mat = torch.sparse_coo_tensor(
                inds, torch.ones(inds.shape[1], dtype=torch.float32), size=(nv, nf))
        return self._v2f_mat

"""Cases, references and the comparison rule for csrc/loss.hip and csrc/eval.hip past one grid pass, on one- and two-face
meshes, for every parity of `bnfloop`, and at ties / degenerate geometry (tests/test_loss_cases_cpu.py without a GPU,
tests/test_gpu_losses.py on one).  Test infrastructure only.

References.  The five losses, their weighted total and both gradients are the oracle's own functions (oracle/ddmp_oracle.py)
evaluated in float64 on the float32 bits the kernels are given; the same functions in float32 are the yardstick of what any
float32 arithmetic can reach.  sigma_c, the bilateral filter, the vertex update and (through the oracle) face normals / MAD
are plain float64 numpy restatements of the formulas in the kernels' comments.

Comparison rule (`check_gradient`).  The L1 terms make both gradients discontinuous where a sign argument is within rounding
of zero, so single rows may differ by a whole +-coefficient in any float32 arithmetic:
  * a row is OFF when any of its components differs from float64 by more than OFF_TOL * max|ref64| (or is not finite);
  * in every consecutive block of BLOCK rows (the last one merged into its predecessor when shorter than MERGE_BELOW) at most
    OFF_SHARE of the rows may be off -- a wrong grid stride corrupts whole blocks, knife edges are spread evenly;
  * off rows must be finite;
  * over the other rows, rel-L2 <= max(floor, MARGIN x the float32 oracle's rel-L2 over ITS other rows); the floor is 1e-5, or
    1e-4 with the bilateral filter in the gradient (the golden tests' bounds), MARGIN = 4 the project's allowance for another
    valid float32 operation order.
Scalars: rel 1e-5 against float64, 1e-9 for the float64-accumulated L1 and L3.

Two cases could not be run as first written, because the float32 ORACLE does not pass them either:
  * tri2 at an even `bnfloop`: two faces that are each other's only neighbour get their own normal back, so L4 (1.1e-8 in
    float64) and the sign that is all of its gradient are decided below float32 resolution: `filter_returns_input`.  L4 is
    held to that resolution, the filter's part of dnorm to its largest possible size, and the same case runs with the gate
    closed, where all of dnorm is compared;
  * "half the vertices shifted by +200" does not make the centroid weights underflow: sigma_c is a mean over all 3F slots and
    grows with the gap (largest exponent 7.4).  `gap200` is kept as it is, `spike200` (one vertex shifted) does underflow.
"""
import types

import numpy as np
import torch

import oracle_jobs

DEFAULT_K = oracle_jobs.DEFAULT_K
CAD_K = (3.0, 0.0, 3.0, 4.0, 2.0)           # k2 == 0: the c2 == 0 skip of vertex_bwd
BLOCK, MERGE_BELOW = 65536, 16384
OFF_TOL, OFF_SHARE, MARGIN = 1.0e-3, 1.0e-3, 4.0
FLOOR, FLOOR_BNF = 1.0e-5, 1.0e-4
SCALAR_RTOL = (1e-9, 1e-5, 1e-9, 1e-5, 1e-5, 1e-5)          # L1 .. L5, total

# name -> ((nx, ny) of synth.open_grid, bnfloops).  V = nx ny, F = 2 (nx - 1)(ny - 1).
SIZE_GRIDS = {
    "e65k": ((129, 257), (1, 4)),           # F = 65,536: the last element of the reducers' first trip (kNB * 256)
    "x65k": ((258, 257), (5,)),             # F = 131,584: reducers' second trips, bnf_diff (3F elements) on its seventh
    "e524k": ((513, 513), (2,)),            # F = 524,288: last first-trip element of the 2,048-block kernels; 3F = three trips
    "x524k": ((726, 725), (2,)),            # F = 1,049,800, V = 526,350: every kernel of both files past its first trip
    "loops": ((12, 9), (0, 1, 2, 3, 4, 5)),  # ping-pong parity of the BNF backward, and loop = 0
}
SMALL = ("tri1", "tri2")
SMALL_LOOPS = (1, 2)


# ------------------------------------------------------------------------------------ cases
class Case:
    """A mesh (targets: ``mesh.vs`` / ``mesh.fn``, float64) and float32 predictions ``pos`` [V,3] / ``norm`` [F,3]."""

    def __init__(self, name, mesh, pos, norm):
        self.name, self.mesh = name, mesh
        self.pos = np.ascontiguousarray(pos, dtype=np.float32)
        self.norm = np.ascontiguousarray(norm, dtype=np.float32)
        self.V, self.F = len(mesh.vs), len(mesh.faces)
        assert self.pos.shape == (self.V, 3) and self.norm.shape == (self.F, 3)
        self._refs = {}

    def ref(self, dtype, loop, k=DEFAULT_K, gate4=1.0):
        """The oracle's run in ``dtype`` (cached: computed once, never modified)."""
        key = (dtype, int(loop), tuple(k), float(gate4))
        if key not in self._refs:
            r = oracle_run(self, dtype, loop, k, gate4)
            for a in (r.scalars, r.dpos, r.dnorm):
                a.setflags(write=False)
            self._refs[key] = r
        return self._refs[key]


def mean_edge(mesh):
    from dual_dmp_amd import synth
    return synth.mean_edge_length(np.asarray(mesh.vs), np.asarray(mesh.edges))


def predict(mesh, seed):
    """vs + 0.3 mean-edge Gaussian noise; fn + 0.3 noise, normalised."""
    rng = np.random.default_rng(seed)
    pos = mesh.vs + 0.3 * mean_edge(mesh) * rng.standard_normal(mesh.vs.shape)
    n = mesh.fn + 0.3 * rng.standard_normal(mesh.fn.shape)
    return pos, n / np.linalg.norm(n, axis=1, keepdims=True)


def mesh_of(vs, faces, seed=3):
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    v, f = synth.permute_vertices(np.asarray(vs, dtype=np.float64), np.asarray(faces, dtype=np.int64), seed)
    return Mesh(vs=v, faces=f)


def grid_vf(nx=12, ny=9):
    from dual_dmp_amd import synth
    return synth.open_grid(nx, ny)


def size_case(name):
    (nx, ny), _ = SIZE_GRIDS[name]
    m = mesh_of(*grid_vf(nx, ny))
    assert (len(m.vs), len(m.faces)) == (nx * ny, 2 * (nx - 1) * (ny - 1))
    return Case(name, m, *predict(m, 7))


def small_case(name):
    if name == "tri1":                      # every f2f slot is -1: the face gathers itself as "the last face"
        vs, faces = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.2, 0.9, -0.1]], [[0, 1, 2]]
    else:                                   # two triangles across one edge, not coplanar
        vs, faces = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.9, 0.5]], [[0, 1, 2], [1, 3, 2]]
    m = mesh_of(vs, faces)
    assert (m.f2f >= 0).sum() == {"tri1": 0, "tri2": 2}[name]
    return Case(name, m, *predict(m, 11))


def _adjacent_vertices(mesh, n):
    """n mutually adjacent vertices of an interior face."""
    f = int(np.flatnonzero((mesh.f2f >= 0).all(1))[0])
    return [int(x) for x in mesh.faces[f][:n]]


def degenerate_case(name):
    """Inputs on the 176-face grid that `main4real` / `preprocess` accept and the golden meshes never reach."""
    v, f = grid_vf()
    if name in ("scale1e-3", "scale1e3", "offset1000"):
        v = {"scale1e-3": v * 1.0e-3, "scale1e3": v * 1.0e3, "offset1000": v + 1000.0}[name]
        m = mesh_of(v, f)
        return Case(name, m, *predict(m, 13))
    if name in ("collapse2", "collapse3"):           # zero-area PREDICTED faces: 2 / 3 adjacent vertices at one position
        m = mesh_of(v, f)
        pos, nrm = predict(m, 13)
        ids = _adjacent_vertices(m, int(name[-1]))
        pos[ids] = pos[ids[0]]
        c = Case(name, m, pos, nrm)
        c.collapsed = ids
        return c
    if name in ("gap200", "spike200"):
        # gap200: half the vertices shifted by +200 in x.  sigma_c is a mean over ALL 3F slots, the 48 that cross the gap and the
        # 38 boundary slots that gather the last face included, so it grows with the gap (18.4 here) and the largest
        # fcd / 2 sigma_c^2 is 7.4 -- and at most ~22 for any gap on this grid: small weights (6e-4), no underflow.
        # spike200: ONE interior vertex shifted instead; sigma_c stays at 2.4 and its fan's weights underflow expf (ratio > 104).
        v = v.copy()
        if name == "gap200":
            v[v[:, 0] >= 6.0, 0] += 200.0
        else:
            v[np.flatnonzero((v[:, 0] == 5.0) & (v[:, 1] == 4.0))[0], 0] += 200.0
        m = mesh_of(v, f)
        return Case(name, m, *predict(m, 13))
    raise KeyError(name)


DEGENERATE = ("scale1e-3", "scale1e3", "offset1000", "collapse2", "collapse3", "gap200", "spike200")


def zero_area_faces(case):
    """Faces of ``case`` with two equal predicted corners (bit for bit)."""
    p = case.pos[case.mesh.faces]
    same = lambda a, b: (p[:, a] == p[:, b]).all(1)
    return np.flatnonzero(same(0, 1) | same(1, 2) | same(0, 2))


def tie_case():
    """A planar patch with dyadic coordinates (integers / 8, z = 0), real == pred bit for bit, every normal and target
    normal (0, 0, 1): every sign argument of L1 / L3 / L5 is an exact 0 in float32 and in float64."""
    nx, ny = 7, 6
    rng = np.random.default_rng(5)
    x, y = np.meshgrid(np.arange(nx) * 8, np.arange(ny) * 8, indexing="ij")
    jit = rng.integers(-2, 3, size=(2, nx, ny))                           # keeps every triangle's orientation
    vs = np.stack([(x + jit[0]) / 8.0, (y + jit[1]) / 8.0, np.zeros((nx, ny))], -1).reshape(-1, 3)
    _, faces = grid_vf(nx, ny)
    m = mesh_of(vs, faces)
    up = np.tile(np.array([0.0, 0.0, 1.0]), (len(m.faces), 1))
    assert np.array_equal(m.fn, up) and np.array_equal(m.vs.astype(np.float32).astype(np.float64), m.vs)
    m.fn = up                                                             # (+0.0 in x and y, whatever the cross product's sign)
    return Case("ties", m, m.vs, up)


# ------------------------------------------------------------------------------------ oracle wrappers
Ref = types.SimpleNamespace


def oracle_mesh(mesh, dtype):
    """oracle_jobs.oracle_inputs' pattern: the float64 run gets double v2v_mat / v_dims."""
    return types.SimpleNamespace(vs=mesh.vs, fn=mesh.fn, faces=mesh.faces, f2f=mesh.f2f,
                                 v2v_mat=mesh.v2v_mat.to(dtype), v_dims=mesh.v_dims.to(dtype))


def oracle_terms(case, dtype, loop):
    """-> (pos leaf, norm leaf, [L1 .. L5]) with L4 ungated, from the float32 bits of the case in ``dtype``."""
    o = oracle_jobs.load_oracle()
    m = oracle_mesh(case.mesh, dtype)
    pos = torch.from_numpy(case.pos).to(dtype).requires_grad_(True)
    nrm = torch.from_numpy(case.norm).to(dtype).requires_grad_(True)
    terms = [o.pos_rec_loss(pos, m.vs), o.mesh_laplacian_loss(pos, m.v2v_mat, m.v_dims), o.norm_rec_loss(nrm, m.fn),
             o.fn_bnf_loss(pos, nrm, m.faces, m.f2f, loop=loop)[0], o.pos_norm_loss(pos, nrm, m.faces, len(m.vs))]
    return pos, nrm, terms


def _grads(out, pos, nrm):
    g = torch.autograd.grad(out, [pos, nrm], allow_unused=True)
    return [(torch.zeros_like(l) if x is None else x).double().numpy() for x, l in zip(g, (pos, nrm))]


def oracle_run(case, dtype, loop, k=DEFAULT_K, gate4=1.0):
    """-> Ref(scalars [L1..L5 (L4 ungated), total] float64, dpos [V,3], dnorm [F,3] float64 arrays) of main.py:94-106."""
    pos, nrm, t = oracle_terms(case, dtype, loop)
    total = k[0] * t[0] + k[1] * t[1] + k[2] * t[2] + k[3] * (t[3] * gate4) + k[4] * t[4]
    dpos, dnorm = _grads(total, pos, nrm)
    return Ref(scalars=np.array([float(x.detach()) for x in t] + [float(total.detach())]), dpos=dpos, dnorm=dnorm)


def oracle_part(case, dtype, which, loop=1):
    """One loss alone (which = 0 .. 4) -> (value, dpos, dnorm)."""
    pos, nrm, t = oracle_terms(case, dtype, loop)
    return (float(t[which].detach()),) + tuple(_grads(t[which], pos, nrm))


# ------------------------------------------------------------------------------------ numpy float64 references
def _last_for_missing(f2f):
    f2f = np.asarray(f2f)
    return np.where(f2f < 0, len(f2f) - 1, f2f)


def weight_exponents(case):
    """fcd / 2 sigma_c^2 of every real neighbour slot (float64)."""
    fc = case.pos.astype(np.float64)[case.mesh.faces].sum(1) / 3.0
    nb = case.mesh.f2f
    d = ((fc[_last_for_missing(nb)] - fc[:, None, :]) ** 2).sum(2)[nb >= 0]
    return d / (2.0 * sigma_c_np(case.pos, case.mesh.faces, nb) ** 2)


def sigma_c_np(pos, faces, f2f):
    """lossbuf[11]: mean over all 3F slots of sqrt(|c_j - c_f|^2 + 1e-12), a -1 slot gathering the LAST face."""
    fc = np.asarray(pos, dtype=np.float64)[faces].sum(1) / 3.0
    d = ((fc[_last_for_missing(f2f)] - fc[:, None, :]) ** 2).sum(2)
    return float(np.sqrt(d + 1.0e-12).sum() / d.size)


def bnf_filter_np(pos, norm, faces, f2f, loop):
    """The `loop` filter passes of L4 -> (new normals, L4): weights exp(-|dc|^2 / 2 sigma_c^2) exp(-|dn|^2 / (2 * 0.3^2)) a_j,
    zero on -1 slots; a_f = 0.5 sqrt(|cross|^2 + 1e-12); n <- A / (sqrt(|A|^2 + 1e-12) + 1e-12)."""
    p = np.asarray(pos, dtype=np.float64)
    n0 = np.asarray(norm, dtype=np.float64)
    tri = p[faces]
    fc = tri.sum(1) / 3.0
    fa = 0.5 * np.sqrt((np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]) ** 2).sum(1) + 1.0e-12)
    nb = _last_for_missing(f2f)
    sc = sigma_c_np(p, faces, f2f)
    wc = np.exp(-((fc[nb] - fc[:, None, :]) ** 2).sum(2) / (2.0 * sc * sc)) * fa[nb] * (np.asarray(f2f) >= 0)
    cur = n0
    for _ in range(loop):
        nn = cur[nb]
        w = wc * np.exp(-((nn - cur[:, None, :]) ** 2).sum(2) / (2.0 * 0.3 ** 2))
        A = (w[:, :, None] * nn).sum(1)
        cur = A / (np.sqrt((A * A).sum(1, keepdims=True) + 1.0e-12) + 1.0e-12)
    return cur, float(np.abs(cur - n0).sum() / len(n0))


def vertex_update_np(pos, norm, faces, loop):
    """Per sweep: c_f = centroid of the current positions; p_v += (1 / |F(v)|) sum_{f at v} ((c_f - p_v) . n_f) n_f."""
    p = np.array(pos, dtype=np.float64)
    n = np.asarray(norm, dtype=np.float64)
    cv = np.asarray(faces).reshape(-1)
    nf = np.repeat(n, 3, axis=0)
    cnt = np.bincount(cv, minlength=len(p)).astype(np.float64)
    for _ in range(loop):
        fc = np.repeat(p[faces].sum(1) / 3.0, 3, axis=0)
        t = ((fc - p[cv]) * nf).sum(1)[:, None] * nf
        p = p + np.stack([np.bincount(cv, weights=t[:, c], minlength=len(p)) for c in range(3)], 1) / cnt[:, None]
    return p


def face_normals_np(pos, faces):
    return oracle_jobs.load_oracle().face_normals_np(np.asarray(pos, dtype=np.float64), np.asarray(faces))


def mad_np(n1, n2):
    return oracle_jobs.load_oracle().mad_np(np.asarray(n1, dtype=np.float64), np.asarray(n2, dtype=np.float64))


# ------------------------------------------------------------------------------------ the comparison rule
def blocks(n):
    """[(start, stop)] of consecutive BLOCK-row blocks, the last merged into its predecessor when < MERGE_BELOW."""
    cuts = list(range(0, n, BLOCK)) + [n]
    if len(cuts) > 2 and cuts[-1] - cuts[-2] < MERGE_BELOW:
        del cuts[-2]
    return list(zip(cuts[:-1], cuts[1:]))


def off_rows(got, ref64):
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(got) | (np.abs(got - ref64) > OFF_TOL * np.abs(ref64).max())
    return bad.any(1)


def _rel_l2(a, ref):
    d, r = float(np.linalg.norm(a - ref)), float(np.linalg.norm(ref))
    return 0.0 if d == 0.0 else (d / r if r > 0.0 else float("inf"))


def grade(got, ref64):
    """-> (off mask, worst block's off share, rel-L2 over the rows that are not off)."""
    got = np.asarray(got, dtype=np.float64)
    off = off_rows(got, ref64)
    share = max(float(off[a:b].mean()) for a, b in blocks(len(off)))
    return off, share, _rel_l2(got[~off], np.asarray(ref64)[~off])


def gradient_misses(got, ref64, ref32, floor, what=""):
    """The rule of the module docstring -> (list of misses, {"off": worst block's off share, "rel": rel-L2 over the other rows,
    "bound": its bound, "rel32": the float32 oracle's rel-L2}); prints the figures."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != ref64.shape:
        return ["%s: shape %s, expected %s" % (what, got.shape, ref64.shape)], {}
    off, share, rel = grade(got, ref64)
    _, share32, rel32 = grade(ref32, ref64)
    bound = max(floor, MARGIN * rel32)
    m = {"off": share, "rel": rel, "bound": bound, "rel32": rel32, "off32": share32}
    print("%-30s off %.2e (cap %.0e, float32 oracle %.2e)  rel-L2 %.2e (bound %.2e, float32 oracle %.2e)"
          % (what, share, OFF_SHARE, share32, rel, bound, rel32))
    miss = []
    if not np.isfinite(got).all():
        miss.append("%s: non-finite rows %s" % (what, np.flatnonzero(~np.isfinite(got).all(1))[:8]))
    for a, b in blocks(len(off)):
        if off[a:b].sum() > OFF_SHARE * (b - a):
            miss.append("%s: %d of rows %d:%d are off (cap %g)" % (what, int(off[a:b].sum()), a, b, OFF_SHARE * (b - a)))
    if not rel <= bound:
        miss.append("%s: rel-L2 %.3e over the rows that are not off > %.3e" % (what, rel, bound))
    return miss, m


def check_gradient(got, ref64, ref32, floor, what=""):
    miss, m = gradient_misses(got, ref64, ref32, floor, what)
    assert not miss, miss
    return m


def scalar_misses(got, ref64, what="", names=("L1", "L2", "L3", "L4", "L5", "total"), rtol=SCALAR_RTOL):
    got, ref64 = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(ref64, dtype=np.float64))
    print("%-30s %s" % (what, "  ".join("%s %.9g (float64 %.9g, rel %.1e)" % (n, g, r, abs(g - r) / abs(r) if r else abs(g))
                                        for n, g, r in zip(names, got, ref64))))
    return ["%s: %s = %.17g, float64 %.17g, rel %.2e > %g" % (what, n, g, r, abs(g - r) / abs(r) if r else np.inf, tol)
            for n, g, r, tol in zip(names, got, ref64, rtol) if not (np.isfinite(g) and abs(g - r) <= tol * abs(r))]


def filter_returns_input(case, loop):
    """Two faces that are each other's only neighbour swap normals in every pass, so an even number of passes hands every face
    its own normal back, shrunk by the 1e-12 epsilons: in float64 L4 is ~1e-8 and sign(n_last - n0), which is ALL of L4's
    gradient, is decided below the float32 resolution of the operands.  The float32 oracle is 0.35 rel from float64 in L4 there
    and has both rows of dnorm off; no float32 arithmetic can do otherwise (see `_sign_noise_misses`)."""
    return case.name == "tri2" and loop > 0 and loop % 2 == 0


L4_RESOLUTION = 1.0e-6     # |n_last - n0|_1 of unit float32 vectors after the ~8 roundings of sqrtf / reciprocal / scale in two
#                            passes: 8 x 2^-24 x sqrt(3) = 8.3e-7


def _sign_noise_misses(got_scalars, got_dnorm, case, loop, k, gate4, what):
    """`filter_returns_input` cases: L1, L2, L3, L5 and the total as everywhere; L4 to the float32 resolution of its operands.
    With the filter in the gradient, dnorm = (its value with the gate closed) + G0 - c4 s for a sign vector s in {-1, 0, 1}^3F
    that rounding picks: G0 is c4 s pulled back through passes that are projections (norm <= 1) on unit normals, so the filter's
    part is at most c4 (1 + sqrt(3F)) per component (c4 = k4 gate4 / F), and finite.  The same case with the gate closed is
    compared in full (ENGINE_RUNS)."""
    r64 = case.ref(torch.float64, loop, k, gate4)
    got = np.asarray(got_scalars, dtype=np.float64)
    keep = [0, 1, 2, 4, 5]
    miss = scalar_misses(got[keep], r64.scalars[keep], what, ("L1", "L2", "L3", "L5", "total"), [SCALAR_RTOL[i] for i in keep])
    print("%-30s L4 %.3e (float64 %.3e): below the float32 resolution of its operands" % (what, got[3], r64.scalars[3]))
    if not abs(got[3] - r64.scalars[3]) <= L4_RESOLUTION:
        miss.append("%s: L4 = %.3e, float64 %.3e" % (what, got[3], r64.scalars[3]))
    c4 = k[3] * gate4 / case.F
    if c4 != 0.0:
        part = np.asarray(got_dnorm, dtype=np.float64) - case.ref(torch.float64, loop, k, 0.0).dnorm
        cap = c4 * (1.0 + np.sqrt(3.0 * case.F))
        print("%-30s the filter's part of dnorm: max |.| %.3e (cap %.3e)" % (what, np.abs(part).max(), cap))
        if not (np.isfinite(part).all() and np.abs(part).max() <= cap * (1.0 + OFF_TOL)):
            miss.append("%s dnorm: the filter's part %s exceeds c4 (1 + sqrt(3F)) = %g" % (what, part.tolist(), cap))
    return miss


def run_misses(got_scalars, got_dpos, got_dnorm, case, loop, k=DEFAULT_K, gate4=1.0, what=""):
    """One forward_backward (or its autograd equivalent) against the case's two oracle runs -> (misses, figures): every figure is
    printed and every bound looked at before the caller asserts."""
    r64, r32 = case.ref(torch.float64, loop, k, gate4), case.ref(torch.float32, loop, k, gate4)
    what = what or "%s loop %d" % (case.name, loop)
    with_bnf = k[3] * gate4 != 0.0 and loop > 0
    noise = filter_returns_input(case, loop)
    miss = (_sign_noise_misses(got_scalars, got_dnorm, case, loop, k, gate4, what) if noise
            else scalar_misses(got_scalars, r64.scalars, what))
    m1, f1 = gradient_misses(got_dpos, r64.dpos, r32.dpos, FLOOR, what + " dpos")
    m2, f2 = ([], {}) if noise and with_bnf else gradient_misses(got_dnorm, r64.dnorm, r32.dnorm,
                                                                   FLOOR_BNF if with_bnf else FLOOR, what + " dnorm")
    return miss + m1 + m2, {"dpos": f1, "dnorm": f2}


def check_run(*a, **kw):
    miss, figures = run_misses(*a, **kw)
    assert not miss, miss
    return figures


# ------------------------------------------------------------------------------------ one build per session
_CASES = {}


def case(name):
    """The named case, built once (the large meshes and their oracle runs are shared by every test that needs them)."""
    if name not in _CASES:
        _CASES[name] = (size_case(name) if name in SIZE_GRIDS else small_case(name) if name in SMALL
                        else tie_case() if name == "ties" else degenerate_case(name))
    return _CASES[name]


def loops_of(name):
    return SIZE_GRIDS[name][1] if name in SIZE_GRIDS else SMALL_LOOPS if name in SMALL else (1,)


# (case, loop, k, gate4) of every LossEngine.forward_backward comparison
ENGINE_RUNS = [(n, l, DEFAULT_K, 1.0) for n in list(SIZE_GRIDS) + list(SMALL) + list(DEGENERATE) for l in loops_of(n)]
ENGINE_RUNS += [(n, loops_of(n)[0], k, g) for n in ("x65k", "x524k") for k, g in ((CAD_K, 1.0), (DEFAULT_K, 0.0))]
ENGINE_RUNS += [("tri2", 2, DEFAULT_K, 0.0)]                     # `filter_returns_input`: dnorm in full with the gate closed


def run_id(r):
    n, l, k, g = r
    return "%s-loop%d%s%s" % (n, l, "-cad" if k == CAD_K else "", "-gate0" if g == 0.0 else "")

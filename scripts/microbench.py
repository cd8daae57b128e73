#!/usr/bin/env python3
"""Kernel micro-benchmarks at bench scale (HIP-event timing); also the target of rocprofv3 --pmc runs.
usage: microbench.py [gemm|spmm|bn|hd|cheb|sddmm|gat|gatv2|transformer|resgated|feast|edge|gmm|spline|sage|pna|gen|cg|ppf|all] [--rows N] [--iters K]
ppf (not part of all): the point-pair launches (ops.ppf_entries on its own; ops.gather_max_attr with and without the winners' store,
ops.gather_max_attr_bwd with and without the 8-row partials, the gatv2_datt column sum of the partials) at C = 64, 128
on the vertex graph of a torus with --rows vertices in RCB order with one loop per node, alternating in one loop with
ops.gather_max / ops.gather_max_bwd at the same width; the figures, the algorithmic byte counts and the size of the partials go to
--out (profiles/ppf_microbench.txt).
cg (not part of all): the crystal-gate launches (ops.cgate_fwd with the root block, cgate_bwd_row with and without the partials,
cgate_bwd_node with the root block's gradient) at C = 64, 128 and dim = 0, 3 on the vertex graph of a torus with --rows
vertices in RCB order, without loops, each alternating in one loop with the rgate_* launch of the same role at the same width; then
the torch edge-list composition on the same inputs and its autograd backward; the figures, the algorithmic byte counts and each
launch's achieved rate on them go to --out (profiles/cg_microbench.txt).
gen (not part of all): the softmax-aggregation launches (ops.gather_softmax, ops.gather_softmax_bwd) at C = 32, 64, 128,
256 on the same graph as sage, alternating in one loop: the forward (with and without the lse store) against the single-mean
ops.gather_stats with root at the same width, and the backward launch against ops.gather_stats_bwd; the figures and the algorithmic
byte counts go to --out (profiles/gen_microbench.txt).
pna (not part of all): the neighbour-moments launches (ops.gather_moments, ops.gather_moments_bwd) at C = 64, 128, 256
on the same graph as sage, alternating in one loop: the fused mean + min + max + std forward (plain and tower-major) against
ops.gather_stats(mean + max + min) plus the two-launch composition of the variance from the gather_stats means of x and of x * x, and
the backward launch against ops.gather_stats_bwd; the figures and the algorithmic byte counts go to --out
(profiles/pna_microbench.txt).
sage (not part of all): the neighbour-statistics launches (ops.gather_stats, ops.gather_stats_bwd) at C = 64, 128,
256 on the vertex graph of a torus with --rows vertices in RCB order, without loops, alternating in one loop: the fused mean + max
and mean + max + min forward against the composition of ops.gather_max and one single-statistic launch per remaining aggregator,
the single mean with root and bias against ops.gmm_fwd at K = 1, and the backward launch against ops.gather_max_bwd; the figures
and the algorithmic byte counts go to --out (profiles/sage_microbench.txt).
spline (not part of all): the two B-spline launches (ops.spline_fwd with the root block and the bias, ops.spline_bwd_node with dR;
DESIGN.md 4.15) with dim = 3 and kernel_size 2 and 5 on the vertex graph of a torus with --rows vertices in RCB order, without loops,
each alternating in one loop with gmm_fwd / gmm_bwd_node at K = 8 (the number of blocks an edge selects) on the same graph and
width; then the torch edge-list composition on the same inputs (the basis, a [E, 8, C] block gather, multiply, sum, index_add_) and
its autograd backward; the figures, the algorithmic byte counts and each launch's achieved rate on them go to --out
(profiles/spline_microbench.txt).
resgated (not part of all): the per-channel gate launches (ops.rgate_fwd with the skip and the bias, rgate_bwd_row, rgate_bwd_node
with dS) on the vertex graph of a torus with --rows vertices in RCB order, without loops, at the --widths, each
alternating in one loop with the tconv_* launch of the same role at heads=1 and the same width and with the valued ops.spmm; then
the torch composition on the same inputs (index_select x3, sigmoid, multiply, index_add_) and its autograd backward; the figures,
the algorithmic byte counts and each launch's achieved rate on them go to --out (profiles/resgated_microbench.txt).
transformer (not part of all): the dot-product attention launches (ops.tconv_fwd with the skip, tconv_bwd_edge, tconv_bwd_node with
dS) on the same graph and at the same (heads, C) as gatv2, each alternating in one loop with the gatv2_* launch of
the same role and the valued ops.spmm at the same total width; the figures and the algorithmic byte counts go to --out
(profiles/transformer_microbench.txt).
gatv2 (not part of all): the dynamic-attention launches (ops.gatv2_fwd, gatv2_bwd_edge, gatv2_bwd_node, gatv2_datt)
on the same graph and at the same (heads, C) as gat, each alternating in one loop with the gat_* launch of the same role and the
valued ops.spmm at the same total width; the figures and the algorithmic byte counts go to --out (profiles/gatv2_microbench.txt).
gmm (not part of all): the Gaussian-mixture launches (ops.gmm_fwd, gmm_bwd_edge, gmm_bwd_node and the feast_dc column sum of the
[N, 2 K dim] partials) with dim = 3 on the same torus without loops, each alternating in one loop with the valued
ops.spmm at the gathered width K * C and with the feast_* launch of the same role at the same (heads, C); the figures and the
algorithmic byte counts go to --out (profiles/gmm_microbench.txt).
edge (not part of all): the two max-aggregation launches (ops.gather_max with and without arg, ops.gather_max_bwd)
at C = 64, 128, 512 on the same torus without loops, against the valued ops.spmm at the same width, alternating in one loop; the
figures and the algorithmic byte counts go to --out (profiles/edge_microbench.txt).
feast (not part of all): the feature-steered launches (ops.feast_fwd, feast_bwd_edge, feast_bwd_node, feast_dc) on
the same graph as gat, against the valued ops.spmm at the gathered width heads * C, alternating in one loop; the figures and the
algorithmic byte counts go to --out (profiles/feast_microbench.txt).
gat (not part of all): the graph-attention launches (ops.gat_scores, gat_fwd, gat_bwd_edge, gat_bwd_node, gat_datt)
on the vertex graph of a torus with --rows vertices in RCB order, against the valued ops.spmm at the same total width on the same
graph, alternating in one loop; the figures and the algorithmic byte counts go to --out (profiles/gat_microbench.txt).
spmm --weighted (instead of the forms above): the gather on a VALUED graph (edge_weight) against the unvalued graph
of the same mesh, and its transpose, alternating in one loop like cheb.
sddmm (not part of all): the per-entry gradient ops.sddmm on the valued face and vertex graphs against (a) ops.spmm on the same
graph and width and (b) the torch composition that materialises [entries, C]; also the host structure build, set_values and
graph_weight_grad.
cheb (not part of all): one Chebyshev step T_k = a S T_{k-1} + c T_{k-2} on the norm="sym" face and vertex graphs of a torus with
--rows faces in RCB order -- the fused kernel (ops.spmm_axpby, 3 streams of N x C) against the composition it replaces (ops.spmm
into a temporary + one torch elementwise pass, 5 streams), alternating in the same loop, one HIP-event pair per launch, median
of --iters (at least 20) repetitions, rotating buffer sets so that no launch finds its operands in the 256 MB MALL.
hd (not part of all): surface-distance grid build and queries on torus(1000, 500) (1M faces), native and randomly
permuted vertex order, with and without the counting sort of the queries; CPU brute-force rate from a subset."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dual_dmp_amd import ops, synth
from dual_dmp_amd.mesh import Mesh

ap = argparse.ArgumentParser()
ap.add_argument("what", nargs="?", default="all")
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--order", default="native")
ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"])
ap.add_argument("--flip", type=int, default=0, help="rounds of random edge flips (irregular valence)")
ap.add_argument("--widths", default="512,256,128,64,32")
ap.add_argument("--rotate", type=int, default=1, help="spmm: cycle through this many (input, output) buffer sets so that narrow "
                "widths are not served from the 256 MB MALL (a 1M x 32 float tensor is 128 MB)")
ap.add_argument("--weighted", action="store_true", help="spmm: valued graph against the unvalued graph of the same mesh")
ap.add_argument("--out", default=None, help="gat / gatv2 / transformer / resgated / feast / edge / gmm / spline / sage / pna / gen: the file the figures are written to (default profiles/<what>_microbench.txt)")
a = ap.parse_args()
dev = torch.device("cuda:0")
n = a.rows
DT = torch.bfloat16 if a.dtype == "bf16" else torch.float32
ES = 2 if a.dtype == "bf16" else 4


def timeit(fn, iters=a.iters):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3     # us


if a.what in ("gemm", "all"):
    for K, M in ((512, 512), (256, 256), (256, 512), (512, 256), (128, 256)):
        A = torch.randn(n, K, device=dev); W = torch.randn(M, K, device=dev) / K ** 0.5
        G = torch.randn(n, M, device=dev)
        sc = torch.rand(K, device=dev) + 0.5; sh = torch.randn(K, device=dev)
        Y = torch.empty(n, M, device=dev); X = torch.empty(n, K, device=dev); dW = torch.empty(M, K, device=dev)
        fl = 2.0 * n * K * M
        for name, fn in (("nt", lambda: ops.gemm_nt(A, W, out=Y)), ("nt+pro", lambda: ops.gemm_nt(A, W, out=Y, pro=(sc, sh))),
                         ("nn", lambda: ops.gemm_nn(G, W, out=X)), ("tn", lambda: ops.gemm_tn(G, A, out=dW)),
                         ("tn+pro", lambda: ops.gemm_tn(G, A, out=dW, pro=(sc, sh)))):
            us = timeit(fn)
            print("gemm_%-7s K=%3d M=%3d  %8.0f us  %6.1f TF-eq" % (name, K, M, us, fl / us / 1e6))

if a.what in ("spmm", "all") and not a.weighted:
    nu = int(round((n / 2.0) ** 0.5)) if a.what == "spmm_v" else None
    # face graph of a torus with n faces (deg 3+1) and vertex graph with n/2 verts (deg 6+1)
    nv_ = int(round((n / 4.0) ** 0.5)); nu_ = n // (2 * nv_)
    v, f = synth.torus(nu_, nv_)
    if a.flip:
        f = synth.flip_edges(v, f, rounds=a.flip, seed=1)
        f = synth.add_hub(v, f, 1234, 24)
    if a.order == "rcb":
        v, f = synth.rcb_relabel(v, f)
    elif a.order == "random":
        v, f = synth.permute_vertices(v, f, 0); f = synth.permute_faces(f, 0)
    elif a.order == "morton":
        v, f = synth.morton_relabel(v, f)
    m = Mesh(vs=v, faces=f)
    e = torch.tensor(m.edges.T, dtype=torch.long); ei = torch.cat([e, e[[1, 0]]], 1).to(dev)
    fi = torch.from_numpy(m.f_edges).to(dev)
    for gname, idx, nn_ in (("face", fi, len(f)), ("vert", ei, len(v))):
        g = ops.graph_for(idx, nn_)
        for C in [int(c) for c in a.widths.split(",")]:
            if a.rotate > 1:                                     # cold-cache figures: every launch works on another buffer set
                R = a.rotate
                Xs = [torch.randn(nn_, C, device=dev).to(DT) for _ in range(R)]
                Ys = [torch.empty(nn_, C, device=dev, dtype=DT) for _ in range(R)]
                Yps = [torch.randn(nn_, C, device=dev).to(DT) for _ in range(R)]
                sc = torch.rand(C, device=dev) + 0.5; sh = torch.randn(C, device=dev)
                bn4 = torch.rand(4, C, device=dev) + 0.5; c10 = torch.rand(2, C, device=dev) * 0.1
                sums = torch.empty(2 * C, dtype=torch.float64, device=dev); ref0 = torch.zeros(C, device=dev)
                k = [0]

                def rot(fn):
                    def go():
                        i = k[0] % R; k[0] += 1
                        fn(Xs[i], Ys[i], Yps[i])
                    return go
                it = max(a.iters, 2 * R)
                t = {name: timeit(rot(fn), it) for name, fn in (
                    ("plain", lambda X, Y, Yp: ops.spmm(g, X, out=Y)),
                    ("prologue", lambda X, Y, Yp: ops.spmm(g, X, out=Y, pro=(sc, sh))),
                    ("statistics", lambda X, Y, Yp: ops.spmm_stats(g, X, Y, ref0, sums, bias=sh)),
                    ("reduction", lambda X, Y, Yp: ops.spmm_bnred(g, X, Y, Yp, bn4, sums)),
                    ("bn-backward", lambda X, Y, Yp: ops.spmm_bnbwd(g, X, Yp, bn4, c10, Y)))}
                b2, b3 = 2.0 * nn_ * C * ES, 3.0 * nn_ * C * ES
                print("spmm %s N=%d C=%3d  cold (%d buffer sets): " % (gname, nn_, C, R) + "   ".join(
                    "%s %5.0f us (%.2f TB/s)" % (nm, us, (b3 if nm in ("reduction", "bn-backward") else b2) / us / 1e6) for nm, us in t.items()), flush=True)
                del Xs, Ys, Yps
                continue
            X = torch.randn(nn_, C, device=dev).to(DT); Y = torch.empty(nn_, C, device=dev, dtype=DT)
            us = timeit(lambda: ops.spmm(g, X, out=Y))
            alg = 2.0 * nn_ * C * ES + 4.0 * g.nnz + 8.0 * nn_
            print("spmm %s N=%d C=%3d  %8.0f us  %7.1f GB/s alg (%.1f%% of 8 TB/s)  gather-logical %.1f GB/s" % (
                gname, nn_, C, us, alg / us / 1e3, alg / us / 1e3 / 80.0, (g.nnz * C * 4.0 + nn_ * C * 4.0) / us / 1e3))
            if C >= 32:
                sc = torch.rand(C, device=dev) + 0.5; sh = torch.randn(C, device=dev)
                us_p = timeit(lambda: ops.spmm(g, X, out=Y, pro=(sc, sh)))
                sums0 = torch.empty(2 * C, dtype=torch.float64, device=dev); ref0 = torch.zeros(C, device=dev)
                us_t = timeit(lambda: ops.spmm_stats(g, X, Y, ref0, sums0, bias=sh))
                bn4 = torch.rand(4, C, device=dev) + 0.5; sums = torch.empty(2 * C, dtype=torch.float64, device=dev)
                Yp = torch.randn(nn_, C, device=dev).to(DT)
                us_r = timeit(lambda: ops.spmm_bnred(g, X, Y, Yp, bn4, sums))
                c10 = torch.rand(2, C, device=dev) * 0.1
                us_b = timeit(lambda: ops.spmm_bnbwd(g, X, Yp, bn4, c10, Y))
                dY = torch.empty_like(X)
                us_a = timeit(lambda: ops.bn_bwd_apply(X, Yp, bn4, c10, dY, sums))
                us_s = timeit(lambda: ops.bn_bwd_reduce(X, Yp, bn4, sums2=sums))
                print("     +statistics %8.0f us (x%.2f)" % (us_t, us_t / us))
                print("     +prologue %8.0f us (x%.2f)   +bn-backward reduce %8.0f us (x%.2f; separate pass %.0f us)   "
                      "bn-backward on the gather %8.0f us (apply pass %.0f us + plain)" % (us_p, us_p / us, us_r, us_r / us, us_s, us_b, us_a))

if a.what in ("bn", "all"):
    for C in (512, 256):
        Y = torch.randn(n, C, device=dev); dZ = torch.randn(n, C, device=dev); dY = torch.empty(n, C, device=dev)
        sums = torch.empty(2 * C, dtype=torch.float64, device=dev)
        bn4 = torch.rand(4, C, device=dev) + 0.5; c10 = torch.rand(2, C, device=dev)
        for name, fn, by in (("stats", lambda: ops.bn_stats(Y, sums=sums), 4.0), ("bwd_reduce", lambda: ops.bn_bwd_reduce(dZ, Y, bn4, sums2=sums), 8.0),
                             ("bwd_apply", lambda: ops.bn_bwd_apply(dZ, Y, bn4, c10, dY, sums), 12.0)):
            us = timeit(fn)
            print("bn_%-10s C=%3d %8.0f us  %7.1f GB/s" % (name, C, us, by * n * C / us / 1e3))

if a.what == "hd":
    import time
    from dual_dmp_amd import evaluate
    from dual_dmp_amd.evaluate import SurfaceDistance
    tv, tf = synth.torus(1000, 500)
    gt, noisy, _ = synth.make_triplet(tv, tf, steps=1)
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(tv)); inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
    for order in ("native", "permuted"):
        A, B = (noisy.vs, gt.vs) if order == "native" else (noisy.vs[perm], gt.vs[perm])
        F_ = tf if order == "native" else inv[tf]
        pa = torch.from_numpy(A.astype(np.float32)).to(dev); pb = torch.from_numpy(B.astype(np.float32)).to(dev)
        sa, sb = SurfaceDistance(pa, F_, dev), SurfaceDistance(pb, F_, dev)
        us_b = timeit(lambda: sb.update(pb))
        print("hd %-8s F=%d grid build %8.0f us" % (order, len(tf), us_b))
        for sort in (False, True):
            us_ab = timeit(lambda: sb.query(pa, sort=sort))
            us_ba = timeit(lambda: sa.query(pb, sort=sort))
            print("hd %-8s sort=%d  noisy->gt %8.0f us  gt->noisy %8.0f us" % (order, sort, us_ab, us_ba))
        sort = evaluate.SORT_QUERIES
        us_t = timeit(lambda: (sa.update(pa), sb.update(pb), sb.query(pa, sort=sort), sa.query(pb, sort=sort)))
        print("hd %-8s two-sided (2 builds + 2 queries, sort=%d) %8.0f us" % (order, sort, us_t))
    # meshes that do not overlap (an output in another frame): the queries start outside the grid box
    diag = float(np.linalg.norm(gt.vs.max(0) - gt.vs.min(0)))
    far = torch.from_numpy((noisy.vs + (2.0 * diag, 0.0, 0.0)).astype(np.float32)).to(dev)
    sg = SurfaceDistance(torch.from_numpy(gt.vs.astype(np.float32)).to(dev), tf, dev)
    print("hd disjoint (noisy moved by 2 bbox diagonals) -> gt %8.0f us" % timeit(lambda: sg.query(far)))
    # CPU brute force: float64 numpy, 16 queries against all 1M triangles, extrapolated to V queries per direction
    a0, b0, c0 = (gt.vs[tf[:, k]] for k in range(3))
    n_ = np.cross(b0 - a0, c0 - a0)
    t0 = time.perf_counter()
    for q in noisy.vs[:16]:
        ap = q - a0
        s = (ap * n_).sum(1)                                         # plane distance + 3 segment distances per triangle
        for u, w in ((a0, b0), (b0, c0), (c0, a0)):
            d = w - u; t = np.clip(((q - u) * d).sum(1) / (d * d).sum(1), 0, 1)
            e = q - u - t[:, None] * d; (e * e).sum(1)
    dt = (time.perf_counter() - t0) / 16
    print("hd cpu brute force (numpy f64, 1 thread-ish): %.3f s per query -> %.0f s per direction at V=%d" % (dt, dt * len(tv), len(tv)))

if a.what == "cheb":
    nv_ = int(round((n / 4.0) ** 0.5)); nu_ = n // (2 * nv_)
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    m = Mesh(vs=v, faces=f)
    e = torch.tensor(m.edges.T, dtype=torch.long); ei = torch.cat([e, e[[1, 0]]], 1).to(dev)
    fi = torch.from_numpy(m.f_edges).to(dev)
    reps = max(a.iters, 20)
    ca, cc = -1.0, 1.0                                           # lambda_max = 2: L^ = -S; one addend, b = 0
    for gname, idx, nn_ in (("face", fi, len(f)), ("vert", ei, len(v))):
        g = ops.graph_for(idx, nn_, norm="sym")
        for C in [int(c) for c in a.widths.split(",")]:
            R = 2 if nn_ * C * 4 >= (1 << 29) else 4
            Xs, Zs, Ys = ([torch.randn(nn_, C, device=dev) for _ in range(R)] for _ in range(3))
            tmp = torch.empty(nn_, C, device=dev)

            def fused(i):
                ops.spmm_axpby(g, Xs[i], out=Ys[i], z=Zs[i], a=ca, c=cc)

            def composed(i):
                ops.spmm(g, Xs[i], out=tmp)
                torch.add(Zs[i], tmp, alpha=ca, out=Ys[i])       # c = 1: ONE elementwise pass (reads tmp, Z, writes Y)

            composed(0); ref = Ys[0].clone(); fused(0)
            err = float((Ys[0] - ref).double().norm() / ref.double().norm())
            t = {"fused": [], "composed": []}
            for r in range(3 + reps):                            # 3 warm-up rounds, then alternating
                for name, fn in (("fused", fused), ("composed", composed)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(r % R); e1.record(); torch.cuda.synchronize()
                    if r >= 3:
                        t[name].append(e0.elapsed_time(e1) * 1e3)
            q = {k: np.percentile(np.array(v_), [0, 25, 50, 75, 100]) for k, v_ in t.items()}
            b3 = 3.0 * nn_ * C * 4 + 4.0 * g.nnz + 8.0 * nn_
            print("cheb step %s N=%d C=%3d (%d buffer sets, %d reps): fused %6.0f us [min %.0f q1 %.0f q3 %.0f max %.0f]  composed %6.0f us "
                  "[min %.0f q1 %.0f q3 %.0f max %.0f]  fused/composed %.3f  fused: %.2f TB/s on the 3-stream count = %.1f%% of 8 TB/s  "
                  "rel-L2 fused vs composed %.1e" % (gname, nn_, C, R, reps, q["fused"][2], q["fused"][0], q["fused"][1], q["fused"][3],
                  q["fused"][4], q["composed"][2], q["composed"][0], q["composed"][1], q["composed"][3], q["composed"][4],
                  q["fused"][2] / q["composed"][2], b3 / q["fused"][2] / 1e6, b3 / q["fused"][2] / 1e6 / 8.0 * 100.0, err), flush=True)
            del Xs, Zs, Ys, tmp


def alternate(fns, reps, R):
    """fns: {name: fn(buffer set)}: 3 warm-up rounds, then `reps` rounds of every fn in rotating order, one HIP-event pair per launch ->
    {name: percentiles [min, q1, median, q3, max] in us}."""
    t = {k: [] for k in fns}
    names = list(fns)
    for r in range(3 + reps):
        # (the forms of a round read the same buffer set: whoever runs second finds part of it in the 256 MB MALL -- the starting
        # form rotates so that no form is always first)
        for name in names[r % len(names):] + names[:r % len(names)]:
            fn = fns[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(r % R); e1.record(); torch.cuda.synchronize()
            if r >= 3:
                t[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: np.percentile(np.array(v_), [0, 25, 50, 75, 100]) for k, v_ in t.items()}


def fmt(q):
    return "%6.0f us [min %.0f q1 %.0f q3 %.0f max %.0f]" % (q[2], q[0], q[1], q[3], q[4])


if (a.what == "spmm" and a.weighted) or a.what == "sddmm":
    import time
    nv_ = int(round((n / 4.0) ** 0.5)); nu_ = n // (2 * nv_)
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    m = Mesh(vs=v, faces=f)
    e = torch.tensor(m.edges.T, dtype=torch.long); ei = torch.cat([e, e[[1, 0]]], 1).to(dev)
    fi = torch.from_numpy(m.f_edges).to(dev)
    reps = max(a.iters, 20)
    for gname, idx, nn_ in (("face", fi, len(f)), ("vert", ei, len(v))):
        w = torch.rand(idx.shape[1], device=dev) + 0.25
        torch.cuda.synchronize(); t0 = time.perf_counter()
        gv = ops.graph_for(idx, nn_, edge_weight=w)
        torch.cuda.synchronize(); t_build = time.perf_counter() - t0
        g0 = ops.graph_for(idx, nn_)
        w2 = [torch.rand(idx.shape[1], device=dev) + 0.25 for _ in range(2)]
        q = alternate({"set_values": lambda i: gv.set_values(w2[i], validate=False)}, reps, 2)
        gv.set_values(w)
        print("valued graph %s N=%d entries=%d: structure build + upload + first values %.2f s (host, once); set_values %s"
              % (gname, nn_, gv.nnz, t_build, fmt(q["set_values"])), flush=True)
        for C in [int(c) for c in a.widths.split(",")]:
            R = 2 if nn_ * C * 4 >= (1 << 29) else 4
            Xs, Ys = ([torch.randn(nn_, C, device=dev) for _ in range(R)] for _ in range(2))
            Out = torch.empty(nn_, C, device=dev)
            alg = 2.0 * nn_ * C * 4 + 4.0 * gv.nnz + 8.0 * nn_
            if a.what == "spmm":
                q = alternate({"unvalued": lambda i: ops.spmm(g0, Xs[i], out=Out), "valued": lambda i: ops.spmm(gv, Xs[i], out=Out),
                               "transpose": lambda i: ops.spmm(gv, Xs[i], out=Out, transpose=True)}, reps, R)
                print("spmm weighted %s N=%d C=%3d (%d buffer sets, %d reps): unvalued %s  valued %s  transpose %s  valued/unvalued %.3f  "
                      "valued: %.2f TB/s alg = %.1f%% of 8 TB/s" % (gname, nn_, C, R, reps, fmt(q["unvalued"]), fmt(q["valued"]),
                      fmt(q["transpose"]), q["valued"][2] / q["unvalued"][2], alg / q["valued"][2] / 1e6, alg / q["valued"][2] / 1e6 / 8.0 * 100.0),
                      flush=True)
            else:
                G = torch.empty(gv.nnz, device=dev)
                t = ops.csr_build_valued_host(idx.cpu().numpy(), nn_, ops.valued_flags())
                row = torch.from_numpy(np.repeat(np.arange(nn_), np.diff(t["rowptr"]))).to(dev)
                col = torch.from_numpy(t["col"]).long().to(dev)
                fns = {"sddmm": lambda i: ops.sddmm(gv, Ys[i], Xs[i], out=G), "spmm": lambda i: ops.spmm(gv, Xs[i], out=Out)}
                if gv.nnz * C * 4 * 3 < (20 << 30):
                    fns["torch"] = lambda i: (Ys[i][row] * Xs[i][col]).sum(1)
                q = alternate(fns, reps, R)
                ref = (Ys[0][row].double() * Xs[0][col].double()).sum(1) if C <= 128 else None
                ops.sddmm(gv, Ys[0], Xs[0], out=G)
                err = float((G.double() - ref).norm() / ref.norm()) if ref is not None else float("nan")
                alg_s = 2.0 * nn_ * C * 4 + 8.0 * gv.nnz + 4.0 * nn_
                print("sddmm %s N=%d C=%3d (%d buffer sets, %d reps): sddmm %s = %.2f TB/s alg (%.1f%% of 8 TB/s; %.0f MB)  spmm %s  "
                      "sddmm/spmm %.3f  torch composition %s  rel-L2 vs float64 %.1e" % (gname, nn_, C, R, reps, fmt(q["sddmm"]),
                      alg_s / q["sddmm"][2] / 1e6, alg_s / q["sddmm"][2] / 1e6 / 8.0 * 100.0, alg_s / 1e6, fmt(q["spmm"]),
                      q["sddmm"][2] / q["spmm"][2], fmt(q["torch"]) if "torch" in q else "(skipped: memory)", err), flush=True)
                del G, row, col
            del Xs, Ys, Out
        if a.what == "sddmm":
            G = torch.randn(gv.nnz, device=dev); dw = torch.empty(idx.shape[1], device=dev)
            q = alternate({"wgrad": lambda i: ops.graph_weight_grad(gv, G, out=dw)}, reps, 1)
            print("graph_weight_grad %s N=%d: %s" % (gname, nn_, fmt(q["wgrad"])), flush=True)


if a.what == "gat":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat")
    reps = max(a.iters, 20)
    lines = ["graph attention on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d (loops included), float32; "
             "median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms alternating in one loop, rotating buffer "
             "sets; bytes = the algorithmic counts of ops.py (MB)" % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    for heads, C in ((4, 128), (8, 32), (1, 64), (8, 4)):
        hc = heads * C
        R = 2 if nn_ * hc * 4 >= (1 << 29) else 4
        Hs, Ds = ([torch.randn(nn_, hc, device=dev) for _ in range(R)] for _ in range(2))
        att_s, att_d = torch.randn(heads, C, device=dev) * 0.1, torch.randn(heads, C, device=dev) * 0.1
        Out = torch.empty(nn_, hc, device=dev)
        st = []
        for i in range(R):                                       # the saved state of a forward per buffer set
            s_src, s_dst = ops.gat_scores(Hs[i], att_s, att_d, heads)
            y, alpha = ops.gat_fwd(g, Hs[i], s_src, s_dst, heads, 0.2)
            ds, ds_dst = ops.gat_bwd_edge(g, Ds[i], Hs[i], s_src, s_dst, alpha, heads, 0.2)
            dhf, ds_src = ops.gat_bwd_node(g, Ds[i], alpha, ds, ds_dst, att_s, att_d, heads)
            st.append((s_src, s_dst, alpha, ds, ds_dst, ds_src))
            del y, dhf
        q = alternate({
            "spmm": lambda i: ops.spmm(g, Hs[i], out=Out),
            "scores": lambda i: ops.gat_scores(Hs[i], att_s, att_d, heads),
            "fwd": lambda i: ops.gat_fwd(g, Hs[i], st[i][0], st[i][1], heads, 0.2, out=Out),
            "bwd_edge": lambda i: ops.gat_bwd_edge(g, Ds[i], Hs[i], st[i][0], st[i][1], st[i][2], heads, 0.2),
            "bwd_node": lambda i: ops.gat_bwd_node(g, Ds[i], st[i][2], st[i][3], st[i][4], att_s, att_d, heads),
            "datt": lambda i: ops.gat_datt(Hs[i], st[i][5], st[i][4], heads)}, reps, R)
        feat, ent, node = 4.0 * nn_ * hc, 4.0 * g.nnz, 4.0 * nn_
        alg = {"spmm": 2 * feat + ent + 2 * node, "scores": feat + 2 * node * heads,
               "fwd": 2 * feat + ent * heads + 2 * node * heads + 2 * ent + node,
               "bwd_edge": 2 * feat + 2 * ent * heads + 3 * node * heads + ent + node,
               "bwd_node": 2 * feat + 2 * ent * heads + 2 * node * heads + 2 * ent + node, "datt": feat + 2 * node * heads}
        lines.append("heads=%d C=%d (width %d, %d buffer sets):" % (heads, C, hc, R))
        for k in ("spmm", "scores", "fwd", "bwd_edge", "bwd_node", "datt"):
            lines.append("  %-9s %s  %7.0f MB  %.2f TB/s alg  x%.2f of the valued spmm" % (
                k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6, q[k][2] / q["spmm"][2]))
        print("\n".join(lines[-7:]), flush=True)
        del Hs, Ds, Out, st
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gat_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "gatv2":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat")
    reps = max(a.iters, 20)
    lines = ["dynamic graph attention (GATv2) on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d (loops included), "
             "float32; median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms alternating in one loop, rotating "
             "buffer sets; bytes = the algorithmic counts of ops.py (MB)" % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    for heads, C in ((4, 128), (8, 32), (1, 64), (8, 4)):
        hc = heads * C
        R = 2 if nn_ * hc * 4 >= (1 << 29) else 4
        Hs, Rs, Ds = ([torch.randn(nn_, hc, device=dev) for _ in range(R)] for _ in range(3))
        att, att_d = torch.randn(heads, C, device=dev) * 0.1, torch.randn(heads, C, device=dev) * 0.1
        Out, Out2 = torch.empty(nn_, hc, device=dev), torch.empty(nn_, hc, device=dev)
        st = []
        for i in range(R):                                       # the saved state of a forward per buffer set, both operators
            s_src, s_dst = ops.gat_scores(Hs[i], att, att_d, heads)
            y, alpha1 = ops.gat_fwd(g, Hs[i], s_src, s_dst, heads, 0.2)
            ds, ds_dst = ops.gat_bwd_edge(g, Ds[i], Hs[i], s_src, s_dst, alpha1, heads, 0.2)
            y, alpha = ops.gatv2_fwd(g, Hs[i], Rs[i], att, heads, 0.2)
            dz, dxr, part = ops.gatv2_bwd_edge(g, Ds[i], Hs[i], Rs[i], att, alpha, heads, 0.2)
            st.append((s_src, s_dst, alpha1, ds, ds_dst, alpha, dz, part))
            del y, dxr
        q = alternate({
            "spmm": lambda i: ops.spmm(g, Hs[i], out=Out),
            "gat_fwd": lambda i: ops.gat_fwd(g, Hs[i], st[i][0], st[i][1], heads, 0.2, out=Out),
            "fwd": lambda i: ops.gatv2_fwd(g, Hs[i], Rs[i], att, heads, 0.2, out=Out),
            "gat_bwd_edge": lambda i: ops.gat_bwd_edge(g, Ds[i], Hs[i], st[i][0], st[i][1], st[i][2], heads, 0.2),
            "bwd_edge": lambda i: ops.gatv2_bwd_edge(g, Ds[i], Hs[i], Rs[i], att, st[i][5], heads, 0.2, out=Out),
            "bwd_edge_nodatt": lambda i: ops.gatv2_bwd_edge(g, Ds[i], Hs[i], Rs[i], att, st[i][5], heads, 0.2, out=Out, want_datt=False),
            "gat_bwd_node": lambda i: ops.gat_bwd_node(g, Ds[i], st[i][2], st[i][3], st[i][4], att, att_d, heads),
            "bwd_node": lambda i: ops.gatv2_bwd_node(g, Ds[i], Hs[i], Rs[i], att, st[i][5], st[i][6], heads, 0.2, out=Out2),
            "datt": lambda i: ops.gatv2_datt(st[i][7], heads)}, reps, R)
        feat, ent, node = 4.0 * nn_ * hc, 4.0 * g.nnz, 4.0 * nn_
        alg = {"spmm": 2 * feat + ent + 2 * node,
               "gat_fwd": 2 * feat + ent * heads + 2 * node * heads + 2 * ent + node,
               "fwd": 3 * feat + ent * heads + 2 * ent + node,
               "gat_bwd_edge": 2 * feat + 2 * ent * heads + 3 * node * heads + ent + node,
               "bwd_edge": 5 * feat + 2 * ent * heads + ent + node, "bwd_edge_nodatt": 4 * feat + 2 * ent * heads + ent + node,
               "gat_bwd_node": 2 * feat + 2 * ent * heads + 2 * node * heads + 2 * ent + node,
               "bwd_node": 4 * feat + 2 * ent * heads + 2 * ent + node, "datt": feat}
        base = {"fwd": "gat_fwd", "bwd_edge": "gat_bwd_edge", "bwd_edge_nodatt": "gat_bwd_edge", "bwd_node": "gat_bwd_node"}
        lines.append("heads=%d C=%d (width %d, %d buffer sets):" % (heads, C, hc, R))
        for k in q:
            tail = "  x%.2f of %s" % (q[k][2] / q[base[k]][2], base[k]) if k in base else ""
            lines.append("  %-15s %s  %7.0f MB  %.2f TB/s alg  x%.2f of the valued spmm%s" % (
                k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6, q[k][2] / q["spmm"][2], tail))
        print("\n".join(lines[-(len(q) + 1):]), flush=True)
        del Hs, Rs, Ds, Out, Out2, st
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gatv2_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "transformer":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat")                       # the gatv2 mode's graph (loops included), for all three operators
    reps = max(a.iters, 20)
    lines = ["graph transformer (TransformerConv) on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d (loops "
             "included, the gatv2 mode's graph), float32; median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms "
             "alternating in one loop, rotating buffer sets; bytes = the algorithmic counts of ops.py (MB)" % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    for heads, C in ((4, 128), (8, 32), (1, 64), (8, 4)):
        hc = heads * C
        R = 2 if nn_ * hc * 4 >= (1 << 29) else 4
        Qs, Ks, Vs, Ss, Ds = ([torch.randn(nn_, hc, device=dev) for _ in range(R)] for _ in range(5))
        att = torch.randn(heads, C, device=dev) * 0.1
        Out, Out2, Out3 = (torch.empty(nn_, hc, device=dev) for _ in range(3))
        st = []
        for i in range(R):                                       # the saved state of a forward per buffer set, both operators
            y, alpha2 = ops.gatv2_fwd(g, Ks[i], Qs[i], att, heads, 0.2)
            dz2, dxr, _ = ops.gatv2_bwd_edge(g, Ds[i], Ks[i], Qs[i], att, alpha2, heads, 0.2, want_datt=False)
            y, alpha = ops.tconv_fwd(g, Qs[i], Ks[i], Vs[i], heads, skip=Ss[i])
            dz, dq = ops.tconv_bwd_edge(g, Ds[i], Ks[i], Vs[i], alpha, heads)
            st.append((alpha2, dz2, alpha, dz))
            del y, dxr, dq
        q = alternate({
            "spmm": lambda i: ops.spmm(g, Vs[i], out=Out),
            "gatv2_fwd": lambda i: ops.gatv2_fwd(g, Ks[i], Qs[i], att, heads, 0.2, out=Out),
            "fwd": lambda i: ops.tconv_fwd(g, Qs[i], Ks[i], Vs[i], heads, skip=Ss[i], out=Out),
            "gatv2_bwd_edge": lambda i: ops.gatv2_bwd_edge(g, Ds[i], Ks[i], Qs[i], att, st[i][0], heads, 0.2, out=Out, want_datt=False),
            "bwd_edge": lambda i: ops.tconv_bwd_edge(g, Ds[i], Ks[i], Vs[i], st[i][2], heads, out=Out),
            "gatv2_bwd_node": lambda i: ops.gatv2_bwd_node(g, Ds[i], Ks[i], Qs[i], att, st[i][0], st[i][1], heads, 0.2, out=Out2),
            "bwd_node": lambda i: ops.tconv_bwd_node(g, Ds[i], Qs[i], st[i][2], st[i][3], heads, out_k=Out, out_v=Out2, out_s=Out3)},
            reps, R)
        feat, ent, node = 4.0 * nn_ * hc, 4.0 * g.nnz, 4.0 * nn_
        alg = {"spmm": 2 * feat + ent + 2 * node,
               "gatv2_fwd": 3 * feat + ent * heads + 2 * ent + node, "fwd": 5 * feat + ent * heads + 2 * ent + node,
               "gatv2_bwd_edge": 4 * feat + 2 * ent * heads + ent + node, "bwd_edge": 4 * feat + 2 * ent * heads + ent + node,
               "gatv2_bwd_node": 4 * feat + 2 * ent * heads + 2 * ent + node, "bwd_node": 5 * feat + 2 * ent * heads + 2 * ent + node}
        base = {"fwd": "gatv2_fwd", "bwd_edge": "gatv2_bwd_edge", "bwd_node": "gatv2_bwd_node"}
        lines.append("heads=%d C=%d (width %d, %d buffer sets):" % (heads, C, hc, R))
        for k in q:
            tail = "  x%.2f of %s" % (q[k][2] / q[base[k]][2], base[k]) if k in base else ""
            lines.append("  %-15s %s  %7.0f MB  %.2f TB/s alg  x%.2f of the valued spmm%s" % (
                k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6, q[k][2] / q["spmm"][2], tail))
        print("\n".join(lines[-(len(q) + 1):]), flush=True)
        del Qs, Ks, Vs, Ss, Ds, Out, Out2, Out3, st
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "transformer_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "resgated":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat", add_self_loops=False)  # the operator's graph (no loops), for both operators
    src, dst = ei[0], ei[1]
    reps = max(a.iters, 20)
    lines = ["residual gated graph convolution (ResGatedGraphConv) on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d "
             "(no loops), float32; median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms alternating in one loop, "
             "rotating buffer sets; bytes = the algorithmic counts of ops.py (MB); tconv_* = the dot-product attention launches at "
             "heads=1 and the same width on the same graph (the in-tree yardstick); torch = index_select x3, sigmoid, multiply, "
             "index_add_ on the same inputs (forward) and its autograd backward, mean of 3 runs"
             % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    for C in [int(c) for c in a.widths.split(",")]:
        R = 2 if nn_ * C * 4 >= (1 << 29) else 4
        Ks, Qs, Vs, Ss, Ds = ([torch.randn(nn_, C, device=dev) for _ in range(R)] for _ in range(5))
        bias = torch.randn(C, device=dev)
        Out, Out2, Out3 = (torch.empty(nn_, C, device=dev) for _ in range(3))
        st = []
        for i in range(R):                                       # the saved state of the attention forward per buffer set
            y, alpha = ops.tconv_fwd(g, Qs[i], Ks[i], Vs[i], 1, skip=Ss[i])
            dz, dq = ops.tconv_bwd_edge(g, Ds[i], Ks[i], Vs[i], alpha, 1)
            st.append((alpha, dz))
            del y, dq
        q = alternate({
            "spmm": lambda i: ops.spmm(g, Vs[i], out=Out),
            "tconv_fwd": lambda i: ops.tconv_fwd(g, Qs[i], Ks[i], Vs[i], 1, skip=Ss[i], out=Out),
            "fwd": lambda i: ops.rgate_fwd(g, Ks[i], Qs[i], Vs[i], skip=Ss[i], bias=bias, out=Out),
            "tconv_bwd_edge": lambda i: ops.tconv_bwd_edge(g, Ds[i], Ks[i], Vs[i], st[i][0], 1, out=Out),
            "bwd_row": lambda i: ops.rgate_bwd_row(g, Ds[i], Ks[i], Qs[i], Vs[i], out=Out),
            "tconv_bwd_node": lambda i: ops.tconv_bwd_node(g, Ds[i], Qs[i], st[i][0], st[i][1], 1, out_k=Out, out_v=Out2, out_s=Out3),
            "bwd_node": lambda i: ops.rgate_bwd_node(g, Ds[i], Ks[i], Qs[i], Vs[i], out_q=Out, out_v=Out2, out_s=Out3)},
            reps, R)
        feat, ent, node = 4.0 * nn_ * C, 4.0 * g.nnz, 4.0 * nn_
        alg = {"spmm": 2 * feat + ent + 2 * node,
               "tconv_fwd": 5 * feat + 3 * ent + node, "fwd": 5 * feat + 2 * ent + node,
               "tconv_bwd_edge": 4 * feat + 3 * ent + node, "bwd_row": 5 * feat + 2 * ent + node,
               "tconv_bwd_node": 5 * feat + 4 * ent + node, "bwd_node": 7 * feat + 3 * ent + node}
        base = {"fwd": "tconv_fwd", "bwd_row": "tconv_bwd_edge", "bwd_node": "tconv_bwd_node"}
        lines.append("C=%d (%d buffer sets):" % (C, R))
        for k in q:
            tail = "  x%.2f of %s" % (q[k][2] / q[base[k]][2], base[k]) if k in base else ""
            lines.append("  %-15s %s  %7.0f MB  %.2f TB/s alg = %4.1f%% of 8 TB/s  x%.2f of the valued spmm%s" % (
                k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6, alg[k] / q[k][2] / 1e6 / 8.0 * 100.0, q[k][2] / q["spmm"][2], tail))
        # the torch composition on the same inputs: five [E, C] tensors and an index_add_, and its autograd backward
        kk, qq_, vv_ = (t.clone().requires_grad_(True) for t in (Ks[0], Qs[0], Vs[0]))

        def torch_fwd():
            gate = torch.sigmoid(kk.index_select(0, dst) + qq_.index_select(0, src))
            return torch.zeros_like(vv_).index_add_(0, dst, gate * vv_.index_select(0, src)) + Ss[0] + bias

        t_f = timeit(lambda: torch_fwd().detach(), 3)
        yt = torch_fwd()
        t_b = timeit(lambda: torch.autograd.grad(yt, (kk, qq_, vv_), Ds[0], retain_graph=True), 3)
        ours_b = q["bwd_row"][2] + q["bwd_node"][2]
        err = float((ops.rgate_fwd(g, Ks[0], Qs[0], Vs[0], skip=Ss[0], bias=bias) - yt.detach()).norm() / yt.detach().norm())
        lines.append("  torch forward %8.0f us = x%.1f of fwd;  torch backward %8.0f us = x%.1f of bwd_row + bwd_node (%.0f us);  "
                     "rel-L2 fwd vs torch %.1e" % (t_f, t_f / q["fwd"][2], t_b, t_b / ours_b, ours_b, err))
        print("\n".join(lines[-(len(q) + 2):]), flush=True)
        del Ks, Qs, Vs, Ss, Ds, Out, Out2, Out3, st, kk, qq_, vv_, yt
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resgated_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "cg":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat", add_self_loops=False)
    src, dst = ei[0], ei[1]
    reps = max(a.iters, 20)
    lines = ["crystal graph convolution (CGConv) on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d = input edges "
             "(no loops, no duplicates), float32, aggr=add; median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms "
             "alternating in one loop, rotating buffer sets; bytes = the algorithmic counts of ops.py (MB); rgate_* = the residual-gate "
             "launches at the same width on the same graph (two gathered streams, one gate: the in-tree yardstick); bwd_row-P = the "
             "row side without the partials; torch = index_select x4, the attribute products, sigmoid, softplus, multiply, "
             "index_add_ on the same inputs (forward) and its autograd backward, mean of 3 runs" % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    for C in (64, 128):
        for dim in (0, 3):
            R = 2 if nn_ * C * 4 >= (1 << 29) else 4
            Af, As, Bf, Bs, Rs, Ds = ([torch.randn(nn_, C, device=dev) for _ in range(R)] for _ in range(6))
            bias = torch.randn(C, device=dev)
            Out, Out2, Out3 = (torch.empty(nn_, C, device=dev) for _ in range(3))
            attr = torch.randn(ei.shape[1], dim, device=dev) if dim else None
            ef, es = (torch.randn(dim, C, device=dev) * 0.5 for _ in range(2)) if dim else (None, None)
            kw = dict(attr=attr, ef=ef, es=es)
            fns = {
                "rgate_fwd": lambda i: ops.rgate_fwd(g, Af[i], Bf[i], Bs[i], skip=Rs[i], bias=bias, out=Out),
                "fwd": lambda i: ops.cgate_fwd(g, Af[i], As[i], Bf[i], Bs[i], root=Rs[i], out=Out, **kw),
                "rgate_bwd_row": lambda i: ops.rgate_bwd_row(g, Ds[i], Af[i], Bf[i], Bs[i], out=Out),
                "bwd_row": lambda i: ops.cgate_bwd_row(g, Ds[i], Af[i], As[i], Bf[i], Bs[i], out_f=Out, out_s=Out2, **kw),
                "rgate_bwd_node": lambda i: ops.rgate_bwd_node(g, Ds[i], Af[i], Bf[i], Bs[i], out_q=Out, out_v=Out2, out_s=Out3),
                "bwd_node": lambda i: ops.cgate_bwd_node(g, Ds[i], Af[i], As[i], Bf[i], Bs[i], out_f=Out, out_s=Out2, out_r=Out3, **kw)}
            if dim:
                fns["bwd_row-P"] = lambda i: ops.cgate_bwd_row(g, Ds[i], Af[i], As[i], Bf[i], Bs[i], out_f=Out, out_s=Out2,
                                                               want_parts=False, **kw)
            q = alternate(fns, reps, R)
            feat, ent, node = 4.0 * nn_ * C, 4.0 * g.nnz, 4.0 * nn_
            gb = ent + node + (ent if dim == 0 else ent + ent * (dim + 1) + 8.0 * dim * C)    # ops._cgate_graph_bytes
            alg = {"rgate_fwd": 5 * feat + 2 * ent + node, "fwd": 6 * feat + gb,
                   "rgate_bwd_row": 5 * feat + 2 * ent + node, "bwd_row": (7 + 2 * dim) * feat + gb, "bwd_row-P": 7 * feat + gb,
                   "rgate_bwd_node": 7 * feat + 3 * ent + node, "bwd_node": 8 * feat + gb + ent}
            base = {"fwd": "rgate_fwd", "bwd_row": "rgate_bwd_row", "bwd_row-P": "rgate_bwd_row", "bwd_node": "rgate_bwd_node"}
            lines.append("C=%d dim=%d (%d buffer sets):" % (C, dim, R))
            for k in q:
                tail = "  x%.2f of %s" % (q[k][2] / q[base[k]][2], base[k]) if k in base else ""
                lines.append("  %-15s %s  %7.0f MB  %.2f TB/s alg = %4.1f%% of 8 TB/s%s" % (
                    k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6, alg[k] / q[k][2] / 1e6 / 8.0 * 100.0, tail))
            if dim:
                lines.append("  the partials: %.0f us = %.0f%% of bwd_row for %.0f MB more" % (
                    q["bwd_row"][2] - q["bwd_row-P"][2], 100.0 * (q["bwd_row"][2] - q["bwd_row-P"][2]) / q["bwd_row"][2],
                    2 * dim * feat / 1e6))
            # the torch edge-list composition on the same inputs, and its autograd backward
            leaves = [t.clone().requires_grad_(True) for t in (Af[0], As[0], Bf[0], Bs[0])]

            def torch_fwd():
                pf = leaves[0].index_select(0, dst) + leaves[2].index_select(0, src)
                ps = leaves[1].index_select(0, dst) + leaves[3].index_select(0, src)
                if dim:
                    pf, ps = pf + attr @ ef, ps + attr @ es
                msg = torch.sigmoid(pf) * torch.nn.functional.softplus(ps)
                return torch.zeros_like(leaves[0]).index_add_(0, dst, msg) + Rs[0]

            t_f = timeit(lambda: torch_fwd().detach(), 3)
            yt = torch_fwd()
            t_b = timeit(lambda: torch.autograd.grad(yt, leaves, Ds[0], retain_graph=True), 3)
            ours_b = q["bwd_row"][2] + q["bwd_node"][2]
            err = float((ops.cgate_fwd(g, Af[0], As[0], Bf[0], Bs[0], root=Rs[0], **kw) - yt.detach()).norm() / yt.detach().norm())
            lines.append("  torch forward %8.0f us = x%.1f of fwd;  torch backward %8.0f us = x%.1f of bwd_row + bwd_node (%.0f us);  "
                         "rel-L2 fwd vs torch %.1e" % (t_f, t_f / q["fwd"][2], t_b, t_b / ours_b, ours_b, err))
            print("\n".join(lines[-(len(q) + 2 + (1 if dim else 0)):]), flush=True)
            del Af, As, Bf, Bs, Rs, Ds, Out, Out2, Out3, leaves, yt, attr, ef, es, kw, fns
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cg_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "ppf":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat")
    reps = max(a.iters, 20)
    lines = ["point-pair-feature convolution (PPFConv) on the vertex graph of torus(%d, %d) in RCB order with one loop per node: N=%d, "
             "entries=%d, float32; median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms alternating in one loop, "
             "rotating buffer sets; bytes = the algorithmic counts of ops.py (MB); gather_max / gather_max_bwd = the arg-max gather "
             "without an edge term at the same width on the same graph (the in-tree yardstick; its backward also writes the dA "
             "copy); fwd-arg = without the winners' store; bwd-P = without the partials" % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    pos = torch.tensor(np.asarray(v), dtype=torch.float32, device=dev)
    nrm = torch.randn(nn_, 3, device=dev)
    nrm = nrm / nrm.norm(dim=1, keepdim=True)
    P2 = [pos.clone() for _ in range(2)]

    def entries(i):
        g._ppf = None                                            # (defeat the cache: time the launch)
        return ops.ppf_entries(g, P2[i], nrm)

    q = alternate({"ppf_entries": entries}, reps, 2)
    alg_e = 24.0 * nn_ + 24.0 * g.nnz
    lines.append("ppf_entries        %s  %7.0f MB  %.2f TB/s alg" % (fmt(q["ppf_entries"]), alg_e / 1e6, alg_e / q["ppf_entries"][2] / 1e6))
    print(lines[-1], flush=True)
    F = ops.ppf_entries(g, pos, nrm)
    for C in (64, 128):
        R = 2 if nn_ * C * 4 >= (1 << 29) else 4
        B, Ds = ([torch.randn(nn_, C, device=dev) for _ in range(R)] for _ in range(2))
        E = torch.randn(4, C, device=dev) * 0.5
        Out = torch.empty(nn_, C, device=dev)
        Out2 = torch.empty(nn_, 2 * C, device=dev)
        _, arg = ops.gather_max_attr(g, B[0], F, E)
        fns = {
            "gather_max": lambda i: ops.gather_max(g, B[i], out=Out),
            "fwd": lambda i: ops.gather_max_attr(g, B[i], F, E, out=Out),
            "fwd-arg": lambda i: ops.gather_max_attr(g, B[i], F, E, out=Out, want_arg=False),
            "gather_max_bwd": lambda i: ops.gather_max_bwd(g, Ds[i], arg, out=Out2),
            "bwd": lambda i: ops.gather_max_attr_bwd(g, Ds[i], arg, F, out=Out),
            "bwd-P": lambda i: ops.gather_max_attr_bwd(g, Ds[i], arg, F, out=Out, want_parts=False)}
        q = alternate(fns, reps, R)
        parts = ops.gather_max_attr_bwd(g, Ds[0], arg, F)[1]
        q.update(alternate({"gatv2_datt": lambda i: ops.gatv2_datt(parts, 4)}, reps, 1))
        feat, ent, node = 4.0 * nn_ * C, 4.0 * g.nnz, 4.0 * nn_
        pbytes = 4.0 * parts.numel()
        alg = {"gather_max": 3 * feat + ent + node, "fwd": 3 * feat + 5 * ent + 16.0 * C + node, "fwd-arg": 2 * feat + 5 * ent + 16.0 * C + node,
               "gather_max_bwd": 4 * feat + ent + node, "bwd": 3 * feat + pbytes + 5 * ent + node, "bwd-P": 3 * feat + ent + node,
               "gatv2_datt": pbytes}
        base = {"fwd": "gather_max", "fwd-arg": "gather_max", "bwd": "gather_max_bwd", "bwd-P": "gather_max_bwd"}
        lines.append("C=%d (%d buffer sets):" % (C, R))
        for k in q:
            tail = "  x%.2f of %s" % (q[k][2] / q[base[k]][2], base[k]) if k in base else ""
            lines.append("  %-15s %s  %7.0f MB  %.2f TB/s alg = %4.1f%% of 8 TB/s%s" % (
                k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6, alg[k] / q[k][2] / 1e6 / 8.0 * 100.0, tail))
        lines.append("  the partials: [N / 8, 4 C] = %.0f MB (per-row partials would be %.0f MB); %.0f us = %.0f%% of bwd" % (
            pbytes / 1e6, 8 * pbytes / 1e6, q["bwd"][2] - q["bwd-P"][2], 100.0 * (q["bwd"][2] - q["bwd-P"][2]) / q["bwd"][2]))
        print("\n".join(lines[-(len(q) + 2):]), flush=True)
        del B, Ds, Out, Out2, arg, parts, fns
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ppf_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "feast":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat")
    reps = max(a.iters, 20)
    lines = ["feature-steered convolution on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d (loops included), "
             "float32; median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms alternating in one loop, rotating "
             "buffer sets; the valued spmm gathers rows of the same width heads * C; bytes = the algorithmic counts of ops.py (MB)"
             % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    for heads, C in ((4, 128), (8, 32), (1, 64), (8, 4)):
        hc = heads * C
        wtp = (hc + heads + 3) // 4 * 4                          # the operator's row buffers: [Hf | P | padding], [dHf | dP | padding]
        R = 2 if nn_ * hc * 4 >= (1 << 29) else 4
        Bs = [torch.randn(nn_, wtp, device=dev) for _ in range(R)]
        Hs, Ps = [b[:, :hc] for b in Bs], [b[:, hc:hc + heads] for b in Bs]
        Ds = [torch.randn(nn_, C, device=dev) for _ in range(R)]
        cvec = torch.randn(heads, device=dev) * 0.5
        Out, Wide, G = torch.empty(nn_, C, device=dev), torch.empty(nn_, hc, device=dev), torch.empty(nn_, wtp, device=dev)
        st = []
        for i in range(R):                                       # the saved state of a forward per buffer set
            y, beta = ops.feast_fwd(g, Hs[i], Ps[i], cvec, heads)
            dz, rs = ops.feast_bwd_edge(g, Ds[i], Hs[i], beta, heads)
            st.append((beta, dz, rs))
            del y
        q = alternate({
            "spmm": lambda i: ops.spmm(g, Hs[i], out=Wide),
            "fwd": lambda i: ops.feast_fwd(g, Hs[i], Ps[i], cvec, heads, out=Out),
            "bwd_edge": lambda i: ops.feast_bwd_edge(g, Ds[i], Hs[i], st[i][0], heads),
            "bwd_node": lambda i: ops.feast_bwd_node(g, Ds[i], st[i][0], st[i][1], st[i][2], heads, out=G),
            "dc": lambda i: ops.feast_dc(st[i][2], heads)}, reps, R)
        wide, narrow, ent, node = 4.0 * nn_ * hc, 4.0 * nn_ * C, 4.0 * g.nnz, 4.0 * nn_
        alg = {"spmm": 2 * wide + ent + 2 * node,
               "fwd": wide + narrow + ent * heads + node * heads + 2 * ent + node,
               "bwd_edge": wide + narrow + 2 * ent * heads + node * heads + ent + node,
               "bwd_node": wide + narrow + 2 * ent * heads + 2 * node * heads + 2 * ent + node,
               "dc": node * heads}
        lines.append("heads=%d C=%d (gathered width %d, %d buffer sets):" % (heads, C, hc, R))
        for k in ("spmm", "fwd", "bwd_edge", "bwd_node", "dc"):
            lines.append("  %-9s %s  %7.0f MB  %.2f TB/s alg  x%.2f of the valued spmm" % (
                k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6, q[k][2] / q["spmm"][2]))
        print("\n".join(lines[-6:]), flush=True)
        del Bs, Hs, Ps, Ds, Out, Wide, G, st
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "feast_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "edge":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat", add_self_loops=False)
    reps = max(a.iters, 20)
    lines = ["max aggregation (EdgeConv) on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d (no loops), float32; "
             "median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms alternating in one loop, rotating buffer "
             "sets; A / B and dA / dB are the halves of one [N, 2 C] row buffer; the valued spmm gathers rows of the same width C; "
             "bytes = the algorithmic counts of ops.py and DESIGN.md 4.10 (MB)" % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    for C in (64, 128, 512):
        R = 2 if nn_ * C * 4 >= (1 << 29) else 4
        Bs = [torch.randn(nn_, 2 * C, device=dev) for _ in range(R)]
        As, Xs = [b[:, :C] for b in Bs], [b[:, C:] for b in Bs]
        Ds = [torch.randn(nn_, C, device=dev) for _ in range(R)]
        Out, G = torch.empty(nn_, C, device=dev), torch.empty(nn_, 2 * C, device=dev)
        args = [ops.gather_max(g, Xs[i], a=As[i])[1] for i in range(R)]          # the saved state of a forward per buffer set
        q = alternate({
            "spmm": lambda i: ops.spmm(g, Xs[i], out=Out),
            "fwd": lambda i: ops.gather_max(g, Xs[i], a=As[i], out=Out),
            "fwd_noarg": lambda i: ops.gather_max(g, Xs[i], a=As[i], out=Out, want_arg=False),
            "bwd": lambda i: ops.gather_max_bwd(g, Ds[i], args[i], out=G)}, reps, R)
        feat, ent, node = 4.0 * nn_ * C, 4.0 * g.nnz, 4.0 * nn_
        alg = {"spmm": 2 * feat + ent + 2 * node, "fwd": 4 * feat + ent + node, "fwd_noarg": 3 * feat + ent + node,
               "bwd": 4 * feat + ent + node}
        lines.append("C=%d (%d buffer sets):" % (C, R))
        for k in ("spmm", "fwd", "fwd_noarg", "bwd"):
            lines.append("  %-9s %s  %7.0f MB  %.2f TB/s alg  x%.2f of the valued spmm" % (
                k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6, q[k][2] / q["spmm"][2]))
        print("\n".join(lines[-5:]), flush=True)
        del Bs, As, Xs, Ds, Out, G, args
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "edge_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "gmm":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat", add_self_loops=False)
    reps = max(a.iters, 20)
    dim = 3
    lines = ["Gaussian-mixture convolution (GMMConv, dim = %d) on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d "
             "(no loops), input edges=%d, float32; median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms "
             "alternating in one loop, rotating buffer sets; the valued spmm gathers rows of the same width K * C, feast_* are the "
             "feature-steered launches of the same role at heads = K on the same graph; [Hf | R] and [dHf | dR] are one row buffer "
             "each; bytes = the algorithmic counts of ops.py (MB)" % (dim, nu_, nv_, nn_, g.nnz, g.nnz_in, reps)]
    print(lines[0], flush=True)
    attr = torch.rand(g.nnz_in, dim, device=dev)
    for K, C in ((4, 128), (8, 32), (1, 64), (8, 4)):
        hc, kd = K * C, K * dim
        wt = hc + C                                              # the operator's row buffers: [Hf | R], [dHf | dR]
        R = 2 if nn_ * hc * 4 >= (1 << 29) else 4
        Bs = [torch.randn(nn_, wt, device=dev) for _ in range(R)]
        Hs, Rs = [b[:, :hc] for b in Bs], [b[:, hc:] for b in Bs]
        Ps = [torch.randn(nn_, K, device=dev) for _ in range(R)]
        Ds = [torch.randn(nn_, C, device=dev) for _ in range(R)]
        mu, sigma = torch.rand(K, dim, device=dev), 0.3 + 0.7 * torch.rand(K, dim, device=dev)
        cvec, bias = torch.randn(K, device=dev) * 0.5, torch.randn(C, device=dev)
        Out, Wide, G = torch.empty(nn_, C, device=dev), torch.empty(nn_, hc, device=dev), torch.empty(nn_, wt, device=dev)
        Gf = torch.empty(nn_, (hc + K + 3) // 4 * 4, device=dev)   # feast's [dHf | dP | padding]
        st = []
        for i in range(R):                                       # the saved state of a forward per buffer set
            y, w = ops.gmm_fwd(g, Hs[i], attr, mu, sigma, K, root=Rs[i], bias=bias)
            parts, _ = ops.gmm_bwd_edge(g, Ds[i], Hs[i], attr, mu, sigma, K)
            y, beta = ops.feast_fwd(g, Hs[i], Ps[i], cvec, K, bias=bias)
            dz, rs = ops.feast_bwd_edge(g, Ds[i], Hs[i], beta, K)
            st.append((w, parts, beta, dz, rs))
            del y
        q = alternate({
            "spmm": lambda i: ops.spmm(g, Hs[i], out=Wide),
            "fwd": lambda i: ops.gmm_fwd(g, Hs[i], attr, mu, sigma, K, root=Rs[i], bias=bias, out=Out),
            "feast_fwd": lambda i: ops.feast_fwd(g, Hs[i], Ps[i], cvec, K, bias=bias, out=Out),
            "bwd_edge": lambda i: ops.gmm_bwd_edge(g, Ds[i], Hs[i], attr, mu, sigma, K),
            "bwd_edge+dattr": lambda i: ops.gmm_bwd_edge(g, Ds[i], Hs[i], attr, mu, sigma, K, want_dattr=True),
            "feast_bwd_edge": lambda i: ops.feast_bwd_edge(g, Ds[i], Hs[i], st[i][2], K),
            "bwd_node": lambda i: ops.gmm_bwd_node(g, Ds[i], st[i][0], K, out=G, root=True),
            "feast_bwd_node": lambda i: ops.feast_bwd_node(g, Ds[i], st[i][2], st[i][3], st[i][4], K, out=Gf),
            "dc": lambda i: ops.feast_dc(st[i][1], 2 * kd)}, reps, R)
        wide, narrow, ent, node, edges = 4.0 * nn_ * hc, 4.0 * nn_ * C, 4.0 * g.nnz, 4.0 * nn_, 4.0 * g.nnz_in
        alg = {"spmm": 2 * wide + ent + 2 * node,
               "fwd": wide + 3 * narrow + ent * K + edges * (dim + 1) + 3 * ent + node,
               "feast_fwd": wide + narrow + ent * K + node * K + 2 * ent + node,
               "bwd_edge": wide + narrow + 2 * ent * K + edges * (dim + 1) + 2 * node * kd + 3 * ent + node,
               "bwd_edge+dattr": wide + narrow + 2 * ent * K + edges * (2 * dim + 1) + 2 * node * kd + 3 * ent + node,
               "feast_bwd_edge": wide + narrow + 2 * ent * K + node * K + ent + node,
               "bwd_node": wide + 2 * narrow + ent * K + 2 * ent + node,
               "feast_bwd_node": wide + narrow + 2 * ent * K + 2 * node * K + 2 * ent + node,
               "dc": 2 * node * kd}
        pair = {"fwd": "feast_fwd", "bwd_edge": "feast_bwd_edge", "bwd_edge+dattr": "feast_bwd_edge", "bwd_node": "feast_bwd_node"}
        lines.append("K=%d C=%d (gathered width %d, %d buffer sets):" % (K, C, hc, R))
        for k in alg:
            extra = ("  x%.2f of %s (bytes x%.2f)" % (q[k][2] / q[pair[k]][2], pair[k], alg[k] / alg[pair[k]])) if k in pair else ""
            lines.append("  %-15s %s  %7.0f MB  %.2f TB/s alg  x%.2f of the valued spmm%s" % (
                k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6, q[k][2] / q["spmm"][2], extra))
        print("\n".join(lines[-(len(alg) + 1):]), flush=True)
        del Bs, Hs, Rs, Ps, Ds, Out, Wide, G, Gf, st
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gmm_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "spline":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    src, dst = ei[0], ei[1]
    g = ops.graph_for(ei, nn_, norm="gat", add_self_loops=False)
    reps = max(a.iters, 20)
    dim, S = 3, 8
    lines = ["B-spline convolution (SplineConv, degree 1, dim = %d, open, mean) on the vertex graph of torus(%d, %d) in RCB order: N=%d, "
             "entries=%d (no loops), input edges=%d, float32; median of %d launches [min q1 q3 max], one HIP-event pair per launch, "
             "forms alternating in one loop, rotating buffer sets; gmm_* are the Gaussian-mixture launches of the same role at K = 8 "
             "(the blocks an edge selects) and the same C on the same graph; [Hf | R] and [dHf | dR] are one row buffer each; bytes = "
             "the algorithmic counts of ops.py (MB): the forward reads S C floats per input edge, not K C; torch = the edge-list "
             "composition (basis, [E, 8, C] block gather, multiply, sum, index_add_, mean) and its autograd backward, mean of 3 runs"
             % (dim, nu_, nv_, nn_, g.nnz, g.nnz_in, reps)]
    print(lines[0], flush=True)
    attr = torch.rand(g.nnz_in, dim, device=dev)
    mu, sigma = torch.rand(8, dim, device=dev), 0.3 + 0.7 * torch.rand(8, dim, device=dev)

    def torch_basis(ksz):
        b = torch.ones(attr.shape[0], S, device=dev)
        k = torch.zeros(attr.shape[0], S, dtype=torch.long, device=dev)
        bits, stride = torch.arange(S, device=dev), 1
        for d in range(dim):
            vv = attr[:, d] * (ksz - 1)
            fl = torch.floor(vv)
            fr, up = (vv - fl).unsqueeze(1), ((bits >> d) & 1).unsqueeze(0)
            b = b * torch.where(up.bool(), fr, 1 - fr)
            k = k + torch.remainder(fl.long().unsqueeze(1) + up, ksz) * stride
            stride *= ksz
        return b, k

    cnt = torch.zeros(nn_, device=dev).index_add_(0, dst, torch.ones(dst.shape[0], device=dev)).clamp(min=1).unsqueeze(1)
    for ksz, C in ((2, 32), (2, 128), (5, 32)):
        ks, op, K = [ksz] * dim, [True] * dim, ksz ** dim
        hc, gc = K * C, 8 * C
        R = 2 if nn_ * hc * 4 >= (1 << 29) else 4
        Bs = [torch.randn(nn_, hc + C, device=dev) for _ in range(R)]
        Hs, Rs = [b[:, :hc] for b in Bs], [b[:, hc:] for b in Bs]
        Gb = Bs if K == 8 else [torch.randn(nn_, gc + C, device=dev) for _ in range(R)]     # gmm's [Hf | R] at K = 8
        GHs, GRs = [b[:, :gc] for b in Gb], [b[:, gc:] for b in Gb]
        Ds = [torch.randn(nn_, C, device=dev) for _ in range(R)]
        bias = torch.randn(C, device=dev)
        Out, G, Gg = torch.empty(nn_, C, device=dev), torch.empty(nn_, hc + C, device=dev), torch.empty(nn_, gc + C, device=dev)
        ws = [ops.gmm_fwd(g, GHs[i], attr, mu, sigma, 8, root=GRs[i], bias=bias)[1] for i in range(R)]
        q = alternate({
            "fwd": lambda i: ops.spline_fwd(g, Hs[i], attr, ks, op, root=Rs[i], bias=bias, out=Out),
            "gmm_fwd": lambda i: ops.gmm_fwd(g, GHs[i], attr, mu, sigma, 8, root=GRs[i], bias=bias, out=Out),
            "bwd_node": lambda i: ops.spline_bwd_node(g, Ds[i], attr, ks, op, C, out=G, root=True),
            "gmm_bwd_node": lambda i: ops.gmm_bwd_node(g, Ds[i], ws[i], 8, out=Gg, root=True)}, reps, R)
        narrow, ent, node, edges = 4.0 * nn_ * C, 4.0 * g.nnz, 4.0 * nn_, 4.0 * g.nnz_in
        alg = {"fwd": edges * S * C + 2 * narrow + edges * (dim + 1) + 2 * ent + node,
               "gmm_fwd": 4.0 * nn_ * gc + 3 * narrow + ent * 8 + edges * (dim + 1) + 3 * ent + node,
               "bwd_node": 4.0 * nn_ * hc + 3 * narrow + edges * (dim + 1) + 3 * ent + node,
               "gmm_bwd_node": 4.0 * nn_ * gc + 2 * narrow + ent * 8 + 2 * ent + node}
        pair = {"fwd": "gmm_fwd", "bwd_node": "gmm_bwd_node"}
        lines.append("kernel_size=%d K=%d C=%d (row width %d, %d buffer sets; gmm at K=8: row width %d):" % (ksz, K, C, hc, R, gc))
        for k_ in alg:
            extra = ("  x%.2f of %s (bytes x%.2f)" % (q[k_][2] / q[pair[k_]][2], pair[k_], alg[k_] / alg[pair[k_]])) if k_ in pair else ""
            lines.append("  %-13s %s  %7.0f MB  %.2f TB/s alg%s" % (k_, fmt(q[k_]), alg[k_] / 1e6, alg[k_] / q[k_][2] / 1e6, extra))
        # the torch edge-list composition on the same inputs, and its autograd backward
        hh = Hs[0].clone().requires_grad_(True)

        def torch_fwd():
            b, k = torch_basis(ksz)
            msg = (b.unsqueeze(-1) * hh.view(nn_, K, C)[src.unsqueeze(1), k]).sum(1)
            return torch.zeros(nn_, C, device=dev).index_add_(0, dst, msg) / cnt + Rs[0] + bias

        t_f = timeit(lambda: torch_fwd().detach(), 3)
        yt = torch_fwd()
        t_b = timeit(lambda: torch.autograd.grad(yt, (hh,), Ds[0], retain_graph=True), 3)
        err = float((ops.spline_fwd(g, Hs[0], attr, ks, op, root=Rs[0], bias=bias) - yt.detach()).norm() / yt.detach().norm())
        lines.append("  torch forward %8.0f us = x%.1f of fwd;  torch backward %8.0f us = x%.1f of bwd_node;  rel-L2 fwd vs torch %.1e"
                     % (t_f, t_f / q["fwd"][2], t_b, t_b / q["bwd_node"][2], err))
        print("\n".join(lines[-(len(alg) + 2):]), flush=True)
        del Bs, Hs, Rs, Gb, GHs, GRs, Ds, Out, G, Gg, ws, hh, yt
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spline_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "sage":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat", add_self_loops=False)
    reps = max(a.iters, 20)
    lines = ["neighbour statistics (SAGEConv) on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d (no loops), float32; "
             "median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms alternating in one loop, rotating buffer "
             "sets; fused = ONE ops.gather_stats launch writing its blocks into one row buffer; composed = ops.gather_max for max + "
             "one single-statistic ops.gather_stats launch per remaining aggregator (the sum of their medians); bytes = the "
             "algorithmic counts of ops.py and DESIGN.md 4.16 (MB)" % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    attr = torch.rand(g.nnz_in, 3, device=dev)
    mu, sigma = torch.rand(1, 3, device=dev), torch.rand(1, 3, device=dev) + 0.5
    for C in (64, 128, 256):
        R = 2 if nn_ * C * 4 >= (1 << 29) else 4
        Bs = [torch.randn(nn_, 2 * C, device=dev) for _ in range(R)]           # [L | R] of the transform-first form
        Xs, Rs = [b[:, :C] for b in Bs], [b[:, C:] for b in Bs]
        Ds = [torch.randn(nn_, 3 * C, device=dev) for _ in range(R)]           # [dS | dMx | dX0]
        bias = torch.randn(C, device=dev)
        O1, O2, O3 = (torch.empty(nn_, k * C, device=dev) for k in (1, 2, 3))
        Oa, Ob = torch.empty(nn_, C, device=dev), torch.empty(nn_, C, device=dev)
        G2 = torch.empty(nn_, 2 * C, device=dev)
        saved = [ops.gather_stats(g, Xs[i], want=("mean", "max")) for i in range(R)]       # the saved state of a forward per buffer set
        amx, inv = [s[1][1] for s in saved], [s[2] for s in saved]
        amx_e = [ops.gather_max(g, Xs[i])[1] for i in range(R)]
        q = alternate({
            "mean": lambda i: ops.gather_stats(g, Xs[i], want=("mean",), out=Oa),
            "min": lambda i: ops.gather_stats(g, Xs[i], want=("min",), out=Ob),
            "gather_max": lambda i: ops.gather_max(g, Xs[i], out=O1),
            "mean+max": lambda i: ops.gather_stats(g, Xs[i], want=("mean", "max"), out=O2),
            "mean+max+min": lambda i: ops.gather_stats(g, Xs[i], want=("mean", "max", "min"), out=O3),
            "mean+root+bias": lambda i: ops.gather_stats(g, Xs[i], want=("mean",), root=Rs[i], bias=bias, out=Oa),
            "gmm_fwd K=1": lambda i: ops.gmm_fwd(g, Xs[i], attr, mu, sigma, 1, root=Rs[i], bias=bias, out=Ob),
            "bwd max": lambda i: ops.gather_stats_bwd(g, dmx=Ds[i][:, C:2 * C], argmx=amx[i], out=Oa),
            "gather_max_bwd": lambda i: ops.gather_max_bwd(g, Ds[i][:, C:2 * C], amx_e[i], out=G2),
            "bwd mean+max+x0": lambda i: ops.gather_stats_bwd(g, ds=Ds[i][:, :C], invdeg=inv[i], dmx=Ds[i][:, C:2 * C], argmx=amx[i],
                                                               dx0=Ds[i][:, 2 * C:], out=Oa),
            "bwd mean+root": lambda i: ops.gather_stats_bwd(g, ds=Ds[i][:, :C], invdeg=inv[i], root=True, out=G2)}, reps, R)
        feat, ent, node = 4.0 * nn_ * C, 4.0 * g.nnz, 4.0 * nn_
        alg = {"mean": 2 * feat + 2 * ent + 2 * node, "min": 3 * feat + 2 * ent + node, "gather_max": 3 * feat + ent + node,
               "mean+max": 4 * feat + 2 * ent + 2 * node, "mean+max+min": 6 * feat + 2 * ent + 2 * node,
               "mean+root+bias": 3 * feat + 2 * ent + 2 * node, "gmm_fwd K=1": 3 * feat + ent + 4.0 * g.nnz_in * 4 + 3 * ent + node,
               "bwd max": 3 * feat + 3 * ent + node, "gather_max_bwd": 4 * feat + ent + node,
               "bwd mean+max+x0": 5 * feat + 3 * ent + 2 * node, "bwd mean+root": 4 * feat + 3 * ent + 2 * node}
        lines.append("C=%d (%d buffer sets):" % (C, R))
        for k in alg:
            lines.append("  %-16s %s  %7.0f MB  %.2f TB/s alg" % (k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6))
        c2, c3 = q["gather_max"][2] + q["mean"][2], q["gather_max"][2] + q["mean"][2] + q["min"][2]
        lines.append("  fused mean+max %.0f us vs composed %.0f us: x%.2f;  fused mean+max+min %.0f us vs composed %.0f us: x%.2f;  "
                     "mean+root+bias x%.2f of gmm_fwd K=1;  bwd max x%.2f of gather_max_bwd"
                     % (q["mean+max"][2], c2, q["mean+max"][2] / c2, q["mean+max+min"][2], c3, q["mean+max+min"][2] / c3,
                        q["mean+root+bias"][2] / q["gmm_fwd K=1"][2], q["bwd max"][2] / q["gather_max_bwd"][2]))
        print("\n".join(lines[-(len(alg) + 2):]), flush=True)
        del Bs, Xs, Rs, Ds, O1, O2, O3, Oa, Ob, G2, saved, amx, inv, amx_e
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sage_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "pna":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat", add_self_loops=False)
    reps = max(a.iters, 20)
    lines = ["neighbour moments (PNAConv) on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d (no loops), float32; "
             "median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms alternating in one loop, rotating buffer "
             "sets; fused = ONE ops.gather_moments launch (mean + min + max + std, root A, mu and both args stored); composed = "
             "ops.gather_stats(mean + max + min) + the variance from two more ops.gather_stats means, of x and of x * x (the sum of "
             "the three medians; the x * x product, the subtraction and the root additions are not counted); bytes = the "
             "algorithmic counts of ops.py and DESIGN.md 4.17 (MB)" % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    for C in (64, 128, 256):
        R = 2 if nn_ * C * 4 >= (1 << 29) else 4
        Bs = [torch.randn(nn_, 2 * C, device=dev) for _ in range(R)]           # [A | B]
        As, Xs = [b[:, :C] for b in Bs], [b[:, C:] for b in Bs]
        X2 = [(x * x).contiguous() for x in Xs]
        Ds = [torch.randn(nn_, 4 * C, device=dev) for _ in range(R)]           # [dS | dQ | dMx | dMn]
        O4, O3 = torch.empty(nn_, 4 * C, device=dev), torch.empty(nn_, 3 * C, device=dev)
        Oa, Ob = torch.empty(nn_, C, device=dev), torch.empty(nn_, C, device=dev)
        saved = [ops.gather_moments(g, Xs[i], want=("mean", "min", "max", "std"), root=As[i]) for i in range(R)]
        amn, amx, inv = [s[1][1] for s in saved], [s[1][2] for s in saved], [s[2] for s in saved]
        tw = C // 4
        q = alternate({
            "moments 4": lambda i: ops.gather_moments(g, Xs[i], want=("mean", "min", "max", "std"), root=As[i], out=O4),
            "moments 4 towers": lambda i: ops.gather_moments(g, Xs[i], want=("mean", "min", "max", "std"), root=As[i], tower_width=tw, out=O4),
            "moments std": lambda i: ops.gather_moments(g, Xs[i], want=("std",), out=Oa),
            "stats mean+max+min": lambda i: ops.gather_stats(g, Xs[i], want=("mean", "max", "min"), out=O3),
            "stats mean x": lambda i: ops.gather_stats(g, Xs[i], want=("mean",), out=Oa),
            "stats mean x*x": lambda i: ops.gather_stats(g, X2[i], want=("mean",), out=Ob),
            "moments bwd": lambda i: ops.gather_moments_bwd(g, ds=Ds[i][:, :C], dq=Ds[i][:, C:2 * C], b=Xs[i], invdeg=inv[i],
                                                            dmx=Ds[i][:, 2 * C:3 * C], argmx=amx[i], dmn=Ds[i][:, 3 * C:], argmn=amn[i], out=Oa),
            "stats bwd": lambda i: ops.gather_stats_bwd(g, ds=Ds[i][:, :C], invdeg=inv[i], dmx=Ds[i][:, 2 * C:3 * C], argmx=amx[i],
                                                        dmn=Ds[i][:, 3 * C:], argmn=amn[i], out=Ob)}, reps, R)
        feat, ent, node = 4.0 * nn_ * C, 4.0 * g.nnz, 4.0 * nn_
        alg = {"moments 4": 9 * feat + 2 * ent + 2 * node, "moments 4 towers": 9 * feat + 2 * ent + 2 * node,
               "moments std": 3 * feat + 2 * ent + 2 * node, "stats mean+max+min": 6 * feat + 2 * ent + 2 * node,
               "stats mean x": 2 * feat + 2 * ent + 2 * node, "stats mean x*x": 2 * feat + 2 * ent + 2 * node,
               "moments bwd": 8 * feat + 3 * ent + 2 * node, "stats bwd": 6 * feat + 3 * ent + 2 * node}
        lines.append("C=%d (%d buffer sets; towers of %d):" % (C, R, tw))
        for k in alg:
            lines.append("  %-19s %s  %7.0f MB  %.2f TB/s alg" % (k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6))
        c3 = q["stats mean+max+min"][2] + q["stats mean x"][2] + q["stats mean x*x"][2]
        lines.append("  fused mean+min+max+std %.0f us vs composed (three sweeps) %.0f us: x%.2f;  tower-major x%.2f of plain;  "
                     "moments bwd (4 streams + B) x%.2f of stats bwd (3 streams)"
                     % (q["moments 4"][2], c3, q["moments 4"][2] / c3, q["moments 4 towers"][2] / q["moments 4"][2],
                        q["moments bwd"][2] / q["stats bwd"][2]))
        print("\n".join(lines[-(len(alg) + 2):]), flush=True)
        del Bs, As, Xs, X2, Ds, O4, O3, Oa, Ob, saved, amn, amx, inv
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pna_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if a.what == "gen":
    nu_ = int(round(n ** 0.5)); nv_ = n // nu_
    v, f = synth.rcb_relabel(*synth.torus(nu_, nv_))
    nn_ = len(v)
    f64 = np.asarray(f, dtype=np.int64)
    e = np.concatenate([f64[:, [0, 1]], f64[:, [1, 2]], f64[:, [2, 0]]])
    key = np.unique(np.concatenate([e[:, 0] * nn_ + e[:, 1], e[:, 1] * nn_ + e[:, 0]]))
    ei = torch.from_numpy(np.stack([key // nn_, key % nn_])).contiguous().to(dev)
    g = ops.graph_for(ei, nn_, norm="gat", add_self_loops=False)
    reps = max(a.iters, 20)
    lines = ["softmax aggregation (GENConv) on the vertex graph of torus(%d, %d) in RCB order: N=%d, entries=%d (no loops), float32; "
             "median of %d launches [min q1 q3 max], one HIP-event pair per launch, forms alternating in one loop, rotating buffer "
             "sets; softmax = ONE ops.gather_softmax launch (message relu + eps, t = 1, root, lse stored; 'no lse': a forward without "
             "a backward), mean = ops.gather_stats(mean) with root at the same width; softmax bwd = ONE ops.gather_softmax_bwd launch "
             "(dH and the root block, dt_rows), mean bwd = ops.gather_stats_bwd (dX and the root block); bytes = the algorithmic counts "
             "of ops.py and DESIGN.md 4.18 (MB)" % (nu_, nv_, nn_, g.nnz, reps)]
    print(lines[0], flush=True)
    for C in (32, 64, 128, 256):
        R = 2 if nn_ * C * 4 >= (1 << 29) else 4
        Bs = [torch.randn(nn_, 2 * C, device=dev) for _ in range(R)]           # [H | D]
        Hs, Rs = [b[:, :C] for b in Bs], [b[:, C:] for b in Bs]
        Ds = [torch.randn(nn_, C, device=dev) for _ in range(R)]
        Oy, Om = torch.empty(nn_, C, device=dev), torch.empty(nn_, C, device=dev)
        G2, G3 = torch.empty(nn_, 2 * C, device=dev), torch.empty(nn_, 2 * C, device=dev)
        saved = [ops.gather_softmax(g, Hs[i], 1.0, msg_eps=1e-7, root=Rs[i]) for i in range(R)]
        Yp, Ls = [s[0] - Rs[i] for i, s in enumerate(saved)], [s[1] for s in saved]
        inv = ops.gather_stats(g, Hs[0], want=("mean",))[2]
        q = alternate({
            "softmax": lambda i: ops.gather_softmax(g, Hs[i], 1.0, msg_eps=1e-7, root=Rs[i], out=Oy),
            "softmax no lse": lambda i: ops.gather_softmax(g, Hs[i], 1.0, msg_eps=1e-7, root=Rs[i], out=Oy, want_lse=False),
            "mean": lambda i: ops.gather_stats(g, Hs[i], want=("mean",), root=Rs[i], out=Om),
            "softmax bwd": lambda i: ops.gather_softmax_bwd(g, Ds[i], Hs[i], Yp[i], Ls[i], 1.0, msg_eps=1e-7, root=True, want_dt=True, out=G2),
            "mean bwd": lambda i: ops.gather_stats_bwd(g, ds=Ds[i], invdeg=inv, root=True, out=G3)}, reps, R)
        feat, ent, node = 4.0 * nn_ * C, 4.0 * g.nnz, 4.0 * nn_
        alg = {"softmax": 4 * feat + 2 * ent + node, "softmax no lse": 3 * feat + 2 * ent + node, "mean": 3 * feat + 2 * ent + 2 * node,
               "softmax bwd": 7 * feat + 3 * ent + 2 * node, "mean bwd": 4 * feat + 3 * ent + 2 * node}
        lines.append("C=%d (%d buffer sets):" % (C, R))
        for k in alg:
            lines.append("  %-15s %s  %7.0f MB  %.2f TB/s alg" % (k, fmt(q[k]), alg[k] / 1e6, alg[k] / q[k][2] / 1e6))
        rate = lambda k: alg[k] / q[k][2]
        lines.append("  softmax x%.2f of mean in time (x%.2f per byte); without lse x%.2f (x%.2f per byte);  softmax bwd x%.2f of mean bwd "
                     "in time (x%.2f per byte)"
                     % (q["softmax"][2] / q["mean"][2], rate("mean") / rate("softmax"), q["softmax no lse"][2] / q["mean"][2],
                        rate("mean") / rate("softmax no lse"), q["softmax bwd"][2] / q["mean bwd"][2], rate("mean bwd") / rate("softmax bwd")))
        print("\n".join(lines[-(len(alg) + 2):]), flush=True)
        del Bs, Hs, Rs, Ds, Oy, Om, G2, G3, saved, Yp, Ls, inv
    out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gen_microbench.txt")
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")

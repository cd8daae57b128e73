"""Worker of tests/test_gpu_edge_weight.py: the valued gather, its transpose and the affine form on the icosphere / open grid /
flipped-with-hub vertex graphs, C in {4, 32, 128, 512}, against the dense float64 operator, under the environment it was started
with (the library reads its route switches once per process, hence a process per setting: DDMP_SPMM_LEAN=0 is the slab route,
DDMP_SPMM_PATCH=1 the LDS-patch route).  The route a setting names is ASSERTED from the library's own selection queries
(``ddmp_spmm_lean_selected``, ``ddmp_spmm_patch_selected``, ``ddmp_graph_patch_info``).  The randomly numbered meshes ("ico",
"grid", "hub") never get patch tables -- a 64-row chunk of theirs references far more than the 192 distinct columns the kernel
holds -- so the LDS-patch route is the "rcbhub" graph's: a flipped torus in RCB order (compact chunks) with a 1200-neighbour hub,
whose chunk is heavy and runs the lean gather's chunk list (hub-chunk path) beside the patch kernel.  Prints every figure, asserts
the project's gather tolerance (rel-L2 < 1e-6, ``test_spmm_matches_dense``) and writes the outputs to the .npz named on the
command line so that the caller can compare routes bit for bit."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WIDTHS = (4, 32, 128, 512)


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def graphs():
    """name -> (edge_index [2, nnz] symmetric structure, n).  "hub": a flipped torus whose vertex 17 is ALSO joined to 1200 other
    vertices -- its 64-row chunk has more entries than the lean gather stages (the hub-chunk path)."""
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    out = {}
    meshes = {"ico": synth.icosphere(3), "grid": synth.open_grid(24, 17)}
    v, f = synth.torus(60, 30)
    meshes["hub"] = (v, synth.add_hub(v, synth.flip_edges(v, f, rounds=10, seed=1), 17, 24))
    v, f = synth.torus(80, 50)                                   # 4000 vertices = 63 chunks: one oversized chunk is < 2 % of them
    meshes["rcbhub"] = (v, synth.add_hub(v, synth.flip_edges(v, f, rounds=10, seed=2), 2000, 24))
    for name, (v, f) in meshes.items():
        v, f = synth.rcb_relabel(v, f) if name == "rcbhub" else synth.permute_vertices(v, f, 1)
        e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
        if "hub" in name:
            hub = 17 if name == "hub" else 2000
            have = set(e[1][e[0] == hub].tolist()) | set(e[0][e[1] == hub].tolist()) | {hub}
            far = torch.tensor([k for k in range(len(v)) if k not in have][:1200], dtype=torch.long)
            e = torch.cat([e, torch.stack([torch.full_like(far, hub), far])], 1)
        out[name] = (torch.cat([e, e[[1, 0]]], 1).contiguous(), len(v))
    return out


def weights(nnz, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(nnz, generator=gen) + 0.25                 # positive, NOT symmetric


def route_of(g, C):
    """The kernel(s) the plain gather of graph ``g`` at width C runs, from the library's selection queries."""
    import ctypes
    from dual_dmp_amd import _lib
    L = _lib.lib()
    if C % 32:
        return "scalar" if C < 8 else "row"
    kd, heavy, split = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.ddmp_graph_patch_info(g.handle, ctypes.byref(kd), ctypes.byref(heavy), ctypes.byref(split)) == 0
    rest = "lean" if L.ddmp_spmm_lean_selected(g.handle, C, C, C) else "slab"
    if L.ddmp_spmm_patch_selected(g.handle, C, 0, 0, 0):
        return "patch+%s-list" % rest if heavy.value > 0 else "patch"
    return rest


def run(dev, names=("ico", "grid", "hub", "rcbhub"), widths=WIDTHS):
    """-> {key: output tensor (CPU)}; asserts rel-L2 < 1e-6 against the dense float64 operator for every case, and the route the
    environment names."""
    from dual_dmp_amd import ops
    from gcnw_ref import dense_gcn_norm
    res = {}
    forced_patch, forced_slab = os.environ.get("DDMP_SPMM_PATCH") == "1", os.environ.get("DDMP_SPMM_LEAN") == "0"
    for name, (ei, n) in graphs().items():
        if name not in names:
            continue
        w = weights(ei.shape[1], n)
        A = dense_gcn_norm(ei, w, n)
        eid, wd = ei.to(dev), w.to(dev)
        g = ops.graph_for(eid, n, edge_weight=wd)
        g1 = ops.Graph.from_edge_index(eid, n, valued=ops.valued_flags())          # all-ones weights, default options
        g0 = ops.graph_for(eid, n)                                                  # the unvalued graph
        assert g.valued and g1.valued and not g0.valued
        for C in widths:
            route = route_of(g, C)
            assert route_of(g1, C) == route and route_of(g0, C) == route         # same structure, same selection
            if C % 32 == 0:
                if name == "rcbhub" and forced_patch and C >= 64:
                    assert route == "patch+lean-list", (name, C, route)      # the patch kernel + the hub's heavy chunk on the list
                elif forced_slab:
                    assert route == "slab", (name, C, route)
                elif not forced_patch or name != "rcbhub":
                    assert route == "lean", (name, C, route)                  # (unordered numberings never get patch tables)
            gen = torch.Generator().manual_seed(C)
            x, z = torch.randn(n, C, generator=gen), torch.randn(n, C, generator=gen)
            xd = x.to(dev)
            bias = torch.randn(C, generator=gen)
            y = ops.spmm(g, xd, bias=bias.to(dev) if C % 4 == 0 else None)
            yt = ops.spmm(g, xd, transpose=True)
            ya = ops.spmm_axpby(g, xd, z=z.to(dev), a=-1.2, b=0.4, c=-1.0)
            e = (relerr(y, A @ x.double() + bias.double()), relerr(yt, A.t() @ x.double()),
                 relerr(ya, -1.2 * (A @ x.double()) + 0.4 * x.double() - z.double()))
            same = torch.equal(ops.spmm(g1, xd), ops.spmm(g0, xd)) and torch.equal(ops.spmm(g1, xd, transpose=True), ops.spmm(g0, xd))
            print("valued gather %s n=%d C=%d [%s]: rel-L2 gather %.2e transpose %.2e affine %.2e; all-ones == unvalued bit for bit: %s"
                  % (name, n, C, route, e[0], e[1], e[2], same), flush=True)
            assert max(e) < 1e-6, (name, C, e)
            assert same, (name, C)
            res["%s_%d" % (name, C)] = y.cpu()
            res["%s_%d_t" % (name, C)] = yt.cpu()
            res["%s_%d_a" % (name, C)] = ya.cpu()
    return res


if __name__ == "__main__":
    out = run(torch.device("cuda:0"))
    np.savez(sys.argv[1], **{k: v.numpy() for k, v in out.items()})

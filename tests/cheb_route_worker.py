"""Worker of tests/test_gpu_cheb.py: ``ops.spmm_axpby`` on the icosphere-3 vertex graph (norm="sym", C = 64, both addends, seeded
inputs) under the environment it was started with; writes the result to the .npy named on the command line.  The library reads
its route switches once per process, hence a process per setting."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs():
    from dual_dmp_amd import synth
    from dual_dmp_amd.mesh import Mesh
    v, f = synth.permute_vertices(*synth.icosphere(3), 1)
    e = torch.tensor(Mesh(vs=v, faces=f).edges.T, dtype=torch.long)
    gen = torch.Generator().manual_seed(64)
    x, z, z2 = (torch.randn(len(v), 64, generator=gen) for _ in range(3))
    return torch.cat([e, e[[1, 0]]], 1), len(v), x, z, z2


def run(dev):
    from dual_dmp_amd import ops
    ei, n, x, z, z2 = inputs()
    eid = ei.to(dev)
    g = ops.graph_for(eid, n, norm="sym")
    return ops.spmm_axpby(g, x.to(dev), z=z.to(dev), z2=z2.to(dev), a=-1.2, b=0.4, c=1.0, d=-1.0).cpu()


if __name__ == "__main__":
    np.save(sys.argv[1], run(torch.device("cuda:0")).numpy())

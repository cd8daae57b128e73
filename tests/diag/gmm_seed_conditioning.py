"""How well conditioned is the teacher-forced GMMConv training comparison of tests/test_gpu_gmm.py for a given seed?  Evaluates the
float64 and the float32 CPU reference nets alone (no GPU, no code under test) for two Adam steps and prints, per step, the smallest
|LeakyReLU input| of the float64 net and the float32 net's own gradient distance from float64.  A distance near 1e-3 means a
float32 rounding moved a LeakyReLU input across zero (slope 0.01 <-> 1): the case then measures where a rounding fell.
usage: python tests/diag/gmm_seed_conditioning.py [--threads T] SEED [SEED ...]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_jobs as OJ  # noqa: E402
from test_gpu_gmm import _RefPosNet, _redraw, relerr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("seeds", type=int, nargs="+")
ap.add_argument("--threads", type=int, default=8, help="CPU threads: another count is another float32 summation order")
a = ap.parse_args()
torch.set_num_threads(a.threads)

from dual_dmp_amd.engine import POS_WIDTHS  # noqa: E402
from dual_dmp_amd.networks import PosNet  # noqa: E402
from dual_dmp_amd.nn_ops import cartesian_pseudo  # noqa: E402

gt, noisy, smooth, data = OJ.case("ico3")
target = torch.tensor(np.asarray(gt.vs), dtype=torch.float64)
z1, x_pos, ei = data.z1.detach().cpu(), data.x_pos.detach().cpu(), data.edge_index.cpu()
attr = cartesian_pseudo(x_pos.float(), ei)


def run(r, dtype, mins):
    hook = r.l_relu.register_forward_pre_hook(lambda m, inp: mins.append(float(inp[0].detach().abs().min())))
    loss = ((r(z1.to(dtype), x_pos.to(dtype), ei, attr.to(dtype)) - target.to(dtype)) ** 2).mean()
    loss.backward()
    hook.remove()
    return {k: p.grad for k, p in r.named_parameters()}


for seed in a.seeds:
    torch.manual_seed(seed)
    net = PosNet("cpu", fused=False, conv="gmm", K=3)             # (the parameters are drawn on the CPU whatever the device)
    for i in range(1, 13):
        _redraw(getattr(net, "conv%d" % i), i)
    r64 = _RefPosNet(POS_WIDTHS, 3, torch.float64)
    r64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in net.state_dict().items()})
    r64.train()
    opt = torch.optim.Adam(r64.parameters(), lr=1e-3)
    out = []
    for step in range(2):
        r32 = _RefPosNet(POS_WIDTHS, 3, torch.float32)
        r32.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in r64.state_dict().items()})
        r32.train()
        opt.zero_grad()
        mins = []
        g64, g32 = run(r64, torch.float64, mins), run(r32, torch.float32, [])
        cat = lambda d: torch.cat([d[k].reshape(-1).double() for k in sorted(g64)])
        out.append((step, min(mins), int(np.argmin(mins)) + 1, relerr(cat(g32), cat(g64))))
        opt.step()
    print("seed %d (%d threads): " % (seed, a.threads)
          + "; ".join("step %d min |lrelu input| %.2e (activation %d), float32 CPU gradient rel-L2 %.2e" % o for o in out), flush=True)

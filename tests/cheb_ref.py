"""Test-side reference for the Chebyshev path: dense float64 restatement of ``torch_geometric.nn.ChebConv`` 2.2.0
(normalization="sym") in plain torch.  ``A`` is built from ``edge_index`` with ``index_put_(accumulate=True)`` (multi-edges
keep their multiplicity), the diagonal is dropped, ``S = D^-1/2 A D^-1/2`` with ``deg^-1/2 = 0`` for isolated nodes,
``L^ = -(2 / lambda_max) S + (2 / lambda_max - 1) I``; gradients come from autograd on it.  Test infrastructure only."""
import math

import torch
import torch.nn as nn


def dense_s(ei, n, dtype=torch.float64):
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((ei[1].cpu(), ei[0].cpu()), torch.ones(ei.shape[1], dtype=torch.float64), accumulate=True)
    A.fill_diagonal_(0.0)                                     # explicit self loops are dropped, none is added
    deg = A.sum(1)
    d = torch.where(deg > 0, deg.clamp(min=1.0).pow(-0.5), torch.zeros_like(deg))
    return (d[:, None] * A * d[None, :]).to(dtype)


def dense_lhat(ei, n, lambda_max=None, dtype=torch.float64):
    lam = 2.0 if lambda_max is None else float(lambda_max)
    S = dense_s(ei, n)
    return ((-2.0 / lam) * S + (2.0 / lam - 1.0) * torch.eye(n, dtype=torch.float64)).to(dtype)


def axpby_ref(S, x, z=None, z2=None, a=1.0, b=0.0, c=0.0, d=0.0):
    """What ops.spmm_axpby computes, in float64."""
    y = a * (S @ x.double()) + b * x.double()
    if z is not None:
        y = y + c * z.double()
    if z2 is not None:
        y = y + d * z2.double()
    return y


class ChebConvRef(nn.Module):
    """Parameters ``lins.k.weight`` [out, in] (Glorot-uniform), ``bias`` [out] (zeros), as PyG names them."""

    def __init__(self, in_channels, out_channels, K, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, K
        self.lins = nn.ModuleList([nn.Linear(in_channels, out_channels, bias=False) for _ in range(K)])
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        a = math.sqrt(6.0 / (in_channels + out_channels))
        with torch.no_grad():
            for lin in self.lins:
                lin.weight.uniform_(-a, a)

    def forward(self, x, edge_index, lambda_max=None):
        L = dense_lhat(edge_index, x.shape[0], lambda_max, x.dtype)
        t0 = x
        out = self.lins[0](t0)
        if self.K > 1:
            t1 = L @ x
            out = out + self.lins[1](t1)
            for lin in self.lins[2:]:
                t2 = 2.0 * (L @ t1) - t0
                out = out + lin(t2)
                t0, t1 = t1, t2
        if self.bias is not None:
            out = out + self.bias
        return out


class CpuChebOps:
    """PyTorch-CPU stand-in for the handful of ``dual_dmp_amd.ops`` calls ChebConv's autograd function makes (float64
    inside, float32 at the interfaces, results written into ``out`` views like the kernels do), so that its HOST logic --
    packing, block layout, the Clenshaw recurrence of the backward pass -- can be checked without a GPU.  Tests inject it
    with ``monkeypatch.setattr(nn_ops, "ops", CpuChebOps(S))``; the product never imports it."""

    def __init__(self, S):
        self.S = S.double()
        self.calls = []

    def on_device(self, dev):
        import contextlib
        return contextlib.nullcontext()

    def spmm_axpby(self, g, x, out=None, z=None, z2=None, a=1.0, b=0.0, c=0.0, d=0.0):
        assert out is not None and out.data_ptr() != x.data_ptr()
        self.calls.append("spmm_axpby")
        out.copy_(axpby_ref(self.S, x, z, z2, a, b, c, d))
        return out

    def gemm_nt(self, a, w, bias=None):
        self.calls.append("gemm_nt")
        y = a.double() @ w.double().t()
        return (y if bias is None else y + bias.double()).float()

    def gemm_nn(self, a, w):
        self.calls.append("gemm_nn")
        return (a.double() @ w.double()).float()

    def gemm_tn(self, g, z):
        self.calls.append("gemm_tn")
        return (g.double().t() @ z.double()).float()

    def colsum(self, x):
        return x.double().sum(0)

"""TEST-SIDE REFERENCE for GMMConv: two independent restatements of torch_geometric 2.2.0's GMMConv (MoNet; int ``in_channels``,
``separate_gaussians=False``, mean aggregation) in plain torch, float64 by default, differentiable.  Written from the published
source from memory -- PyG cannot be installed here.

* ``gmm_edge_list`` / ``GMMConvRef`` -- the edge-list form PyG itself uses: per edge K Gaussians of its pseudo-coordinates, the
  Gaussian-mixed source rows, a scatter mean over the edges of each target (``index_add_`` and a count), then the root term and the
  bias.  No self loops are added; duplicate edges are separate edges with their own pseudo-coordinates.
* ``dense_gmm`` -- a dense [N, N, K] form: the Gaussians of all edges j -> i accumulated into one table, one contraction.

``edge_index`` row 0 = source j, row 1 = target i; ``g``: [in, K * out], ``mu`` / ``sigma``: [K, dim], ``root``: [out, in] or None,
``bias``: [out] or None."""
import math

import torch
import torch.nn as nn

EPS = 1e-15


def gaussians(attr, mu, sigma):
    """-> [E, K]: exp(-1/2 sum_d (attr[t,d] - mu[k,d])^2 / (EPS + sigma[k,d]^2))."""
    d = attr.unsqueeze(1) - mu.unsqueeze(0)
    return torch.exp((-0.5 * d.pow(2) / (EPS + sigma.unsqueeze(0).pow(2))).sum(-1))


def gmm_edge_list(x, edge_index, attr, g, mu, sigma, root, bias, K, full=False):
    """The edge-list form.  ``full``: -> (out, dict(src, dst, hf, gamma, deg)); ``gamma`` (the per-edge Gaussians, [E, K]) keeps its
    gradient."""
    n = x.shape[0]
    C = g.shape[1] // K
    hf = (x @ g).view(n, K, C)
    src, dst = edge_index[0], edge_index[1]
    gamma = gaussians(attr, mu, sigma)
    if full:
        gamma.retain_grad()
    msg = (gamma.unsqueeze(-1) * hf[src]).sum(1)
    deg = torch.zeros(n, dtype=x.dtype).index_add_(0, dst, torch.ones(len(dst), dtype=x.dtype))
    out = torch.zeros((n, C), dtype=x.dtype).index_add_(0, dst, msg) / deg.clamp(min=1.0).unsqueeze(-1)
    if root is not None:
        out = out + x @ root.t()
    if bias is not None:
        out = out + bias
    if full:
        return out, dict(src=src, dst=dst, hf=hf, gamma=gamma, deg=deg)
    return out


def dense_gmm(x, edge_index, attr, g, mu, sigma, root, bias, K):
    """The dense form: T[i, j, k] = sum over the edges j -> i of their k-th Gaussian, cnt[i] = number of edges with target i;
    out[i] = sum_j sum_k T[i, j, k] Hf[j, k] / cnt[i] + x_i root^T + bias."""
    n = x.shape[0]
    C = g.shape[1] // K
    hf = torch.einsum("ni,ikc->nkc", x, g.view(-1, K, C))
    gam = torch.stack([torch.exp(-0.5 * sum((attr[:, d] - mu[k, d]) ** 2 / (EPS + sigma[k, d] ** 2) for d in range(mu.shape[1])))
                       for k in range(K)], 1)
    T = torch.zeros((n, n, K), dtype=x.dtype).index_put((edge_index[1], edge_index[0]), gam, accumulate=True)
    cnt = torch.zeros((n, n), dtype=x.dtype).index_put((edge_index[1], edge_index[0]),
                                                       torch.ones(edge_index.shape[1], dtype=x.dtype), accumulate=True).sum(1)
    out = torch.einsum("ijk,jkc->ic", T, hf) / torch.where(cnt > 0, cnt, torch.ones_like(cnt)).unsqueeze(1)
    if root is not None:
        out = out + torch.einsum("ni,ci->nc", x, root)
    if bias is not None:
        out = out + bias
    return out


class GMMConvRef(nn.Module):
    """Edge-list reference with PyG's parameter names and shapes."""

    def __init__(self, in_channels, out_channels, dim, kernel_size, root_weight=True, bias=True, dtype=torch.float64):
        super().__init__()
        self.in_channels, self.out_channels, self.dim, self.kernel_size = in_channels, out_channels, dim, kernel_size
        self.g = nn.Parameter(torch.empty(in_channels, kernel_size * out_channels, dtype=dtype))
        self.mu = nn.Parameter(torch.empty(kernel_size, dim, dtype=dtype))
        self.sigma = nn.Parameter(torch.empty(kernel_size, dim, dtype=dtype))
        self.root = nn.Linear(in_channels, out_channels, bias=False, dtype=dtype) if root_weight else None
        self.bias = nn.Parameter(torch.zeros(out_channels, dtype=dtype)) if bias else None
        with torch.no_grad():
            for t in (self.g, self.mu, self.sigma) + ((self.root.weight,) if root_weight else ()):
                a = math.sqrt(6.0 / (t.shape[0] + t.shape[1]))
                t.uniform_(-a, a)

    def load_from(self, conv):
        """Copy the parameters of a ``GMMConv`` (or another reference) into this one, in this one's dtype."""
        with torch.no_grad():
            for name in ("g", "mu", "sigma"):
                getattr(self, name).copy_(getattr(conv, name).detach().cpu())
            if self.root is not None:
                self.root.weight.copy_(conv.root.weight.detach().cpu())
            if self.bias is not None:
                self.bias.copy_(conv.bias.detach().cpu())
        return self

    def forward(self, x, edge_index, edge_attr, full=False):
        return gmm_edge_list(x, edge_index, edge_attr, self.g, self.mu, self.sigma,
                             None if self.root is None else self.root.weight, self.bias, self.kernel_size, full=full)

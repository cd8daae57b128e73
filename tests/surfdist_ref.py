"""float64 brute-force point-to-triangle distance: the reference the surface-distance kernel is tested against (test code
only).  Written independently of the kernel's Voronoi-region walk: the distance to a triangle is the smaller of the
distances to its three edges and, when the point projects inside the triangle, the distance to its plane.  A degenerate
triangle (a repeated vertex, three collinear vertices) has no inside and is its edges.  torch, so that the same code runs
on the host and, for the 1M-face check, on the GPU."""
import numpy as np
import torch


def _cross(u, v):
    return torch.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                        u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _seg_d2(p, a, b):
    d = b - a
    ap = p - a
    dd = (d * d).sum(-1)
    t = torch.where(dd > 0, (ap * d).sum(-1) / torch.where(dd > 0, dd, torch.ones_like(dd)), torch.zeros_like(dd))
    t = t.clamp(0.0, 1.0)
    e = ap - t.unsqueeze(-1) * d
    return (e * e).sum(-1)


def point_tri_d2(p, a, b, c):
    """squared distances, broadcasting p [..., 3] against a, b, c [..., 3] (float64)."""
    d2 = torch.minimum(_seg_d2(p, a, b), torch.minimum(_seg_d2(p, b, c), _seg_d2(p, c, a)))
    n = _cross(b - a, c - a)
    nn = (n * n).sum(-1)
    ok = nn > 1e-300
    nns = torch.where(ok, nn, torch.ones_like(nn))
    s = (n * (p - a)).sum(-1)
    q = p - (s / nns).unsqueeze(-1) * n
    inside = ok
    for u, v in ((a, b), (b, c), (c, a)):
        inside = inside & ((_cross(v - u, q - u) * n).sum(-1) >= 0)
    return torch.where(inside, torch.minimum(d2, s * s / nns), d2)


def brute_force(points, vs, faces, chunk=256, device="cpu"):
    """exact distances (float64 numpy [Q]) from points [Q, 3] to the surface (vs [V, 3], faces [F, 3])."""
    P = torch.as_tensor(np.asarray(points, dtype=np.float64), device=device)
    V = torch.as_tensor(np.asarray(vs, dtype=np.float64), device=device)
    Fc = torch.as_tensor(np.asarray(faces, dtype=np.int64), device=device)
    a, b, c = V[Fc[:, 0]], V[Fc[:, 1]], V[Fc[:, 2]]
    out = torch.empty(len(P), dtype=torch.float64, device=device)
    for i in range(0, len(P), chunk):
        p = P[i:i + chunk].unsqueeze(1)
        out[i:i + chunk] = point_tri_d2(p, a, b, c).min(dim=1).values
    return out.sqrt().cpu().numpy()

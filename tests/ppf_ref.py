"""TEST-SIDE REFERENCE for PPFConv: two independent restatements of torch_geometric 2.2.0's PPFConv (max aggregation over
point-pair features) in plain torch, float64 by default, differentiable with respect to x and the modules' parameters.

* ``ppf_features`` / ``ppf_edge_list`` / ``PPFConvRef`` -- the edge-list form PyG itself uses: with ``add_self_loops`` explicit
  loops are removed and one loop per node is appended; per edge j -> i the features
  ``f_ij = [|d|, angle(n_i, d), angle(n_j, d), angle(n_i, n_j)]``, ``d = pos_j - pos_i``, ``angle(a, b) = atan2(|a x b|, a . b)``
  (``torch.cross``, ``torch.atan2``); the FULL ``local_nn`` (activations included) on ``cat[x_j, f_ij]`` (``f_ij`` alone when x is
  None); ``scatter_reduce("amax")`` over the edges of each target, 0 for a target without edges; then ``global_nn``.
* ``ppf_dense`` -- an [N, N] mask and a maximum over it.

``ppf_messages`` gives the bias-free LINEAR message of every coalesced entry, ``ppf_winners_and_gaps`` the smallest source id
that attains each (i, c)'s maximum and the gap to the runner-up among the row's other entries: the conditioning of the arg-max.

``edge_index`` row 0 = source j, row 1 = target i."""
import copy

import torch
import torch.nn as nn


def with_loops(edge_index, n, add_self_loops):
    if not add_self_loops:
        return edge_index
    keep = edge_index[0] != edge_index[1]
    loops = torch.arange(n, dtype=edge_index.dtype)
    return torch.cat([edge_index[:, keep], torch.stack([loops, loops])], 1)


def angle(a, b):
    return torch.atan2(torch.cross(a, b, dim=1).norm(dim=1), (a * b).sum(1))


def ppf_features(pos, normal, edge_index):
    """[E, 4], one row per edge j -> i."""
    j, i = edge_index[0], edge_index[1]
    d = pos[j] - pos[i]
    return torch.stack([d.norm(dim=1), angle(normal[i], d), angle(normal[j], d), angle(normal[i], normal[j])], 1)


def ppf_edge_list(x, pos, normal, edge_index, local_nn, global_nn=None, add_self_loops=True):
    n = pos.shape[0]
    ei = with_loops(edge_index, n, add_self_loops)
    f = ppf_features(pos, normal, ei)
    msg = local_nn(f if x is None else torch.cat([x[ei[0]], f], 1))
    idx = ei[1].view(-1, 1).expand(-1, msg.shape[1])
    out = torch.zeros((n, msg.shape[1]), dtype=msg.dtype).scatter_reduce(0, idx, msg, "amax", include_self=False)
    return out if global_nn is None else global_nn(out)


def ppf_dense(x, pos, normal, edge_index, local_nn, global_nn=None, add_self_loops=True):
    """z[i, j, :] = local_nn(cat[x_j, f_ij]) for every pair, a maximum over the j with an edge j -> i."""
    n = pos.shape[0]
    ei = with_loops(edge_index, n, add_self_loops)
    mask = torch.zeros((n, n), dtype=torch.bool)
    mask[ei[1], ei[0]] = True
    ii, jj = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    pairs = torch.stack([jj.reshape(-1), ii.reshape(-1)])         # source j, target i, at flat index i * n + j
    f = ppf_features(pos, normal, pairs)
    z = local_nn(f if x is None else torch.cat([x[pairs[0]], f], 1)).reshape(n, n, -1)
    z = torch.where(mask.unsqueeze(-1), z, torch.full_like(z, -float("inf")))
    out = torch.where(mask.any(1, keepdim=True), z.amax(1), torch.zeros((), dtype=z.dtype))
    return out if global_nn is None else global_nn(out)


def as_dtype(fn, dtype):
    return None if fn is None else copy.deepcopy(fn).to("cpu").to(dtype)


class PPFConvRef(nn.Module):
    """Edge-list reference with PyG's attribute names: ``local_nn``, ``global_nn``."""

    def __init__(self, local_nn, global_nn=None, add_self_loops=True, dtype=torch.float64):
        super().__init__()
        self.local_nn, self.global_nn = as_dtype(local_nn, dtype), as_dtype(global_nn, dtype)
        self.add_self_loops = add_self_loops

    def forward(self, x, pos, normal, edge_index):
        return ppf_edge_list(x, pos, normal, edge_index, self.local_nn, self.global_nn, self.add_self_loops)


def ppf_messages(x, pos, normal, edge_index, weight, add_self_loops=True):
    """-> (dst, src int64 [entries], msg [entries, C]): the bias-free linear message ``W cat[x_j, f_ij]`` of every COALESCED entry,
    sorted by (target, source)."""
    n = pos.shape[0]
    ei = with_loops(edge_index, n, add_self_loops)
    key = torch.unique(ei[1] * n + ei[0])
    dst, src = key // n, key % n
    f = ppf_features(pos, normal, torch.stack([src, dst]))
    return dst, src, (f if x is None else torch.cat([x[src], f], 1)) @ weight.t()


def ppf_winners_and_gaps(dst, src, msg, n):
    """-> (arg int64 [n, C], gap [n, C], empty bool [n]).  arg[i, c]: the smallest source among row i's entries whose message
    attains the maximum; -1 for a row without entries.  gap[i, c]: that maximum minus the largest message of the row's OTHER
    entries (inf when there is none)."""
    C = msg.shape[1]
    idx = dst.view(-1, 1).expand(-1, C)
    neg = torch.full((n, C), -float("inf"), dtype=msg.dtype)
    mx = neg.scatter_reduce(0, idx, msg, "amax")
    big = torch.iinfo(torch.int64).max
    cand = torch.where(msg == mx[dst], src.view(-1, 1).expand(-1, C), torch.full((), big, dtype=torch.int64))
    arg = torch.full((n, C), big, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin")
    others = torch.where(src.view(-1, 1) == arg[dst], torch.full((), -float("inf"), dtype=msg.dtype), msg)
    second = neg.scatter_reduce(0, idx, others, "amax")
    empty = torch.ones(n, dtype=torch.bool)
    empty[dst] = False
    arg[empty] = -1
    gap = mx - second
    gap[empty] = float("inf")
    return arg, gap, empty

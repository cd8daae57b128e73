"""The host-side helpers every packed drop-in of ``nn_ops`` is written on -- ``_packed_gemm`` / ``_packed_grads`` and the
``concat=False`` pair ``_heads_mean`` / ``_heads_mean_bwd`` -- over the GEMM restatements of tests/gat_ops_stub.py, on
integer-valued float32 data: every product and sum is exact, so every comparison below is ``torch.equal``."""
import pytest
import torch

import gat_ops_stub

CIN, N, ROWS = 5, 7, (3, 4, None, 6)                             # block k has ROWS[k] rows; None: an absent block


def _ints(gen, *shape):
    return torch.randint(-4, 5, shape, generator=gen).float()


def _inputs(bias_pattern):
    """-> (x [7, 5], the weight blocks, the biases or None); ``bias_pattern``: "some" (block 1 has none), "none", "absent"."""
    gen = torch.Generator().manual_seed(3)
    x = _ints(gen, N, CIN)
    weights = [None if r is None else _ints(gen, r, CIN) for r in ROWS]
    biases = [None if r is None else _ints(gen, r) for r in ROWS]
    biases[1] = None
    if bias_pattern == "none":
        biases = [None] * len(ROWS)
    return x, weights, None if bias_pattern == "absent" else biases


class _Counting:
    """gat_ops_stub with the GEMM calls and their keyword arguments recorded."""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        fn = getattr(gat_ops_stub, name)
        if not name.startswith("gemm_"):
            return fn

        def wrapped(*a, **k):
            self.seen.append((name, k))
            return fn(*a, **k)
        return wrapped


@pytest.mark.parametrize("pad_each", [False, True])
@pytest.mark.parametrize("bias_pattern", ["some", "none", "absent"])
def test_packed_gemm_and_packed_grads_are_exact_on_integer_data(monkeypatch, pad_each, bias_pattern):
    from dual_dmp_amd import nn_ops
    stub = _Counting()
    monkeypatch.setattr(nn_ops, "ops", stub)
    x, weights, biases = _inputs(bias_pattern)
    xp, wp, buf, spans = nn_ops._packed_gemm(x, weights, biases, pad_each=pad_each)
    # the spans as documented: end to end (3, 4, 6 rows -> 13, padded to 16), or every block rounded up to 4 on its own
    assert spans == ([(0, 3), (4, 8), None, (8, 14)] if pad_each else [(0, 3), (3, 7), None, (7, 13)])
    assert xp.shape == (N, 8) and torch.equal(xp[:, :CIN], x) and not xp[:, CIN:].any()
    assert wp.shape == (16, 8) and buf.shape == (N, 16)
    (name, kw), = stub.seen
    assert name == "gemm_nt"
    used = torch.zeros(16, dtype=torch.bool)
    for k, (w, s) in enumerate(zip(weights, spans)):
        if w is None:
            continue
        b = None if biases is None else biases[k]
        want = x @ w.t() + (0 if b is None else b)               # a None bias among present ones: the zero block
        assert torch.equal(buf[:, s[0]:s[1]], want), k
        assert torch.equal(nn_ops._cols(buf, s), want) and torch.equal(wp[s[0]:s[1], :CIN], w) and not wp[s[0]:s[1], CIN:].any()
        used[s[0]:s[1]] = True
    assert nn_ops._cols(buf, spans[2]) is None
    assert not buf[:, ~used].any() and not wp[~used].any()      # the padding columns of buf (rows of wp) are zero
    if bias_pattern == "some":
        lb = kw["bias"]
        assert lb.shape == (16,) and not lb[~used].any() and not lb[spans[1][0]:spans[1][1]].any()
    else:
        assert kw.get("bias") is None                            # all None: no bias reaches gemm_nt

    gen = torch.Generator().manual_seed(4)
    g = nn_ops._grad_rows(N, spans, 16, x.device)
    assert not g[:, ~used].any()                                 # the buffer the kernels fill: its padding comes zeroed
    g[:, used] = _ints(gen, N, int(used.sum()))
    del stub.seen[:]
    dx, dw, db = nn_ops._packed_grads(g, xp, wp, spans, CIN, (True, False, True, False), (False, True, True, True), True)
    assert [n for n, _ in stub.seen] == ["gemm_tn", "gemm_nn"]
    assert dx.shape == (N, CIN) and torch.equal(dx, (g @ wp)[:, :CIN])
    for k, s in enumerate(spans):
        if s is None:                                            # an absent block: None, whatever was asked
            assert dw[k] is None and db[k] is None
            continue
        assert torch.equal(dw[k], g[:, s[0]:s[1]].t() @ x), k   # one gemm_tn serves every present block
        assert (db[k] is None) if k == 0 else torch.equal(db[k], g[:, s[0]:s[1]].sum(0)), k
    # nothing asked: no GEMM at all, None everywhere; bias gradients alone: still no gemm_tn
    del stub.seen[:]
    dx, dw, db = nn_ops._packed_grads(g, xp, wp, spans, CIN, (False,) * 4, None, False)
    assert dx is None and dw == [None] * 4 and db == [None] * 4 and stub.seen == []
    dx, dw, db = nn_ops._packed_grads(g, xp, wp, spans, CIN, (False, False, True, False), (True,) * 4, True)   # block 2 is absent
    assert [n for n, _ in stub.seen] == ["gemm_nn"] and dw == [None] * 4 and dx is not None
    assert [b is None for b in db] == [False, False, True, False]


def test_packed_rows_keeps_its_layout():
    """``_packed_rows`` (the GPU tests of GATv2Conv build their operands with it) against the layout written out."""
    from dual_dmp_amd import nn_ops
    gen = torch.Generator().manual_seed(5)
    a, b = _ints(gen, 3, 5), _ints(gen, 6, 4)
    for pad_each, rows, at in ((False, 12, 3), (True, 12, 4)):
        wp = nn_ops._packed_rows((a, None, b), 8, a.device, pad_each=pad_each)
        want = torch.zeros(rows, 8)
        want[:3, :5], want[at:at + 6, :4] = a, b
        assert torch.equal(wp, want)


def test_heads_mean_backward_is_the_gradient_of_its_forward():
    from dual_dmp_amd import nn_ops
    heads, C, n = 3, 4, 5
    gen = torch.Generator().manual_seed(6)
    y = (3 * _ints(gen, n, heads * C)).requires_grad_(True)      # multiples of 3: the mean over 3 heads is exact
    add = _ints(gen, C).requires_grad_(True)
    dy = 3 * _ints(gen, n, C)                                    # multiples of 3: dy / heads is exact
    out = nn_ops._heads_mean(y, heads, add)
    assert torch.equal(out, y.detach().view(n, heads, C).sum(1) / 3 + add.detach())
    assert torch.equal(nn_ops._heads_mean(y, heads), y.detach().view(n, heads, C).sum(1) / 3)
    gy, gadd = torch.autograd.grad(out, (y, add), dy)
    back = nn_ops._heads_mean_bwd(dy, heads)
    assert back.shape == (n, heads * C) and torch.equal(back, gy) and torch.equal(gadd, dy.sum(0))

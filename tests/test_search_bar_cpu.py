"""tests/_search_bar.py checked on the CPU: the float64 reference rounded to
fp32 and an fp32 torch matmul with a stable sort pass assert_topk, and an
answer with one modelled kernel fault is refused. The faults are the ones a
tiled, sliced top-k kernel can have (csrc/kernels/sim_topk.hip): a
zero-scored pad row of a partial tile returned when every score is negative;
ties by descending index; the last row of a slice never considered; the last
partial tile dropped; rank k-1 replaced by rank k; a slice's candidates merged
twice (a duplicate index); the query scale left out under the cosine metric.
"""
import pytest
import torch

from _search_bar import (assert_rejects, assert_topk, bf16r, inv_norm64, reference, stable_topk)

TILE = 128
K = 16
# (B, N, D): odd sizes, a partial last tile, more than one tile
SHAPES = [(37, 1003, 64), (5, 300, 512)]


def _randn(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, generator=g).bfloat16().float(), torch.randn(N, D, generator=g).bfloat16()


def _ints(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-3, 4, (B, D), generator=g).float(),
            torch.randint(-3, 4, (N, D), generator=g).float().bfloat16())


def _scores32(q, g, cosine, q_scale=True):
    """The kernel's arithmetic in torch fp32: an fp32 matmul of the bf16 values, then the fp32 scales."""
    s = q.bfloat16().float() @ g.float().t()
    if cosine:
        rq = inv_norm64(bf16r(q)).float()
        rg = inv_norm64(g.double()).float()
        s = (s * rq[:, None] if q_scale else s) * rg[None, :]
    return s


def _select(s, k):
    order, vals = stable_topk(s, k)
    return order.to(torch.int32), vals


@pytest.mark.parametrize("cosine", [False, True], ids=["dot", "cosine"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_correct_answers_pass(shape, cosine):
    B, N, D = shape
    q, g = _randn(B, N, D, seed=N + D)
    flag = True if cosine else None
    ref, _ = reference(q, g, cosine)
    idx, vals = _select(ref, K)
    assert_topk(idx, vals.float(), q, g, K, flag, flag)       # the float64 reference rounded to fp32
    idx, vals = _select(_scores32(q, g, cosine), K)
    assert_topk(idx, vals, q, g, K, flag, flag)               # an fp32 matmul with a stable sort
    qi, gi = _ints(B, N, D, seed=N)                           # plenty of ties
    idx, vals = _select(_scores32(qi, gi, False), K)
    assert_topk(idx, vals, qi, gi, K)


def test_pad_row_returned():
    """Every score negative: the zero-scored rows that pad the last tile win unless they are masked."""
    B, N, D = 7, 129, 64
    q, g = _randn(B, N, D, seed=1)
    q, g = q.abs(), -g.abs()
    s = _scores32(q, g, False)
    assert float(s.max()) < 0
    idx, vals = _select(s, K)
    assert_topk(idx, vals, q, g, K)
    padded = torch.cat([s, torch.zeros(B, 2 * TILE - N)], 1)
    idx, vals = _select(padded, K)
    assert "(a)" in assert_rejects(idx, vals, q, g, K, what="pad row")


def test_ties_by_descending_index():
    B, N, D = 9, 300, 32
    q, g = _ints(B, N, D, seed=2)
    s = _scores32(q, g, False)
    rev = torch.sort(s.flip(-1), dim=-1, descending=True, stable=True)
    idx = (N - 1 - rev.indices[:, :K]).to(torch.int32)
    vals = rev.values[:, :K]
    assert bool((vals.diff(dim=-1) == 0).any())  # (the data has ties among the best)
    assert_rejects(idx, vals, q, g, K, what="ties by descending index")


def _planted(B, N, D, rows, seed):
    """bf16 randn with gallery row rows[i] = 3 q[i % B]: that query's best row by far."""
    q, g = _randn(B, N, D, seed)
    for i, n in enumerate(rows):
        g[n] = (3 * q[i % B]).bfloat16()
    return q, g


@pytest.mark.parametrize("fault", ["slice last row", "partial tile"])
def test_rows_never_considered(fault):
    B, N, D, slices = 6, 1003, 64, 3
    tiles = (N + TILE - 1) // TILE
    ends = [min(N, TILE * ((i + 1) * tiles // slices)) for i in range(slices)]
    lost = [e - 1 for e in ends] if fault == "slice last row" else list(range(N // TILE * TILE, N))
    q, g = _planted(B, N, D, [e - 1 for e in ends], seed=3)
    s = _scores32(q, g, False)
    idx, vals = _select(s, K)
    assert_topk(idx, vals, q, g, K)
    s[:, lost] = -float("inf")
    idx, vals = _select(s, K)
    assert "(d)" in assert_rejects(idx, vals, q, g, K, what=fault)


def test_rank_shifted():
    B, N, D = 37, 1003, 64
    q, g = _randn(B, N, D, seed=4)
    order, vals = stable_topk(_scores32(q, g, False), K + 1)
    idx = torch.cat([order[:, :K - 1], order[:, K:]], 1).to(torch.int32)
    vals = torch.cat([vals[:, :K - 1], vals[:, K:]], 1)
    assert_rejects(idx, vals, q, g, K, what="rank k-1 replaced by rank k")


def test_slice_merged_twice():
    B, N, D = 5, 300, 64
    q, g = _randn(B, N, D, seed=5)
    s = _scores32(q, g, False)
    first = s[:, :TILE]                      # slice 0's candidates, twice, and the other slice's
    order, vals = stable_topk(torch.cat([first, first, s[:, TILE:]], 1), K)
    idx = torch.where(order < TILE, order, order - TILE).to(torch.int32)
    assert "(a)" in assert_rejects(idx, vals, q, g, K, what="a slice merged twice")


def test_query_scale_left_out():
    B, N, D = 37, 1003, 64
    q, g = _randn(B, N, D, seed=6)
    idx, vals = _select(_scores32(q, g, True), K)
    assert_topk(idx, vals, q, g, K, True, True)
    idx, vals = _select(_scores32(q, g, True, q_scale=False), K)
    assert "(c)" in assert_rejects(idx, vals, q, g, K, True, True, what="no query scale")

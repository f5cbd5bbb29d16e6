"""tests/_knn_ref.py checked on the CPU, on rows worked by hand: the replay of
the k-NN vote rule (csrc/kernels/knn_vote.hip) and the masked exact ranking
the filtered-search tests compare csrc/kernels/sim_topk.hip with.
"""
import numpy as np
import torch

from _knn_ref import masked_topk, vote_replay

INF = float("inf")
LABELS = torch.tensor([0, 1, 2, 1, 0, 2, 7], dtype=torch.int32)  # of gallery rows 0..6


def _vote(idx, score, weighted, **kw):
    label, share = vote_replay(torch.tensor(idx, dtype=torch.int32), torch.tensor(score, dtype=torch.float32), LABELS,
                               weighted, **kw)
    assert label.dtype == torch.int32 and share.dtype == torch.float32
    return label.tolist(), share.tolist()


def test_tie_decided_by_best_rank():
    # labels 1 0 1 0: 2 - 2, label 1 holds rank 0
    assert _vote([[1, 0, 3, 4]], [[.9, .8, .7, .6]], False) == ([1], [0.5])
    # labels 0 1 0 1
    assert _vote([[0, 1, 4, 3]], [[.9, .8, .7, .6]], False) == ([0], [0.5])
    # the wrong rule (lowest label) differs on the first row only
    assert _vote([[1, 0, 3, 4]], [[.9, .8, .7, .6]], False, tie="label") == ([0], [0.5])
    assert _vote([[0, 1, 4, 3]], [[.9, .8, .7, .6]], False, tie="label") == ([0], [0.5])
    # 2 - 1 - 1: label 2 (ranks 1 and 3) beats rank 0's label
    assert _vote([[6, 2, 0, 5]], [[.9, .8, .7, .6]], False) == ([2], [0.5])


def test_weighted_and_clamped():
    # labels 0 1 1 0 with weights 0.5, 0.25, 0.125, max(-4, 0) = 0: label 0 has 0.5, label 1 0.375, all 0.875
    label, share = _vote([[0, 1, 3, 4]], [[.5, .25, .125, -4.]], True)
    assert label == [0] and share == [float(np.float32(0.5) / np.float32(0.875))]
    # unclamped, label 0 would have -3.5 and lose
    # sequential float32 adds: (1 + 2^-24) + 2^-24 = 1 in float32, 1 + (2^-24 + 2^-24) is not
    e = 2.0 ** -24
    label, share = _vote([[0, 4, 0]], [[1., e, e]], True)
    assert label == [0] and share == [1.0]
    label, share = _vote([[1, 0, 4]], [[1., e, e]], True)   # label 1: 1; label 0: 2^-23; all: (1 + e) + e = 1
    assert label == [1] and share == [1.0]


def test_missing_ranks_are_skipped():
    # ranks 0 and 2 are empty; labels of the rest: 2 1 2
    assert _vote([[-1, 2, -1, 3, 5]], [[-INF, .9, -INF, .8, .7]], False) == ([2], [float(np.float32(2) / np.float32(3))])
    label, share = _vote([[-1, 2, -1, 3, 5]], [[-INF, .5, -INF, .25, .25]], True)
    assert label == [2] and share == [0.75]


def test_no_voters():
    assert _vote([[-1, -1, -1]], [[-INF, -INF, -INF]], False) == ([-1], [0.0])
    assert _vote([[-1, -1, -1]], [[-INF, -INF, -INF]], True) == ([-1], [0.0])


def test_all_weights_zero():
    # every score <= 0: totals all 0, rank 0's label wins by the best-rank rule, share 0
    assert _vote([[6, 0, 1]], [[0., -1., -2.]], True) == ([7], [0.0])
    assert _vote([[6, 0, 1]], [[0., -1., -2.]], True, tie="label") == ([0], [0.0])


def test_several_rows_at_once():
    idx = [[1, 0, 3, 4], [-1, -1, -1, -1], [6, 6, 6, 6]]
    score = [[.9, .8, .7, .6], [-INF] * 4, [1., 1., 1., 1.]]
    assert _vote(idx, score, False) == ([1, -1, 7], [0.5, 0.0, 1.0])


def _brute(q, g, k, g_label, q_want):
    B, N = q.shape[0], g.shape[0]
    idx = torch.full((B, k), -1, dtype=torch.int32)
    score = torch.full((B, k), -INF, dtype=torch.float32)
    for b in range(B):
        cand = []
        for n in range(N):
            if g_label[n] < 0 or (q_want is not None and q_want[b] >= 0 and g_label[n] != q_want[b]):
                continue
            cand.append((-sum(float(q[b, d]) * float(g[n, d]) for d in range(q.shape[1])), n))
        for j, (neg, n) in enumerate(sorted(cand)[:k]):   # descending score, equal scores by ascending n
            idx[b, j], score[b, j] = n, -neg
    return idx, score


def test_masked_ranking_against_brute_force():
    gen = torch.Generator().manual_seed(0)
    q = torch.randint(-2, 3, (3, 4), generator=gen).float()
    g = torch.randint(-2, 3, (9, 4), generator=gen).float()
    g[5] = g[2]                                                     # a tie across a removed row
    g_label = torch.tensor([0, 1, 1, -1, 0, 1, 2, -1, 1], dtype=torch.int32)
    for q_want in (None, torch.tensor([1, -1, 3], dtype=torch.int32)):   # class 3 has no rows
        for k in (1, 4, 9):
            got = masked_topk(q, g, k, g_label, q_want)
            want = _brute(q, g, k, g_label, q_want)
            assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (q_want, k)
    idx, score = masked_topk(q, g, 9, g_label, torch.tensor([1, -1, 3], dtype=torch.int32))
    assert (idx[2] == -1).all() and (score[2] == -INF).all()       # nobody has label 3
    assert (idx[0, :4] >= 0).all() and (idx[0, 4:] == -1).all()    # four rows of label 1
    assert (idx[1, :7] >= 0).all() and (idx[1, 7:] == -1).all()    # seven live rows
    assert set(idx[1, :7].tolist()) == {0, 1, 2, 4, 5, 6, 8}

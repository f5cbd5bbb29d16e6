"""ops.knn_vote (csrc/kernels/knn_vote.hip) against the host replay of its
rule (tests/_knn_ref.py, checked by hand in test_knn_ref_cpu.py): label and
share bit for bit. Labels from 3 classes so that ties are common, some ranks
empty (idx = -1, score = -inf) and one query with none filled, scores of both
signs, sentinel-tailed outputs. Negative control: the replay with ties broken
by the lowest label instead of the best rank must differ from the kernel on
inputs that are checked, on the CPU, to contain such a tie.
"""
import pytest
import torch

from _knn_ref import vote_replay
from dmlc import ops

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PAD = 64
N = 50
INF = float("inf")


def _inputs(B, k, seed):
    gen = torch.Generator().manual_seed(seed)
    g_label = torch.randint(0, 3, (N,), generator=gen).to(torch.int32)
    g_label[0], g_label[1] = 2, 0
    idx = torch.stack([torch.randperm(N, generator=gen)[:k] for _ in range(B)]).to(torch.int32)
    # eighths: sums of up to 16 are exact, so weighted totals tie as well
    score = (torch.randint(-8, 17, (B, k), generator=gen).float() / 8)
    if k >= 3 and B >= 5:
        # a 1 - 1 tie (and a weighted 1.0 - 1.0 tie) between rank 0's label 2 and rank 1's label 0
        idx[3, :3] = torch.tensor([0, 1, -1], dtype=torch.int32)
        idx[3, 3:] = -1
        score[3, :2] = 1.0
    empty = torch.rand(B, k, generator=gen) < 0.2
    if B >= 5:
        empty[3] = idx[3] < 0
        empty[B - 1] = True                  # one query with no voter
    idx[empty] = -1
    score[empty] = -INF
    return idx, score, g_label


def _vote(idx, score, g_label, weighted, gpu):
    B = idx.shape[0]
    lbuf = torch.full((B + PAD,), -7, dtype=torch.int32, device=gpu)
    sbuf = torch.full((B + PAD,), SENTINEL, dtype=torch.float32, device=gpu)
    label, share = ops.knn_vote(idx.to(gpu), score.to(gpu), g_label.to(gpu), weighted, out=(lbuf[:B], sbuf[:B]))
    torch.cuda.synchronize()
    assert label.data_ptr() == lbuf.data_ptr() and share.data_ptr() == sbuf.data_ptr()
    assert (lbuf[B:] == -7).all() and (sbuf[B:] == SENTINEL).all()
    return label.cpu(), share.cpu()


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("B", [1, 5, 70])
def test_knn_vote(gpu, B, k, weighted):
    idx, score, g_label = _inputs(B, k, seed=100 * B + k)
    want_l, want_s = vote_replay(idx, score, g_label, weighted)
    label, share = _vote(idx, score, g_label, weighted, gpu)
    assert label.dtype == torch.int32 and share.dtype == torch.float32
    assert torch.equal(label, want_l), (label.tolist(), want_l.tolist())
    assert torch.equal(share, want_s)
    if B >= 5:
        assert int(label[B - 1]) == -1 and float(share[B - 1]) == 0.0
    # without out=: new tensors, the same answer
    l2, s2 = ops.knn_vote(idx.to(gpu), score.to(gpu), g_label.to(gpu), weighted)
    assert torch.equal(l2.cpu(), label) and torch.equal(s2.cpu(), share)
    if B >= 5 and k >= 3:
        # the negative control: query 3 is a tie that the lowest-label rule decides the other way
        wrong_l, _ = vote_replay(idx, score, g_label, weighted, tie="label")
        assert int(want_l[3]) == 2 and int(wrong_l[3]) == 0 and float(want_s[3]) == 0.5
        assert not torch.equal(label, wrong_l)


def test_ties_are_common():
    """(CPU) The inputs hold ties beyond the planted one: queries where the two tie rules disagree."""
    n = 0
    for weighted in (False, True):
        idx, score, g_label = _inputs(70, 16, seed=7016)
        a, _ = vote_replay(idx, score, g_label, weighted)
        b, _ = vote_replay(idx, score, g_label, weighted, tie="label")
        n += int((a != b).sum())
    assert n >= 2


def test_bad_arguments(gpu):
    idx = torch.zeros(4, 5, dtype=torch.int32, device=gpu)
    score = torch.zeros(4, 5, device=gpu)
    lab = torch.zeros(9, dtype=torch.int32, device=gpu)
    bad = [
        lambda: ops.knn_vote(idx.long(), score, lab),
        lambda: ops.knn_vote(idx, score.double(), lab),
        lambda: ops.knn_vote(idx, score[:, :4].contiguous(), lab),
        lambda: ops.knn_vote(idx, score, lab.long()),
        lambda: ops.knn_vote(idx, score, lab.cpu()),
        lambda: ops.knn_vote(idx, score, lab[:0]),
        lambda: ops.knn_vote(torch.zeros(4, 17, dtype=torch.int32, device=gpu), torch.zeros(4, 17, device=gpu), lab),
        lambda: ops.knn_vote(idx, score, lab, out=(torch.zeros(3, dtype=torch.int32, device=gpu),
                                                   torch.zeros(4, device=gpu))),
    ]
    for f in bad:
        with pytest.raises((ValueError, RuntimeError)):
            f()
    # an id past the labels does not vote (nothing is read out of bounds)
    idx[0] = torch.tensor([9, 100, 2 ** 31 - 1, 3, -5], dtype=torch.int32)
    label, share = ops.knn_vote(idx, score, lab + 4)
    torch.cuda.synchronize()
    assert label.tolist() == [4] * 4 and share.tolist() == [1.0] * 4

"""Host references of the labelled-gallery tests (test_knn_ref_cpu.py,
test_search_filter_gpu.py, test_knn_vote_gpu.py, test_gallery_labels_gpu.py).

vote_replay: csrc/kernels/knn_vote.hip's rule in numpy float32 with sequential
adds, so the kernel's label and share can be compared bit for bit. Rank j
votes iff idx >= 0, with label g_label[idx] and weight 1 or max(score, 0); a
label's total is the float32 sum of its ranks' weights in ascending rank order
from 0; the largest total wins, equal totals by the best (lowest) rank; share
= the winner's total / the float32 sum of all voting weights in ascending rank
order, 0 if that is 0; no voter: (-1, 0). tie="label" is the wrong rule the
negative control uses: equal totals by the lowest label.

masked_topk: the float64 stable ranking of _search_bar.exact_topk with the
rows that fail the filter dropped and the ranks nobody fills as (-1, -inf).
"""
import numpy as np
import torch

from _search_bar import stable_topk


def vote_replay(idx, score, g_label, weighted=False, tie="rank"):
    """(label int32 [B], share float32 [B]) of idx / score [B, k] (tensors or arrays) and g_label [N]."""
    idx = np.asarray(torch.as_tensor(idx).cpu()).astype(np.int64)
    score = np.asarray(torch.as_tensor(score).cpu()).astype(np.float32)
    g_label = np.asarray(torch.as_tensor(g_label).cpu()).astype(np.int64)
    B, k = idx.shape
    label, share = np.full(B, -1, np.int32), np.zeros(B, np.float32)
    for b in range(B):
        totals, best, everything = {}, {}, np.float32(0)
        for j in range(k):
            if idx[b, j] < 0:
                continue
            lab = int(g_label[idx[b, j]])
            w = np.maximum(score[b, j], np.float32(0)) if weighted else np.float32(1)
            totals[lab] = np.float32(totals.get(lab, np.float32(0)) + np.float32(w))
            best.setdefault(lab, j)
            everything = np.float32(everything + np.float32(w))
        if not totals:
            continue
        order = (lambda lab: (-totals[lab], best[lab])) if tie == "rank" else (lambda lab: (-totals[lab], lab))
        win = min(totals, key=order)
        label[b] = win
        share[b] = np.float32(totals[win]) / everything if everything != 0 else np.float32(0)
    return torch.from_numpy(label), torch.from_numpy(share)


def allowed(g_label, q_want, B):
    """bool [B, N]: row n is a candidate of query b."""
    g_label = torch.as_tensor(g_label).cpu().long()
    ok = (g_label >= 0)[None, :].expand(B, -1)
    if q_want is not None:
        q_want = torch.as_tensor(q_want).cpu().long()
        ok = ok & ((q_want < 0)[:, None] | (g_label[None, :] == q_want[:, None]))
    return ok


def masked_ranking(ref, k, ok):
    """ref float64 [B, N], ok bool [B, N] -> (idx int64 [B, k], ref's values float64 [B, k]); (-1, -inf) where a
    query has fewer than k candidates. Finite scores assumed."""
    order, _ = stable_topk(ref.masked_fill(~ok, -float("inf")), k)
    real = ok.gather(1, order)
    return order.masked_fill(~real, -1), ref.gather(1, order).masked_fill(~real, -float("inf"))


def masked_topk(q, g, k, g_label, q_want=None):
    """exact_topk under the filter: small-integer operands, (idx int32, score float32) bit for bit."""
    ref = q.cpu().double() @ g.cpu().double().t()
    assert float(ref.abs().max()) < 2 ** 24
    idx, vals = masked_ranking(ref, k, allowed(g_label, q_want, ref.shape[0]))
    return idx.to(torch.int32), vals.to(torch.float32)

"""The row filter of the nearest-neighbour search (csrc/kernels/sim_topk.hip's
FILTER instantiations through ops.sim_topk(g_label=, q_want=)): a row is a
candidate only if its label is >= 0 and, where the query wants a label, equal
to it; ranks nobody fills are (-1, -inf).

Exact. Small-integer operands (every fp32 sum exact, ties plentiful): idx and
score equal tests/_knn_ref.py's masked float64 stable ranking bit for bit, fp32
and bf16 queries, every slice count. The cases: fewer live rows than k; the
one-row second tile removed, and alone alive; half the rows removed with
wanted classes of which one is empty, one has one row in each of the 8 tiles
and one has exactly 16 rows (two per tile: N = 1000 has 8 tiles, so 16 rows
cannot lie one per tile); two query blocks whose wants differ between query b
and b + 256; every live row in the last slice.

Removed winners: a removed row that would have scored best by far never
appears; with every score negative neither a padding row nor a removed row
wins. bf16 randn, dot and cosine: the filtered answer equals the unfiltered
kernel's on the gathered candidate rows with the ids mapped back (a score's
bits do not depend on N or on the row's place in its tile, and the id map is
monotone, so no tolerance is involved), for all live rows and per wanted
class, the same bits at 1 and 7 slices; the same comparison refuses the answer
when the labels are rolled by one row. Outputs go to sentinel-tailed buffers.
"""
import pytest
import torch

import dmlc
from _knn_ref import allowed, masked_topk
from dmlc import native, ops

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PAD = 64
K = 16
INF = float("inf")


def _search(q, g, k, q_scale=None, g_scale=None, slices=None, g_label=None, q_want=None):
    """ops.sim_topk into sentinel-tailed buffers; the tails must stay untouched."""
    B = q.shape[0]
    ibuf = torch.full((B * k + PAD,), -7, dtype=torch.int32, device=q.device)
    sbuf = torch.full((B * k + PAD,), SENTINEL, dtype=torch.float32, device=q.device)
    kw = {}
    if g_label is not None:
        kw["g_label"] = g_label.to(q.device)
    if q_want is not None:
        kw["q_want"] = q_want.to(q.device)
    idx, score = ops.sim_topk(q, g, k, q_scale, g_scale, out=(ibuf[:B * k].view(B, k), sbuf[:B * k].view(B, k)),
                              slices=slices, **kw)
    torch.cuda.synchronize()
    assert idx.data_ptr() == ibuf.data_ptr() and score.data_ptr() == sbuf.data_ptr()
    assert (ibuf[B * k:] == -7).all() and (sbuf[B * k:] == SENTINEL).all()
    return idx, score


def _slice_counts(N):
    most = native().sim_topk_max_slices(N)
    return [None] + sorted({s for s in (1, 2, 7, most) if s <= most})


def _ints(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-3, 4, (B, D), generator=g).float(),
            torch.randint(-3, 4, (N, D), generator=g).float().bfloat16())


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32)


def _assert_exact(q, g, k, gpu, g_label, q_want=None, slice_counts=None):
    want_i, want_s = masked_topk(q, g, k, g_label, q_want)
    gd = g.to(gpu)
    for slices in slice_counts or _slice_counts(g.shape[0]):
        for bf in (False, True):
            qd = (q.bfloat16() if bf else q).to(gpu)
            idx, score = _search(qd, gd, k, slices=slices, g_label=g_label, q_want=q_want)
            assert torch.equal(idx.cpu(), want_i), (slices, bf)
            assert torch.equal(score.cpu(), want_s), (slices, bf)
    return want_i, want_s


def test_exact_fewer_live_than_k(gpu):
    B, N, D, k = 3, 17, 64, 16
    q, g = _ints(B, N, D, seed=B + N + D)
    g_label = torch.zeros(N, dtype=torch.int32)
    g_label[[0, 1, 2, 4, 5, 7, 8, 10, 11, 13, 14, 16]] = -1   # 12 of 17, the last row among them
    want_i, want_s = _assert_exact(q, g, k, gpu, g_label)
    assert (want_i[:, :5] >= 0).all() and (want_i[:, 5:] == -1).all() and (want_s[:, 5:] == -INF).all()
    _assert_exact(q, g, k, gpu, g_label, _i32([0, -1, 0]))


def test_exact_one_row_tile(gpu):
    B, N, D, k = 17, 129, 512, 5
    q, g = _ints(B, N, D, seed=B + N + D)
    g_label = torch.zeros(N, dtype=torch.int32)
    g_label[128] = -1                                  # the second tile's only row
    _assert_exact(q, g, k, gpu, g_label)
    g_label = torch.full((N,), -1, dtype=torch.int32)
    g_label[128] = 3                                   # nothing but that row
    want_i, _ = _assert_exact(q, g, k, gpu, g_label)
    assert (want_i[:, 0] == 128).all() and (want_i[:, 1:] == -1).all()
    want = _i32([3 if b % 2 else 2 for b in range(B)])
    want_i, _ = _assert_exact(q, g, k, gpu, g_label, want)
    assert (want_i[0::2] == -1).all() and (want_i[1::2, 0] == 128).all()


def test_exact_classes(gpu):
    B, N, D, k = 37, 1000, 2048, 16
    q, g = _ints(B, N, D, seed=B + N + D)
    gen = torch.Generator().manual_seed(1)
    g_label = torch.randint(0, 4, (N,), generator=gen).to(torch.int32)     # classes 0..3 at random
    g_label[torch.rand(N, generator=gen) < 0.5] = -1                       # about half removed
    tiles = (N + 127) // 128
    assert tiles == 8
    for t in range(tiles):
        g_label[128 * t + 5 * t] = 4                   # class 4: one row per tile
        g_label[128 * t + 3] = 5                       # class 5: exactly 16 rows, two per tile
        g_label[min(N - 1, 128 * t + 127)] = 5
    assert int((g_label == 4).sum()) == 8 and int((g_label == 5).sum()) == 16 and int((g_label == 6).sum()) == 0
    assert 0.4 < float((g_label < 0).float().mean()) < 0.6
    q_want = _i32([b % 7 for b in range(B)])           # class 6 has no rows
    want_i, want_s = _assert_exact(q, g, k, gpu, g_label, q_want)
    assert (want_i[6::7] == -1).all() and (want_s[6::7] == -INF).all()
    assert (want_i[5::7] >= 0).all()                   # all 16 rows of class 5, every rank filled
    assert (want_i[4::7, :8] >= 0).all() and (want_i[4::7, 8:] == -1).all()
    _assert_exact(q, g, k, gpu, g_label)               # any live row


def test_exact_two_query_blocks(gpu):
    B, N, D, k = 300, 1031, 512, 16
    q, g = _ints(B, N, D, seed=B + N + D)
    gen = torch.Generator().manual_seed(2)
    g_label = torch.randint(-1, 5, (N,), generator=gen).to(torch.int32)
    q_want = _i32([(b % 6) - 1 if b < 256 else ((b + 3) % 6) - 1 for b in range(B)])
    # an offset of b0 left out would give query b + 256 query b's want
    assert all(int(q_want[b]) != int(q_want[b + 256]) for b in range(B - 256))
    assert bool((q_want < 0).any()) and bool((q_want >= 0).any())
    assert bool((q_want[256:] < 0).any()) and bool((q_want[256:] >= 0).any())
    _assert_exact(q, g, k, gpu, g_label, q_want)


def test_exact_all_live_rows_in_the_last_slice(gpu):
    B, N, D, k = 5, 1031, 64, 16
    q, g = _ints(B, N, D, seed=B + N + D)
    C = native()
    most = C.sim_topk_max_slices(N)
    for slices in (4, most):
        first, end = C.sim_topk_slice_rows(N, slices, slices - 1)
        assert end == N
        g_label = torch.full((N,), -1, dtype=torch.int32)
        g_label[first:] = _i32([n % 3 for n in range(first, N)])
        for q_want in (None, _i32([0, 1, 2, -1, 7])):
            want_i, _ = _assert_exact(q, g, k, gpu, g_label, q_want, slice_counts=[slices])
            assert int(want_i[want_i >= 0].min()) >= first
    # (at the maximum the last slice is the 7-row tile: fewer candidates than k)
    assert N - first == 7 and (want_i[4] == -1).all() and (want_i[3, 7:] == -1).all()


def test_removed_winners(gpu):
    B, N, D, slices = 5, 1031, 64, 4
    q, g = _ints(B, N, D, seed=7)
    C = native()
    rows = []
    for i in range(slices):
        first, end = C.sim_topk_slice_rows(N, slices, i)
        rows += [first, end - 1]
    assert rows[-1] == N - 1 and N % 128
    for i, n in enumerate(rows):       # the first and last row of every slice: 3 x a query, its best row by far
        g[n] = (3 * q[i % B]).bfloat16()
    from _search_bar import exact_topk
    assert bool((exact_topk(q, g, K)[0][:, 0] == torch.tensor(rows[:B])).all())   # unfiltered, they win
    g_label = torch.zeros(N, dtype=torch.int32)
    g_label[rows] = -1
    for s in (slices, 1, 2, C.sim_topk_max_slices(N), None):
        want_i, _ = _assert_exact(q, g, K, gpu, g_label, slice_counts=[s])
        idx, _ = _search(q.to(gpu), g.to(gpu), K, slices=s, g_label=g_label)
        assert not bool(torch.isin(idx.cpu().long(), torch.tensor(rows)).any())
        assert (idx >= 0).all()


@pytest.mark.parametrize("N", [17, 129])
def test_all_negative(gpu, N):
    q, g = _ints(9, N, 64, seed=N)
    q, g = q.abs() + 1, -(g.float().abs() + 1).bfloat16()
    k = min(K, N)
    g_label = _i32([n % 3 for n in range(N)])
    g_label[1::4] = -1
    g_label[N - 1] = -1
    q_want = _i32([-1, 0, 1, 2, 5, -1, 0, 1, 2])
    removed = (g_label < 0).nonzero().flatten()
    for want in (None, q_want):
        want_i, want_s = _assert_exact(q, g, k, gpu, g_label, want)
        assert float(want_s[want_i >= 0].max()) < 0
        for slices in _slice_counts(N):
            idx, score = _search(q.to(gpu), g.to(gpu), k, slices=slices, g_label=g_label, q_want=want)
            idx = idx.cpu().long()
            assert int(idx.max()) < N and int(idx.min()) >= -1          # no padding row
            assert not bool(torch.isin(idx, removed).any())             # no removed row
            assert bool(((idx == -1) == (score.cpu() == -INF)).all())


RANDOM = [(37, 5003, 512, 16), (256, 20011, 512, 16)]


def _compacted(qb, qinv, gb, ginv, k, ok):
    """The answer the filter must give, from the unfiltered kernel: for every distinct row of ok (bool [B, N] on
    the CPU: the candidates of a query), the unfiltered search of its queries over the gathered candidate rows at
    k' = min(k, their number), ids mapped back through the (ascending) candidate list; the rest (-1, -inf)."""
    B = qb.shape[0]
    idx = torch.full((B, k), -1, dtype=torch.int32)
    score = torch.full((B, k), -INF, dtype=torch.float32)
    patterns, which = torch.unique(ok.to(torch.uint8), dim=0, return_inverse=True)
    for p in range(patterns.shape[0]):
        rows = patterns[p].nonzero().flatten()
        sel = (which == p).nonzero().flatten()
        if rows.numel() == 0:
            continue
        kk = min(k, rows.numel())
        rd, sd = rows.to(qb.device), sel.to(qb.device)
        i, s = ops.sim_topk(qb[sd].contiguous(), gb[rd].contiguous(), kk,
                            None if qinv is None else qinv[sd].contiguous(),
                            None if ginv is None else ginv[rd].contiguous())
        idx[sel, :kk] = rows[i.cpu().long()].to(torch.int32)
        score[sel, :kk] = s.cpu()
    return idx, score


@pytest.mark.parametrize("shape", RANDOM, ids=lambda s: "-".join(map(str, s)))
def test_filtered_equals_unfiltered_on_compacted(gpu, shape):
    B, N, D, k = shape
    gen = torch.Generator().manual_seed(N + D)
    q32, g32 = torch.randn(B, D, generator=gen), torch.randn(N, D, generator=gen)
    g_label = torch.randint(0, 7, (N,), generator=gen).to(torch.int32)
    g_label[torch.rand(N, generator=gen) < 0.3] = -1
    q_want = _i32([b % 7 for b in range(B)])
    gb, ginv = ops.gallery_pack(g32.to(gpu), with_norms=True)
    qb, qinv = ops.gallery_pack(q32.to(gpu), with_norms=True)
    rolled = g_label.roll(1)
    assert bool((allowed(rolled, None, 1) != allowed(g_label, None, 1)).any())
    for name, qs, gs in (("dot", None, None), ("cosine", qinv, ginv)):
        for want in (None, q_want):
            idx, score = _search(qb, gb, k, qs, gs, g_label=g_label, q_want=want)
            idx, score = idx.cpu(), score.cpu()
            exp_i, exp_s = _compacted(qb, qs, gb, gs, k, allowed(g_label, want, B))
            assert (exp_i >= 0).all()                     # (every class has more than k live rows here)
            assert torch.equal(idx, exp_i) and torch.equal(score, exp_s), (name, want is not None)
            for slices in (1, 7):
                i2, s2 = _search(qb, gb, k, qs, gs, slices=slices, g_label=g_label, q_want=want)
                assert torch.equal(i2.cpu(), idx) and torch.equal(s2.cpu(), score), (name, slices)
            # the negative control: the same comparison against the labels rolled by one row
            bad_i, bad_s = _compacted(qb, qs, gb, gs, k, allowed(rolled, want, B))
            n_diff = int((bad_i != idx).sum())
            print(f"control {name} want={want is not None}: {n_diff} of {B * k} ids differ under rolled labels")
            assert not (torch.equal(idx, bad_i) and torch.equal(score, bad_s))


def test_small_class_against_compacted(gpu):
    """A wanted class with fewer rows than k: the unfiltered search at k' = the class size, the rest (-1, -inf)."""
    B, N, D, k = 9, 700, 512, 16
    gen = torch.Generator().manual_seed(5)
    q32, g32 = torch.randn(B, D, generator=gen), torch.randn(N, D, generator=gen)
    g_label = torch.randint(0, 2, (N,), generator=gen).to(torch.int32)
    g_label[[3, 130, 131, 699]] = 2                     # class 2: 4 rows in 3 tiles; class 3: none
    q_want = _i32([b % 4 for b in range(B)])
    gb, ginv = ops.gallery_pack(g32.to(gpu), with_norms=True)
    qb, qinv = ops.gallery_pack(q32.to(gpu), with_norms=True)
    for slices in (None, 1, 2):
        idx, score = _search(qb, gb, k, qinv, ginv, slices=slices, g_label=g_label, q_want=q_want)
        exp_i, exp_s = _compacted(qb, qinv, gb, ginv, k, allowed(g_label, q_want, B))
        assert torch.equal(idx.cpu(), exp_i) and torch.equal(score.cpu(), exp_s)
    assert (exp_i[2::4, :4] >= 0).all() and (exp_i[2::4, 4:] == -1).all() and (exp_i[3::4] == -1).all()


def test_no_filter_arguments(gpu):
    """Every label 0 and no wants: the filtered kernel gives the unfiltered call's bits."""
    for B, N, D, k in ((37, 5003, 512, 16), (300, 1031, 64, 5)):
        gen = torch.Generator().manual_seed(N)
        gb, ginv = ops.gallery_pack(torch.randn(N, D, generator=gen).to(gpu), with_norms=True)
        qb, qinv = ops.gallery_pack(torch.randn(B, D, generator=gen).to(gpu), with_norms=True)
        zeros = torch.zeros(N, dtype=torch.int32)
        for qs, gs in ((None, None), (qinv, ginv)):
            for slices in (None, 1, 7):
                a = _search(qb, gb, k, qs, gs, slices=slices)
                b = _search(qb, gb, k, qs, gs, slices=slices, g_label=zeros)
                c = _search(qb, gb, k, qs, gs, slices=slices, g_label=zeros, q_want=torch.full((B,), -1).int())
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
                assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_bad_arguments(gpu):
    q = torch.zeros(2, 64, device=gpu)
    g = torch.zeros(40, 64, dtype=torch.bfloat16, device=gpu)
    lab = torch.zeros(40, dtype=torch.int32, device=gpu)
    want = torch.zeros(2, dtype=torch.int32, device=gpu)
    bad = [
        lambda: ops.sim_topk(q, g, 1, q_want=want),                          # q_want without g_label
        lambda: ops.sim_topk(q, g, 1, g_label=lab.long()),
        lambda: ops.sim_topk(q, g, 1, g_label=lab.float()),
        lambda: ops.sim_topk(q, g, 1, g_label=lab[:39]),
        lambda: ops.sim_topk(q, g, 1, g_label=lab.cpu()),
        lambda: ops.sim_topk(q, g, 1, g_label=lab, q_want=want.long()),
        lambda: ops.sim_topk(q, g, 1, g_label=lab, q_want=torch.zeros(3, dtype=torch.int32, device=gpu)),
        lambda: ops.sim_topk(q, g, 1, g_label=lab, q_want=want.cpu()),
    ]
    for f in bad:
        with pytest.raises((ValueError, RuntimeError)):
            f()
    C = native()
    idx = torch.full((2, 16), -7, dtype=torch.int32, device=gpu)
    score = torch.full((2, 16), SENTINEL, device=gpu)
    ws = torch.empty(C.sim_topk_ws_bytes(2, 16, 1), dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):                                          # the native check
        C.sim_topk(q.data_ptr(), C.TensorDType.F32, 0, g.data_ptr(), 0, 2, 40, 64, 16, idx.data_ptr(),
                   score.data_ptr(), ws.data_ptr(), ws.numel(), 256, torch.cuda.current_stream().cuda_stream,
                   q_want=want.data_ptr())
    torch.cuda.synchronize()
    assert (idx == -7).all() and (score == SENTINEL).all()

    # the Gallery's checks
    gen = torch.Generator().manual_seed(3)
    feats = torch.randn(12, 64, generator=gen).to(gpu)
    gal = dmlc.Gallery(64, 16, metric="dot", max_batch=8)
    for labels in ([0] * 11, [0] * 13, [0] * 11 + [-1], torch.zeros(12), torch.zeros(12, dtype=torch.int32)[:, None],
                   torch.full((12,), -2, dtype=torch.int64, device=gpu)):
        with pytest.raises(ValueError):
            gal.add(feats, labels=labels)
    assert len(gal) == 0 and gal.live == 0
    assert gal.add(feats, labels=[n % 3 for n in range(12)]) == range(0, 12)
    assert (len(gal), gal.live) == (12, 12)
    gal.remove([4])
    before = gal.search(feats[:8].contiguous(), 4)
    lab_before = gal.labels()
    for ids in ([12], [-1], [0, 1, 12], [0, -1], torch.tensor([2, 99]), [1.0]):
        with pytest.raises(ValueError):
            gal.remove(ids)
    with pytest.raises(ValueError):                                          # the bound C++ check: nothing removed
        gal._g.remove([0, 1, 12], torch.cuda.current_stream().cuda_stream)
    assert (len(gal), gal.live) == (12, 11)
    after = gal.search(feats[:8].contiguous(), 4)
    assert torch.equal(gal.labels(), lab_before)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    for where in (torch.zeros(7, dtype=torch.int64), torch.zeros(9, dtype=torch.int32, device=gpu),
                  torch.zeros(8), torch.zeros(8, 1, dtype=torch.int64), [0] * 8, 1.5):
        with pytest.raises(ValueError):
            gal.search(feats[:8].contiguous(), 4, where=where)
    idx, score = gal.search(feats[:8].contiguous(), 4, where=1)
    # label 1: rows 1, 4 (removed), 7, 10
    assert set(idx[:, :3].flatten().tolist()) == {1, 7, 10} and (idx[:, 3] == -1).all() and (score[:, 3] == -INF).all()
    assert int(idx[1, 0]) == 1 and int(idx[7, 0]) == 7        # |v|^2 = 64 +- 11 against N(0, 8)
    torch.cuda.synchronize()

"""The e4m3 gallery on the GPU (csrc/kernels/sim_topk.hip's FP8 form,
gallery_pack8, dmlc.Gallery(dtype="e4m3"), InferenceEngine.index / search /
classify_knn).

gallery_pack8's codes and dot scales are compared bit for bit with the
reference quantiser (_e4m3_ref.py). The search is checked by
_search_bar.py, unchanged: dequantised codes and raw codes are bf16 values,
so for the dot metric the reference gets the dequantised operands and no
scales, for cosine the codes as bf16 tensors with the scale flags set. Its
bars hold for any fp32 summation order. Small integers are exact under the
rule (3 * 2^7 = 384 is an e4m3 value), so those answers are bit-equal to
exact_topk on the unquantised data.
"""
import numpy as np
import pytest
import torch

import dmlc
from _e4m3_ref import dequantise, planted, quantise
from _search_bar import EPS_SUM, assert_rejects, assert_topk, exact_topk
from dmlc import native, ops
from dmlc.models import state_dict_f32
from dmlc.models.calibrated import calibrated, mixed_images
from dmlc.runtime import InferenceEngine

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PAD = 64
K = 16


def _search(q, codes, scale, k, metric="dot", slices=None, g_label=None, q_want=None):
    """ops.sim_topk8 into sentinel-tailed buffers; the tails must stay untouched."""
    B = q.shape[0]
    ibuf = torch.full((B * k + PAD,), -7, dtype=torch.int32, device=q.device)
    sbuf = torch.full((B * k + PAD,), SENTINEL, dtype=torch.float32, device=q.device)
    idx, score = ops.sim_topk8(q, codes, scale, k, metric, out=(ibuf[:B * k].view(B, k), sbuf[:B * k].view(B, k)),
                               slices=slices, g_label=g_label, q_want=q_want)
    torch.cuda.synchronize()
    assert idx.data_ptr() == ibuf.data_ptr() and score.data_ptr() == sbuf.data_ptr()
    assert (ibuf[B * k:] == -7).all() and (sbuf[B * k:] == SENTINEL).all()
    return idx, score


def _rows_of(codes, rows):
    """codes[rows] (gathered through uint8: one byte an element)."""
    return codes.view(torch.uint8)[rows].contiguous().view(torch.float8_e4m3fn)


def _slice_counts(N):
    most = native().sim_topk_max_slices(N)
    return [None] + sorted({s for s in (1, 2, 7, most) if s <= most})


# ---------------------------------------------------------------- gallery_pack8
def _pack_rows(M, D):
    rows = torch.randn(M, D, generator=torch.Generator().manual_seed(M + D))
    rows *= torch.logspace(-20, 20, M, base=2.0)[torch.randperm(M, generator=torch.Generator().manual_seed(M))][:, None]
    if M > 2:
        rows[1] = 0                                      # e = 0, codes 0
        rows[2] = rows[2].clamp(-50, 50)
        rows[2, D // 2] = -448 * 2.0 ** -3               # amax exactly 56: e = 3
        rows[0] = rows[2]
        rows[0, 7] = float(np.nextafter(np.float32(56), np.float32(64)))  # just above: e = 2
    return rows


@pytest.mark.parametrize("M,D", [(1, 128), (5, 512), (67, 2048), (3, 4096)])
def test_gallery_pack8(gpu, M, D):
    rows32 = _pack_rows(M, D)
    for rows in (rows32, rows32.bfloat16()):
        want_c, want_s, e = quantise(rows, "dot")
        if M > 2 and rows.dtype == torch.float32:
            assert int(e[2]) == 3 and int(e[0]) == 2 and int(e[1]) == 0
        for metric in ("dot", "cosine"):
            cbuf = torch.full((M * D + PAD,), 0x55, dtype=torch.uint8, device=gpu)
            codes, scale = ops.gallery_pack8(rows.to(gpu), metric)
            # the native call again, into sentinel-tailed buffers
            sbuf = torch.full((M + PAD,), SENTINEL, device=gpu)
            C = native()
            C.gallery_pack8(rows.to(gpu).data_ptr(), C.TensorDType.BF16 if rows.dtype == torch.bfloat16
                            else C.TensorDType.F32, cbuf.data_ptr(), sbuf.data_ptr(), metric == "cosine", M, D,
                            torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert (cbuf[M * D:] == 0x55).all() and (sbuf[M:] == SENTINEL).all()
            assert codes.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32
            assert torch.equal(cbuf[:M * D].cpu(), codes.cpu().view(torch.uint8).flatten())
            assert torch.equal(sbuf[:M], scale)
            assert torch.equal(codes.cpu().view(torch.uint8), want_c.view(torch.uint8)), (rows.dtype, metric)
            if metric == "dot":
                assert torch.equal(scale.cpu(), want_s)
            else:
                ref = quantise(rows, "cosine")[1]
                err = (scale.double().cpu() - ref).abs() / ref
                print(f"gallery_pack8 M={M} D={D} {rows.dtype}: worst relative error / ((D + 4) 2^-24) = "
                      f"{err.max().item() / ((D + 4) * 2.0 ** -24):.3f}")
                assert (err <= (D + 4) * 2.0 ** -24).all()
                if M > 2:
                    assert scale[1].item() == float(np.float32(1) / np.float32(1e-12))


# ---------------------------------------------------------------- exact answers
def _ints(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (B, D), generator=g).float(), torch.randint(-3, 4, (N, D), generator=g).float()


def _assert_exact(q, g, k, gpu, slices_list):
    want_i, want_s = exact_topk(q, g, k)
    codes, scale = ops.gallery_pack8(g.to(gpu), "dot")
    for slices in slices_list:
        for bf in (False, True):
            qd = (q.bfloat16() if bf else q).to(gpu)
            idx, score = _search(qd, codes, scale, k, "dot", slices)
            assert torch.equal(idx.cpu(), want_i), (slices, bf)
            assert torch.equal(score.cpu(), want_s), (slices, bf)
    return want_i, want_s


# one row; k = N; a second tile of one row; a wave of queries past B = 17 and 4 K blocks; 16 K blocks; the full query
# block at the widest D; two query blocks (256 + 44) and 9 tiles
EXACT = [(1, 1, 128, 1), (1, 16, 128, 16), (3, 17, 128, 16), (17, 129, 512, 5), (37, 1000, 2048, 16),
         (256, 300, 4096, 16), (300, 1031, 512, 16)]


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "-".join(map(str, s)))
def test_exact(gpu, shape):
    B, N, D, k = shape
    q, g = _ints(B, N, D, seed=B + N + D)
    _assert_exact(q, g, k, gpu, _slice_counts(N))


@pytest.mark.parametrize("N", [17, 129])
def test_all_negative(gpu, N):
    q, g = _ints(9, N, 128, seed=N)
    q, g = q.abs().clamp_min(1), -g.abs().clamp_min(1)
    k = min(K, N)
    want_i, want_s = _assert_exact(q, g, k, gpu, _slice_counts(N))
    assert float(want_s.max()) < 0 and int(want_i.max()) < N and int(want_i.min()) >= 0


def test_planted_winners(gpu):
    B, N, D, slices = 5, 1031, 128, 4
    q, g = _ints(B, N, D, seed=7)
    q[q == 0] = 1
    C = native()
    rows = []
    for i in range(slices):
        first, end = C.sim_topk_slice_rows(N, slices, i)
        rows += [first, end - 1]
    assert rows[-1] == N - 1 and N % 128  # (row N - 1 of a partial tile)
    for i, n in enumerate(rows):  # 8 rows over 5 queries: 3 queries have their best row twice, in different slices
        g[n] = 3 * q[i % B].sign()
    want_i, want_s = exact_topk(q, g, K)
    assert bool((want_s[:3, 0] == want_s[:3, 1]).all()) and bool((want_i[:, 0] == torch.tensor(rows[:B])).all())
    _assert_exact(q, g, K, gpu, (slices, 1, 2, C.sim_topk_max_slices(N), None))


# ---------------------------------------------------------------- random data
RANDOM = [(37, 5003, 512, 16), (17, 1000, 2048, 16), (256, 20011, 512, 16)]


@pytest.mark.parametrize("shape", RANDOM, ids=lambda s: "-".join(map(str, s)))
def test_random(gpu, shape):
    B, N, D, k = shape
    gen = torch.Generator().manual_seed(N + D)
    q32, g32 = torch.randn(B, D, generator=gen), torch.randn(N, D, generator=gen)
    (cq, _, eq), (cg, _, eg) = quantise(q32), quantise(g32)
    qd, gd = q32.to(gpu), g32.to(gpu)
    answers = {}
    for metric in ("dot", "cosine"):
        codes, scale = ops.gallery_pack8(gd, metric)
        assert torch.equal(codes.cpu().view(torch.uint8), cg.view(torch.uint8))
        if metric == "dot":  # float64 on the dequantised operands, no scales
            ref_q, ref_g, flags = dequantise(cq, eq), dequantise(cg, eg).bfloat16(), (None, None)
        else:                # float64 cosine of the codes
            ref_q, ref_g, flags = cq.float(), cg.to(torch.bfloat16), (True, True)
        idx, score = _search(qd, codes, scale, k, metric)
        assert_topk(idx, score, ref_q, ref_g, k, *flags)
        for slices in (1, 7):
            i2, s2 = _search(qd, codes, scale, k, metric, slices)
            assert torch.equal(i2, idx) and torch.equal(s2, score), (metric, slices)
        answers[metric] = (idx, score, ref_q, ref_g.roll(1, 0), flags)
    # the negative control: the same answers against the gallery rolled by one row
    for metric, (idx, score, ref_q, rolled, flags) in answers.items():
        assert_rejects(idx, score, ref_q, rolled, k, *flags, what=f"{metric}, rolled gallery")


def test_planted_neighbours(gpu):
    q, g = planted()
    codes, scale = ops.gallery_pack8(g.to(gpu), "cosine")
    idx, score = _search(q.to(gpu), codes, scale, K, "cosine")
    want = 16 * torch.arange(q.shape[0])[:, None] + torch.arange(16)[None, :]
    assert torch.equal(idx.cpu().long(), want)
    steps = 0.9 - 0.04 * torch.arange(16, dtype=torch.float64)
    print(f"planted neighbours: worst |score - planted cosine| = {(score.cpu().double() - steps).abs().max().item():.4f}")
    assert float((score.cpu().double() - steps).abs().max()) < 0.02  # (half a step: the codes' rounding is ~0.002)


# ---------------------------------------------------------------- the row filter
@pytest.mark.parametrize("slices", [1, 4])
def test_filter(gpu, slices):
    B, N, D, k = 9, 1031, 512, 16
    gen = torch.Generator().manual_seed(31)
    q, g = torch.randn(B, D, generator=gen), torch.randn(N, D, generator=gen)
    labels = torch.randint(0, 6, (N,), generator=gen).to(torch.int32)
    labels[torch.tensor([5, 400, 1030])] = 6             # a class of 3 rows: fewer than k candidates
    labels[::3] = -1                                      # every third row removed (row 1030 = 3 * 343 + 1 stays)
    want = torch.tensor([0, 1, -1, 6, 2, -5, 3, 6, 5], dtype=torch.int32)
    codes, scale = ops.gallery_pack8(g.to(gpu), "cosine")
    qd = q.to(gpu)
    idx, score = _search(qd, codes, scale, k, "cosine", slices, labels.to(gpu), want.to(gpu))
    short = 0
    for b in range(B):
        ok = (labels >= 0) & ((labels == want[b]) if want[b] >= 0 else torch.ones(N, dtype=torch.bool))
        rows = ok.nonzero()[:, 0].to(gpu)
        kk = min(k, len(rows))
        # (a gathered gallery: the scores' bits do not depend on N or on a row's place)
        i2, s2 = _search(qd[b:b + 1], _rows_of(codes, rows), scale[rows].contiguous(), kk, "cosine", 1)
        assert torch.equal(idx[b, :kk].long(), rows[i2[0].long()]) and torch.equal(score[b, :kk], s2[0]), b
        assert (idx[b, kk:] == -1).all() and (score[b, kk:] == float("-inf")).all(), b
        short += kk < k
    assert short == 2
    # removed rows only, no q_want
    idx, score = _search(qd, codes, scale, k, "cosine", slices, labels.to(gpu))
    rows = (labels >= 0).nonzero()[:, 0].to(gpu)
    i2, s2 = _search(qd, _rows_of(codes, rows), scale[rows].contiguous(), k, "cosine", 1)
    assert torch.equal(idx.long(), rows[i2.long()]) and torch.equal(score, s2)


def test_bad_arguments(gpu):
    q = torch.zeros(2, 128, device=gpu)
    codes, scale = ops.gallery_pack8(torch.ones(40, 128, device=gpu), "dot")
    bad = [
        lambda: ops.gallery_pack8(torch.zeros(2, 96, device=gpu)),
        lambda: ops.gallery_pack8(torch.zeros(2, 128, device=gpu).half()),
        lambda: ops.gallery_pack8(torch.zeros(2, 128, device=gpu), "l2"),
        lambda: ops.gallery_pack8(torch.zeros(2, 128)),
        lambda: ops.sim_topk8(q, codes, scale, 0),
        lambda: ops.sim_topk8(q, codes, scale, 17),
        lambda: ops.sim_topk8(q, codes[:9], scale[:9], 10),
        lambda: ops.sim_topk8(q, codes.view(torch.uint8), scale, 1),
        lambda: ops.sim_topk8(q, codes.float().bfloat16(), scale, 1),
        lambda: ops.sim_topk8(q, codes, None, 1),
        lambda: ops.sim_topk8(q, codes, scale[:39], 1),
        lambda: ops.sim_topk8(q, codes, scale, 1, "l2"),
        lambda: ops.sim_topk8(q[:, :64], codes, scale, 1),
        lambda: ops.sim_topk8(q.cpu(), codes, scale, 1),
        lambda: ops.sim_topk8(q, codes, scale, 1, slices=2),       # one tile only
        lambda: ops.sim_topk8(q, codes, scale, 1, q_want=torch.zeros(2, dtype=torch.int32, device=gpu)),
        lambda: ops.sim_topk8(q, codes, scale, 1, g_label=torch.zeros(40, dtype=torch.int64, device=gpu)),
        lambda: ops.sim_topk(q, codes, 1),                          # the bf16 search takes no codes
    ]
    for f in bad:
        with pytest.raises((ValueError, RuntimeError)):
            f()
    idx, score = ops.sim_topk8(q + 1, codes, scale, 16, "dot")
    assert (score == 128).all() and torch.equal(idx[0].cpu(), torch.arange(16, dtype=torch.int32))


# ---------------------------------------------------------------- Gallery and engine
@pytest.fixture(scope="module")
def r18():
    model = calibrated("resnet18", seed=11)
    return model, InferenceEngine("resnet18", state_dict_f32(model), max_batch=32)


def _self_bar(D):
    return (2 * D + 8) * EPS_SUM


def test_gallery_and_engine(gpu, r18):
    from dmlc.models.calibrated import normalize
    model, eng = r18
    D = eng.feature_dim
    u8 = mixed_images(32, seed=72)
    with torch.no_grad():
        assert len(set(model(normalize(u8)).argmax(-1).tolist())) >= 8
    img = u8.to(gpu)
    before = eng.predict(img, return_logits=True)
    gal = dmlc.Gallery(D, 40, metric="cosine", max_batch=32, dtype="e4m3")
    assert (gal.dim, gal.capacity, gal.metric, gal.dtype, len(gal), gal.live) == (D, 40, "cosine", "e4m3", 0, 0)
    assert dmlc.Gallery(D, 8).dtype == "bf16"
    class_of = torch.arange(32, dtype=torch.int32) % 5
    assert eng.index(img[:16], gal, labels=class_of[:16]) == range(0, 16)
    assert eng.index(img[16:], gal, labels=class_of[16:]) == range(16, 32)
    assert len(gal) == 32 and gal.live == 32 and torch.equal(gal.labels().cpu(), class_of)
    ids = torch.arange(32, dtype=torch.int32, device=gpu)

    # (the rows compared bit for bit come from batches of 16, as index() made them)
    feats = torch.cat([eng.embed(img[:16]), eng.embed(img[16:])])
    idx, score = gal.search(feats, 4)
    assert idx.shape == (32, 4) and idx.dtype == torch.int32 and score.dtype == torch.float32
    assert torch.equal(idx[:, 0], ids)
    print(f"self-similarity: worst |score - 1| / bar = {((score[:, 0].double() - 1).abs().max() / _self_bar(D)).item():.3f}")
    assert ((score[:, 0].double() - 1).abs() <= _self_bar(D)).all()
    # the Gallery is the kernels on the same rows, bit for bit
    codes, scale = ops.gallery_pack8(feats, "cosine")
    ki, ks = ops.sim_topk8(feats, codes, scale, 4, "cosine")
    assert torch.equal(ki, idx) and torch.equal(ks, score)
    # the negative control for "ignores its input": a batch rolled by one image finds the rolled ids
    for half, want in ((img[:16], ids[:16]), (img[16:], ids[16:])):
        ridx, rscore = eng.search(half.roll(1, 0), gal, k=4)
        assert torch.equal(ridx[:, 0], want.roll(1))
        assert ((rscore[:, 0].double() - 1).abs() <= _self_bar(D)).all()
    # engine.search is gallery.search of embed(), eager and graph
    for use_graph in (True, False):
        a = eng.search(img, gal, k=5, use_graph=use_graph)
        b = gal.search(eng.embed(img, use_graph=use_graph), 5)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    # classify_knn, where and remove against a bf16 gallery of the same rows: every image's nearest row is itself
    # in both (the premise, checked), so k = 1 votes and filtered first ranks agree
    ref = dmlc.Gallery(D, 40, metric="cosine", max_batch=32)
    ref.add(feats, labels=class_of)
    assert torch.equal(ref.search(feats, 1)[0][:, 0], ids) and torch.equal(gal.search(feats, 1)[0][:, 0], ids)
    la, sa = gal.classify(feats, 1)
    lb, sb = ref.classify(feats, 1)
    assert torch.equal(la, lb) and torch.equal(la.cpu(), class_of) and torch.equal(sa, sb)
    le, _ = eng.classify_knn(img[:16], gal, k=1)
    assert torch.equal(le.cpu(), class_of[:16])
    own = class_of.to(gpu)
    wa, wb = gal.search(feats, 1, where=own), ref.search(feats, 1, where=own)
    assert torch.equal(wa[0], wb[0]) and torch.equal(wa[0][:, 0], ids)
    other = (own + 1) % 5                                   # another class: never the image itself
    wa = gal.search(feats, 2, where=other)[0]
    assert bool((gal.labels()[wa.long().flatten()] == other.repeat_interleave(2)).all())
    for g_ in (gal, ref):
        g_.remove(range(0, 32, 2))
    assert len(gal) == 32 and gal.live == 16 and torch.equal(gal.labels().cpu(), ref.labels().cpu())
    assert bool((gal.labels()[::2] == -1).all())
    ra, rb = gal.search(feats[1::2].contiguous(), 1), ref.search(feats[1::2].contiguous(), 1)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[0][:, 0], ids[1::2])
    assert not bool((gal.search(feats, 16)[0] % 2 == 0).any())   # no removed row at any rank; 16 live rows
    la, lb = gal.classify(feats[1::2].contiguous(), 1)[0], ref.classify(feats[1::2].contiguous(), 1)[0]
    assert torch.equal(la, lb) and torch.equal(la.cpu(), class_of[1::2])
    few = gal.search(feats[:2].contiguous(), 16, where=torch.tensor([0, 4]))   # class 0: rows 5, 15, 25 live
    assert few[0][0].tolist()[3:] == [-1] * 13 and bool((few[1][0, 3:] == float("-inf")).all())
    assert sorted(few[0][0].tolist()[:3]) == [5, 15, 25]

    # predict is untouched
    after = eng.predict(img, return_logits=True)
    torch.cuda.synchronize()
    for a, b in zip(before, after):
        assert torch.equal(a, b)

    # the dot metric: the Gallery is the kernels on the same rows
    dot = dmlc.Gallery(D, 32, metric="dot", max_batch=32, dtype="e4m3")
    dot.add(feats)
    di, ds = dot.search(feats, 4)
    codes, scale = ops.gallery_pack8(feats, "dot")
    ki, ks = ops.sim_topk8(feats, codes, scale, 4, "dot")
    assert torch.equal(ki, di) and torch.equal(ks, ds)

    # errors
    with pytest.raises(ValueError):
        dmlc.Gallery(96, 8, dtype="e4m3")
    with pytest.raises(ValueError):
        native().Gallery(96, 8, 0, "cosine", 8, "e4m3")
    with pytest.raises(ValueError):
        dmlc.Gallery(128, 8, dtype="fp8")
    with pytest.raises(ValueError):
        native().Gallery(128, 8, 0, "cosine", 8, "fp8")
    with pytest.raises(ValueError):
        gal.search(feats, 17)
    with pytest.raises(ValueError):
        gal.search(feats.cpu(), 1)                   # wrong device
    with pytest.raises(ValueError):
        eng.index(img[:9], gal)                      # 32 + 9 > 40
    with pytest.raises(ValueError):
        eng.search(img, dmlc.Gallery(128, 8, dtype="e4m3"), 1)   # dim != feature_dim
    assert len(gal) == 32

    # clear() then add reuses ids from 0 and forgets the removals
    gal.clear()
    assert len(gal) == 0 and gal.live == 0
    assert gal.add(feats[8:16].contiguous()) == range(0, 8) and gal.live == 8
    idx, _ = gal.search(feats[8:16].contiguous(), 1)
    assert torch.equal(idx[:, 0], ids[:8]) and bool((gal.labels() == 0).all())
    torch.cuda.synchronize()


@pytest.mark.parametrize("arch,D", [("resnet50", 2048), ("alexnet", 4096)])
def test_other_feature_widths(gpu, arch, D):
    eng = InferenceEngine(arch, state_dict_f32(calibrated(arch, seed=11)), max_batch=4)
    assert eng.feature_dim == D
    img = mixed_images(4, seed=90).to(gpu)
    gal = dmlc.Gallery(D, 4, max_batch=4, dtype="e4m3")
    assert eng.index(img, gal) == range(0, 4)
    idx, score = eng.search(img, gal, k=4)
    ref = gal.search(eng.embed(img), 4)
    torch.cuda.synchronize()
    assert torch.equal(idx, ref[0]) and torch.equal(score, ref[1])
    assert torch.equal(idx[:, 0].cpu(), torch.arange(4, dtype=torch.int32))
    assert ((score[:, 0].double() - 1).abs() <= _self_bar(D)).all()
    feats = eng.embed(img)
    codes, scale = ops.gallery_pack8(feats, "cosine")
    ki, ks = ops.sim_topk8(feats, codes, scale, 4, "cosine")
    assert torch.equal(ki, idx) and torch.equal(ks, score)

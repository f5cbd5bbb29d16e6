"""Nearest-neighbour search over embeddings: the kernels
(csrc/kernels/sim_topk.hip through ops.sim_topk / ops.gallery_pack), the
runtime object (csrc/runtime/gallery.cpp through dmlc.Gallery) and the engine
(InferenceEngine.index / search).

Kernel. Small-integer operands make every fp32 sum exact (|sum| <= 9 * 4096 <
2^24) and ties plentiful: idx and score must equal the float64 stable
descending sort bit for bit, for every slice count. All-negative scores: no
row that pads a partial tile may win. Planted winners at the first and last
row of every slice and at row N - 1, with duplicate rows in different slices:
equal scores across the merge follow the tie rule. bf16 randn: conditions
(a)-(e) of tests/_search_bar.py under the dot metric (fp32 and bf16 queries)
and the cosine metric (scales from ops.gallery_pack), the same bits for every
slice count, and the same comparison refuses the answer against the gallery
rolled by one row. Outputs go to sentinel-tailed buffers.

Gallery / engine, on calibrated models and mixed_images (>= 8 distinct fp32
top-1 classes, as test_embed_gpu.py): an image finds itself at rank 0 with a
cosine score within the bar of 1 ((2 D + 8) 2^-23: mag rq rg = 1 for a vector
against itself); a batch rolled by one image finds the rolled ids;
engine.search equals gallery.search(engine.embed()) bit for bit; predict
returns the same bits before and after. The Gallery's answers are compared
bit for bit with ops.sim_topk on the packed rows, not with assert_topk: at
B k = 128 one swapped near tie is 2 positions, above condition (e)'s 1 %.

Measured on an MI355X: worst |err| / bar 0.0022 (dot) and 0.0011 (cosine) at
(256, 20011, 512), no position off the float64 ranking at any shape; the
rolled-gallery controls miss the bar by 367 to 9010 times; gallery_pack's
inverse norms reach 0.075 of their bar (D = 8), self-similarity 0.004 of its.
"""
import numpy as np
import pytest
import torch

import dmlc
from _search_bar import EPS_SUM, assert_rejects, assert_topk, bf16r, exact_topk, inv_norm64
from dmlc import native, ops
from dmlc.models import state_dict_f32
from dmlc.models.calibrated import calibrated, mixed_images, normalize
from dmlc.runtime import InferenceEngine

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PAD = 64
K = 16


def _search(q, g, k, q_scale=None, g_scale=None, slices=None):
    """ops.sim_topk into sentinel-tailed buffers; the tails must stay untouched."""
    B = q.shape[0]
    ibuf = torch.full((B * k + PAD,), -7, dtype=torch.int32, device=q.device)
    sbuf = torch.full((B * k + PAD,), SENTINEL, dtype=torch.float32, device=q.device)
    idx, score = ops.sim_topk(q, g, k, q_scale, g_scale, out=(ibuf[:B * k].view(B, k), sbuf[:B * k].view(B, k)),
                              slices=slices)
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


def _assert_exact(q, g, k, gpu, slices, want=None):
    want_i, want_s = want or exact_topk(q, g, k)
    for bf in (False, True):
        qd = (q.bfloat16() if bf else q).to(gpu)
        idx, score = _search(qd, g.to(gpu), k, slices=slices)
        assert torch.equal(idx.cpu(), want_i), (slices, bf)
        assert torch.equal(score.cpu(), want_s), (slices, bf)


# one tile of one row; k = N; a second tile of one row; 2 tiles with a 2-row wave of queries past B = 17; 8 tiles
# and 32 K blocks; the full query block at the widest D; two query blocks (256 + 44) and 9 tiles
EXACT = [(1, 1, 32, 1), (1, 16, 32, 16), (3, 17, 64, 16), (17, 129, 512, 5), (37, 1000, 2048, 16),
         (256, 300, 4096, 16), (300, 1031, 512, 16)]


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "-".join(map(str, s)))
def test_exact(gpu, shape):
    B, N, D, k = shape
    q, g = _ints(B, N, D, seed=B + N + D)
    want = exact_topk(q, g, k)
    for slices in _slice_counts(N):
        _assert_exact(q, g, k, gpu, slices, want)


def test_exact_k_block_of_32(gpu):
    """D % 64 == 32: the last K block is half a stage."""
    q, g = _ints(5, 200, 96, seed=96)
    for slices in (1, 2):
        _assert_exact(q, g, 7, gpu, slices)


@pytest.mark.parametrize("N", [17, 129])
def test_all_negative(gpu, N):
    q, g = _ints(9, N, 64, seed=N)
    q, g = q.abs() + 1, -(g.float().abs() + 1).bfloat16()
    k = min(K, N)
    assert float(exact_topk(q, g, k)[1].max()) < 0
    for slices in _slice_counts(N):
        _assert_exact(q, g, k, gpu, slices)
        idx, _ = _search(q.to(gpu), g.to(gpu), k, slices=slices)
        assert int(idx.max()) < N and int(idx.min()) >= 0


def test_planted_winners(gpu):
    B, N, D, slices = 5, 1031, 64, 4
    q, g = _ints(B, N, D, seed=7)
    C = native()
    rows = []
    for i in range(slices):
        first, end = C.sim_topk_slice_rows(N, slices, i)
        rows += [first, end - 1]
    assert rows[-1] == N - 1 and N % 128  # (row N - 1 of a partial tile)
    for i, n in enumerate(rows):  # 8 rows over 5 queries: 3 queries have their best row twice, in different slices
        g[n] = (3 * q[i % B]).bfloat16()
    want_i, want_s = exact_topk(q, g, K)
    assert bool((want_s[:3, 0] == want_s[:3, 1]).all()) and bool((want_i[:, 0] == torch.tensor(rows[:B])).all())
    for s in (slices, 1, 2, C.sim_topk_max_slices(N), None):
        _assert_exact(q, g, K, gpu, s)


RANDOM = [(37, 5003, 512, 16), (17, 1000, 2048, 16), (256, 20011, 512, 16)]


@pytest.fixture(scope="module")
def random_data():
    cache = {}

    def get(shape):
        if shape not in cache:
            B, N, D, _ = shape
            gen = torch.Generator().manual_seed(N + D)
            cache[shape] = (torch.randn(B, D, generator=gen), torch.randn(N, D, generator=gen))
        return cache[shape]
    return get


@pytest.mark.parametrize("shape", RANDOM, ids=lambda s: "-".join(map(str, s)))
def test_random(gpu, random_data, shape):
    B, N, D, k = shape
    q32, g32 = random_data(shape)  # fp32 randn: the kernel rounds the queries, gallery_pack the rows
    qd = q32.to(gpu)
    gb, ginv = ops.gallery_pack(g32.to(gpu), with_norms=True)
    qb, qinv = ops.gallery_pack(qd, with_norms=True)
    g_cpu = gb.cpu()
    assert torch.equal(g_cpu, g32.bfloat16()) and torch.equal(qb.cpu(), q32.bfloat16())
    answers = {}
    for name, args in (("dot fp32", (qd, None, None)), ("dot bf16", (qb, None, None)), ("cosine", (qb, qinv, ginv))):
        idx, score = _search(args[0], gb, k, args[1], args[2])
        assert_topk(idx, score, q32, g_cpu, k, args[1], args[2])
        for slices in (1, 7):
            i2, s2 = _search(args[0], gb, k, args[1], args[2], slices=slices)
            assert torch.equal(i2, idx) and torch.equal(s2, score), (name, slices)
        answers[name] = (idx, score)
    assert torch.equal(answers["dot fp32"][0], answers["dot bf16"][0])
    assert torch.equal(answers["dot fp32"][1], answers["dot bf16"][1])
    # the negative control: the same answer against the gallery rolled by one row
    rolled = g_cpu.roll(1, 0)
    assert_rejects(*answers["dot fp32"], q32, rolled, k, what="dot, rolled gallery")
    assert_rejects(*answers["cosine"], q32, rolled, k, True, True, what="cosine, rolled gallery")


@pytest.mark.parametrize("M,D", [(1, 8), (5, 512), (67, 2048), (3, 4096), (2, 8192)])
def test_gallery_pack(gpu, M, D):
    rows = torch.randn(M, D, generator=torch.Generator().manual_seed(M + D))
    if M > 2:
        rows[1] = 0
    g, inv = ops.gallery_pack(rows.to(gpu), with_norms=True)
    torch.cuda.synchronize()
    assert g.dtype == torch.bfloat16 and torch.equal(g.cpu(), rows.bfloat16())
    assert torch.equal(ops.gallery_pack(rows.to(gpu)), g)
    # fp32 sum of D non-negative terms halved by the root, the root and the divide at 2^-24 each: (D / 2 + 2) 2^-24,
    # doubled as the project's summation terms are
    ref = inv_norm64(bf16r(rows))
    err = (inv.double().cpu() - ref).abs() / ref
    print(f"gallery_pack M={M} D={D}: worst relative error / ((D + 4) 2^-24) = {err.max().item() / ((D + 4) * 2.0 ** -24):.3f}")
    assert (err <= (D + 4) * 2.0 ** -24).all()
    if M > 2:
        assert inv[1].item() == float(np.float32(1) / np.float32(1e-12))
        if D % 32 == 0 and D <= 4096:
            q = torch.randn(4, D, generator=torch.Generator().manual_seed(1)).to(gpu)
            k = min(M, K)
            idx, score = _search(q, g, k, None, inv)
            assert bool((score[idx == 1] == 0).all()) and (k < M or int((idx == 1).sum()) == 4)


def test_bad_arguments(gpu):
    q = torch.zeros(2, 64, device=gpu)
    g = torch.zeros(40, 64, dtype=torch.bfloat16, device=gpu)
    idx = torch.full((2, 16), -7, dtype=torch.int32, device=gpu)
    score = torch.full((2, 16), SENTINEL, device=gpu)
    bad = [
        lambda: ops.sim_topk(torch.zeros(2, 48, device=gpu), torch.zeros(40, 48, dtype=torch.bfloat16, device=gpu), 1),
        lambda: ops.sim_topk(q, g, 0),
        lambda: ops.sim_topk(q, g, 17),
        lambda: ops.sim_topk(q, g[:9], 10),
        lambda: ops.sim_topk(q.half(), g, 1),
        lambda: ops.sim_topk(q, g.float(), 1),
        lambda: ops.sim_topk(q[:, :32], g, 1),
        lambda: ops.sim_topk(q.cpu(), g, 1),
        lambda: ops.sim_topk(q, g, 1, slices=2),                       # one tile only
        lambda: ops.sim_topk(q, g, 1, q_scale=torch.ones(3, device=gpu)),
        lambda: ops.sim_topk(q, g, 1, g_scale=torch.ones(40, dtype=torch.float64, device=gpu)),
        lambda: ops.sim_topk(q, g, 16, out=(idx[:, :8], score[:, :8])),
        lambda: ops.gallery_pack(q.bfloat16()),
        lambda: ops.gallery_pack(torch.zeros(2, 12, device=gpu)),
    ]
    for f in bad:
        with pytest.raises((ValueError, RuntimeError)):
            f()
    # the native checks, past the Python ones
    C = native()
    F32 = C.TensorDType.F32
    ws = torch.empty(C.sim_topk_ws_bytes(2, 16, 1), dtype=torch.uint8, device=gpu)
    stream = torch.cuda.current_stream().cuda_stream

    def call(D=64, k=16, N=40, ws_bytes=ws.numel(), dt=F32, slices=0):
        C.sim_topk(q.data_ptr(), dt, 0, g.data_ptr(), 0, 2, N, D, k, idx.data_ptr(), score.data_ptr(), ws.data_ptr(),
                   ws_bytes, 256, stream, slices=slices)
    for kw in (dict(D=48), dict(k=0), dict(k=17), dict(k=10, N=9), dict(ws_bytes=ws.numel() - 1), dict(N=0),
               dict(dt=C.TensorDType.F16), dict(slices=2)):
        with pytest.raises(ValueError):
            call(**kw)
    torch.cuda.synchronize()
    assert (idx == -7).all() and (score == SENTINEL).all()  # nothing was launched
    call()
    torch.cuda.synchronize()
    assert (score == 0).all() and torch.equal(idx[0].cpu(), torch.arange(16, dtype=torch.int32))


# ---------------------------------------------------------------- Gallery and engine
@pytest.fixture(scope="module")
def r18():
    model = calibrated("resnet18", seed=11)
    return model, InferenceEngine("resnet18", state_dict_f32(model), max_batch=32)


def _self_bar(D):
    return (2 * D + 8) * EPS_SUM


def test_gallery_index_and_search(gpu, r18):
    model, eng = r18
    D = eng.feature_dim
    u8 = mixed_images(32, seed=72)
    with torch.no_grad():
        assert len(set(model(normalize(u8)).argmax(-1).tolist())) >= 8
    img = u8.to(gpu)
    gal = dmlc.Gallery(D, 40, metric="cosine", max_batch=32)
    assert (gal.dim, gal.capacity, gal.metric, len(gal)) == (D, 40, "cosine", 0)
    before = eng.predict(img, return_logits=True)
    # (a batch of 16 takes other kernels than one of 32 and its features differ in the last bf16 bit here and
    # there: the rows compared bit for bit below all come from the batch of 32)
    feats = eng.embed(img)
    assert gal.add(feats[:16]) == range(0, 16) and len(gal) == 16
    assert gal.add(feats[16:]) == range(16, 32) and len(gal) == 32
    ids = torch.arange(32, dtype=torch.int32, device=gpu)
    # index() = add(embed())
    gal16 = dmlc.Gallery(D, 16, max_batch=32)
    assert eng.index(img[:8], gal16) == range(0, 8) and eng.index(img[8:16], gal16) == range(8, 16)
    own, _ = gal16.search(eng.embed(img[8:16]), 1)
    assert len(gal16) == 16 and torch.equal(own[:, 0], ids[8:16])

    idx, score = eng.search(img, gal, k=4)
    torch.cuda.synchronize()
    assert idx.shape == (32, 4) and idx.dtype == torch.int32 and score.dtype == torch.float32
    assert torch.equal(idx[:, 0], ids)
    print(f"self-similarity: worst |score - 1| / bar = {((score[:, 0].double() - 1).abs().max() / _self_bar(D)).item():.3f}")
    assert ((score[:, 0].double() - 1).abs() <= _self_bar(D)).all()
    # the Gallery is the kernel on the packed rows, bit for bit (the kernel's own answer is checked above)
    gb, ginv = ops.gallery_pack(feats, with_norms=True)
    ki, ks = ops.sim_topk(feats, gb, 4, q_scale=ginv, g_scale=ginv)
    assert torch.equal(ki, idx) and torch.equal(ks, score)
    # the negative control for "ignores its input": a batch rolled by one image finds the rolled ids
    ridx, rscore = eng.search(img.roll(1, 0), gal, k=4)
    assert torch.equal(ridx[:, 0], ids.roll(1))
    assert ((rscore[:, 0].double() - 1).abs() <= _self_bar(D)).all()
    # engine.search is gallery.search of embed(), u8 and float-tensor images, eager and graph
    for x in (img, normalize(u8).to(gpu)):
        for use_graph in (True, False):
            a = eng.search(x, gal, k=5, use_graph=use_graph)
            b = gal.search(eng.embed(x, use_graph=use_graph), 5)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    out = (torch.empty(32, 4, dtype=torch.int32, device=gpu), torch.empty(32, 4, device=gpu))
    got = gal.search(feats.bfloat16(), 4, out=out)  # bf16 queries: what fp32 ones are rounded to
    assert got[0].data_ptr() == out[0].data_ptr() and torch.equal(out[0], idx) and torch.equal(out[1], score)
    # predict is untouched
    after = eng.predict(img, return_logits=True)
    torch.cuda.synchronize()
    for a, b in zip(before, after):
        assert torch.equal(a, b)

    # the dot metric on the same rows: the float64 dot of the rounded features
    dot = dmlc.Gallery(D, 32, metric="dot", max_batch=32)
    dot.add(feats)
    di, ds = dot.search(feats, 4)
    ki, ks = ops.sim_topk(feats, gb, 4)
    assert torch.equal(ki, di) and torch.equal(ks, ds)
    f64 = feats.double()  # (the features are bf16 values)
    want, mag = (f64 @ f64.t()).gather(1, di.long()), (f64.abs() @ f64.abs().t()).gather(1, di.long())
    assert ((ds.double() - want).abs() <= D * EPS_SUM * mag).all()

    # errors
    with pytest.raises(ValueError):
        eng.index(img[:9], gal)                      # 32 + 9 > 40
    assert len(gal) == 32
    with pytest.raises(ValueError):
        gal.search(feats, 17)
    with pytest.raises(ValueError):
        gal.search(feats[:, :256].contiguous(), 1)
    with pytest.raises(ValueError):
        gal.search(feats.cpu(), 1)                   # wrong device
    with pytest.raises(ValueError):
        gal.add(feats.double())
    with pytest.raises(ValueError):
        eng.search(img, dmlc.Gallery(64, 8), 1)      # dim != feature_dim
    with pytest.raises(ValueError):
        dmlc.Gallery(48, 8)
    with pytest.raises(ValueError):
        dmlc.Gallery(64, 8, metric="l2")

    class Elsewhere:
        dim, device = D, torch.device("cuda", 1)
    with pytest.raises(ValueError):
        eng.search(img, Elsewhere(), 1)
    with pytest.raises(ValueError):
        eng.index(img, Elsewhere())
    empty = dmlc.Gallery(D, 8, max_batch=32)
    with pytest.raises(ValueError):
        empty.search(feats, 1)
    with pytest.raises(ValueError):                   # the bound C++ check
        empty._g.search(feats.data_ptr(), native().TensorDType.F32, 4, 1, out[0].data_ptr(), out[1].data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    empty.add(feats[:3])
    with pytest.raises(ValueError):
        empty.search(feats, 4)                        # k > len
    with pytest.raises(ValueError):
        empty._g.add(feats.data_ptr(), 6, torch.cuda.current_stream().cuda_stream)

    # clear() then add reuses ids from 0
    gal.clear()
    assert len(gal) == 0
    assert gal.add(feats[8:16].contiguous()) == range(0, 8)
    idx, _ = gal.search(feats[8:16].contiguous(), 1)
    assert torch.equal(idx[:, 0], ids[:8])
    torch.cuda.synchronize()


@pytest.mark.parametrize("arch,D", [("resnet50", 2048), ("alexnet", 4096)])
def test_other_feature_widths(gpu, arch, D):
    eng = InferenceEngine(arch, state_dict_f32(calibrated(arch, seed=11)), max_batch=4)
    assert eng.feature_dim == D
    img = mixed_images(4, seed=90).to(gpu)
    gal = dmlc.Gallery(D, 4, max_batch=4)
    assert eng.index(img, gal) == range(0, 4)
    idx, score = eng.search(img, gal, k=4)
    ref = gal.search(eng.embed(img), 4)
    torch.cuda.synchronize()
    assert torch.equal(idx, ref[0]) and torch.equal(score, ref[1])
    assert torch.equal(idx[:, 0].cpu(), torch.arange(4, dtype=torch.int32))
    assert ((score[:, 0].double() - 1).abs() <= _self_bar(D)).all()
    feats = eng.embed(img)
    gb, ginv = ops.gallery_pack(feats, with_norms=True)
    ki, ks = ops.sim_topk(feats, gb, 4, q_scale=ginv, g_scale=ginv)
    assert torch.equal(ki, idx) and torch.equal(ks, score)

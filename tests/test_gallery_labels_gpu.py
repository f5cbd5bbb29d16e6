"""The labelled gallery through dmlc.Gallery and InferenceEngine: labels,
filtered search, removal and k-NN classification (csrc/runtime/gallery.cpp,
csrc/kernels/sim_topk.hip's row filter, csrc/kernels/knn_vote.hip).

On a calibrated ResNet18 and mixed_images(32, seed=72), labelled with the fp32
model's top-1 class (>= 8 distinct): every image classifies as its own label
at k = 1; classify_knn is ops.knn_vote of gallery.search(embed()) bit for bit,
eager and graph, u8 and float-tensor images; search(where=labels) returns only
rows of that label, the image itself first; removed rows never come back, the
rest still find themselves, and the answer is ops.sim_topk(g_label=labels())
bit for bit; a gallery without labels or removals answers as the unfiltered
kernel does; predict returns the same bits before and after.
"""
import pytest
import torch

import dmlc
from dmlc import ops
from dmlc.models import state_dict_f32
from dmlc.models.calibrated import calibrated, mixed_images, normalize
from dmlc.runtime import InferenceEngine

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def r18():
    model = calibrated("resnet18", seed=11)
    return model, InferenceEngine("resnet18", state_dict_f32(model), max_batch=32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_labelled_gallery(gpu, r18):
    model, eng = r18
    D = eng.feature_dim
    u8 = mixed_images(32, seed=72)
    with torch.no_grad():
        labels = model(normalize(u8)).argmax(-1).to(torch.int32)
    assert len(set(labels.tolist())) >= 8
    img, lab_d = u8.to(gpu), labels.to(gpu)
    ids = torch.arange(32, dtype=torch.int32, device=gpu)
    before = eng.predict(img, return_logits=True)
    feats = eng.embed(img)
    gb, ginv = ops.gallery_pack(feats, with_norms=True)

    # a fresh gallery without labels or removals: the unfiltered kernel's answer, labels all zero
    plain = dmlc.Gallery(D, 32, metric="cosine", max_batch=32)
    assert eng.index(img, plain) == range(0, 32) and (len(plain), plain.live) == (32, 32)
    assert _same(plain.search(feats, 4), ops.sim_topk(feats, gb, 4, q_scale=ginv, g_scale=ginv))
    assert _same(eng.search(img, plain, k=4), ops.sim_topk(feats, gb, 4, q_scale=ginv, g_scale=ginv))
    assert plain.labels().dtype == torch.int32 and torch.equal(plain.labels(), torch.zeros_like(ids))
    one, share = eng.classify_knn(img, plain, k=3)
    assert (one == 0).all() and (share == 1).all()

    gal = dmlc.Gallery(D, 40, metric="cosine", max_batch=32)
    assert eng.index(img[:16], gal, labels=labels[:16]) == range(0, 16)       # (a CPU tensor)
    assert eng.index(img[16:], gal, labels=lab_d[16:].tolist()) == range(16, 32)
    # (the rows of the two batches of 16 may differ from the batch of 32's in the last bf16 bit: what is compared
    # bit for bit below uses one gallery throughout)
    gal.clear()
    assert (len(gal), gal.live) == (0, 0)
    assert eng.index(img, gal, labels=lab_d) == range(0, 32) and (len(gal), gal.live) == (32, 32)
    assert torch.equal(gal.labels(), lab_d)

    # k = 1: every image is its own nearest row
    label, share = eng.classify_knn(img, gal, k=1)
    assert label.dtype == torch.int32 and share.dtype == torch.float32 and label.shape == share.shape == (32,)
    assert torch.equal(label, lab_d) and (share == 1).all()
    # classify_knn = knn_vote(search(embed)), eager and graph, u8 and float-tensor images
    for x in (img, normalize(u8).to(gpu)):
        for use_graph in (True, False):
            for weighted in (False, True):
                a = eng.classify_knn(x, gal, k=5, weighted=weighted, use_graph=use_graph)
                b = ops.knn_vote(*gal.search(eng.embed(x, use_graph=use_graph), 5), gal.labels(), weighted=weighted)
                assert _same(a, b)
                assert _same(a, gal.classify(eng.embed(x, use_graph=use_graph), 5, weighted))
    out = (torch.empty(32, dtype=torch.int32, device=gpu), torch.empty(32, device=gpu))
    got = eng.classify_knn(img, gal, k=5, out=out)
    assert got[0].data_ptr() == out[0].data_ptr() and _same(out, eng.classify_knn(img, gal, k=5))

    # where: only rows of the wanted label, the image itself first
    idx, score = eng.search(img, gal, k=4, where=lab_d)
    assert torch.equal(idx[:, 0], ids)
    found = torch.where(idx >= 0, lab_d[idx.clamp_min(0).long()], lab_d[:, None].expand(-1, 4))
    assert torch.equal(found, lab_d[:, None].expand(-1, 4))
    assert bool(((idx == -1) == (score == -INF)).all())
    counts = torch.bincount(labels.long())[labels.long()].to(gpu)            # rows of each image's label
    assert torch.equal((idx >= 0).sum(1), counts.clamp_max(4))
    assert _same((idx, score), ops.sim_topk(feats, gb, 4, q_scale=ginv, g_scale=ginv, g_label=lab_d, q_want=lab_d))
    assert _same((idx, score), eng.search(img, gal, k=4, where=labels.long()))   # (an int64 CPU tensor)
    c = int(labels[5])
    idx_c, _ = eng.search(img, gal, k=4, where=c)
    assert set(lab_d[idx_c[idx_c >= 0].long()].tolist()) == {c} and int(idx_c[5, 0]) == 5

    # remove
    gal.remove(range(8))
    assert (len(gal), gal.live) == (32, 24)
    assert torch.equal(gal.labels()[:8], torch.full_like(ids[:8], -1)) and torch.equal(gal.labels()[8:], lab_d[8:])
    idx, score = eng.search(img, gal, k=16)
    assert int(idx.min()) >= 8 and torch.equal(idx[8:, 0], ids[8:])
    assert _same((idx, score), ops.sim_topk(feats, gb, 16, q_scale=ginv, g_scale=ginv, g_label=gal.labels()))
    gal.remove(torch.tensor([3, 3, 7]))                                      # again: nothing changes
    gal.remove([])
    assert (len(gal), gal.live) == (32, 24)
    assert _same((idx, score), eng.search(img, gal, k=16))
    idx30, score30 = gal.search(feats, 16, where=-1)                         # the same search through q_want
    assert _same((idx30, score30), (idx, score))
    gal.remove(range(8, 20))                                                 # 12 live rows: ranks 12.. are empty
    idx, score = eng.search(img, gal, k=16)
    assert (idx[:, :12] >= 20).all() and (idx[:, 12:] == -1).all() and (score[:, 12:] == -INF).all()
    label, share = eng.classify_knn(img[20:], gal, k=1)
    assert torch.equal(label, lab_d[20:]) and (share == 1).all()
    assert _same(eng.classify_knn(img, gal, k=16), ops.knn_vote(idx, score, gal.labels()))

    # clear() then add starts again at id 0, every row live
    gal.clear()
    assert eng.index(img[8:16], gal) == range(0, 8) and (len(gal), gal.live) == (8, 8)
    assert torch.equal(gal.labels(), torch.zeros_like(ids[:8]))
    own, _ = gal.search(eng.embed(img[8:16]), 1)
    assert torch.equal(own[:, 0], ids[:8])

    # predict is untouched
    after = eng.predict(img, return_logits=True)
    torch.cuda.synchronize()
    for a, b in zip(before, after):
        assert torch.equal(a, b)

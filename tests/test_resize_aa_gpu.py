"""The ragged resize kernels (csrc/kernels/resize.hip) through
`ops.resize_u8_ragged`, plain and antialiased, against the fp64 oracle
(dmlc.utils.resize_ref), and a `--resize-antialias` node end to end.

The bar is tests/_resize_bar.py's. Where every filter weight is a multiple of
1/16 (the two-tap rule at scales 2, 8 and 10 samples at fractions of exactly
one half, so a quarter of its values are ties) fp32 is exact and a tie is not
excluded: it must round to even like every other value. The antialiased kernel
reads source rows straight from global memory (no LDS stage), so there is no
row width at which it changes path."""
import os
import struct

import numpy as np
import pytest
import torch

import dmlc
from dmlc import ops
from dmlc.utils.resize_ref import resize_exact

from _resize_bar import assert_bar, assert_envelope, sixteenths, two_tap_coordinate_eps

pytestmark = pytest.mark.gpu

# the S = 16 shapes of the CPU test, one launch: shrink, copy, wide, tall, enlarging, scale 10, scale 1.25
S16 = [(37, 53), (16, 16), (9, 40), (131, 17), (12, 10), (160, 200), (20, 28)]
# the serving size: a query-sized image, exactly scale 2, a photo (scale 6.9; 4 column blocks, 28 row strips)
S224 = [(375, 500), (448, 448), (1536, 2048)]
S8 = [(96, 64)]
# an S that is no multiple of the antialiased kernel's 8-row strip: its last strip has 4 rows
S12 = [(30, 41), (12, 12), (7, 5)]
# The two-tap kernel computes its sample coordinate in fp32. Over 1536 x 2048
# pixels that alone can move a value of a noise image by 0.086 grey levels
# (two_tap_coordinate_eps), and 17 % of such an image's values are that close
# to a half, so the bar's input condition cannot hold for it at any eps that
# is true of the kernel. That image is checked against the envelope instead:
# every value is the rounding of something within that distance of the exact
# one. The antialiased kernel's weights divide a coordinate error by the
# support (6.9 here), and it meets the bar on the same image.
TWO_TAP_COORDINATE_LIMITED = {(1536, 2048)}


@pytest.fixture(scope="module")
def cases():
    """(S, images, {antialias: [exact per image]}): the oracle, computed once."""
    rng = np.random.default_rng(0)
    out = []
    for S, shapes in ((16, S16), (224, S224), (8, S8), (12, S12)):
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
        out.append((S, imgs, {aa: [resize_exact(im, S, aa) for im in imgs] for aa in (True, False)}))
    return out


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "plain"])
def test_ragged_launches_meet_the_bar(gpu, cases, antialias):
    for S, imgs, exact in cases:
        dev = [torch.from_numpy(im).to(gpu) for im in imgs]
        got = ops.resize_u8_ragged(dev, S, antialias=antialias)
        assert got.shape == (len(imgs), S, S, 3) and got.dtype == torch.uint8
        got = got.cpu().numpy()
        for i, im in enumerate(imgs):
            h, w = im.shape[:2]
            what = f"{h}x{w} -> {S} antialias={antialias}"
            if not antialias and (h, w) in TWO_TAP_COORDINATE_LIMITED:
                assert_envelope(got[i], exact[antialias][i], two_tap_coordinate_eps(h, w), what)
            else:
                assert_bar(got[i], exact[antialias][i], what, sixteenths(h, w, S, antialias))


def test_checkerboard_is_averaged_only_with_the_flag(gpu):
    y, x = np.mgrid[0:48, 0:48]
    cb = torch.from_numpy(np.repeat((((x + y) % 2) * 254).astype(np.uint8)[:, :, None], 3, axis=2)).to(gpu)
    aa = ops.resize_u8_ragged([cb], 16, antialias=True)[0].cpu().numpy().astype(int)
    assert np.abs(aa - 127).max() <= 3, (aa.min(), aa.max())  # exact: 125.4 and 128.6
    plain = ops.resize_u8_ragged([cb], 16)[0].cpu().numpy()
    yy, xx = np.mgrid[0:16, 0:16]
    first = int(plain[0, 0, 0])
    assert first in (0, 254)
    assert (plain == np.where((xx + yy) % 2 == 0, first, 254 - first)[:, :, None]).all()


def test_resize_u8_ragged_validates_its_arguments(gpu):
    ok = torch.zeros(20, 30, 3, dtype=torch.uint8, device=gpu)
    assert ops.resize_u8_ragged([ok], 8).shape == (1, 8, 8, 3)
    with pytest.raises(RuntimeError):
        ops.resize_u8_ragged([ok.cpu()], 8)
    with pytest.raises(ValueError):
        ops.resize_u8_ragged([ok.float()], 8)
    with pytest.raises(ValueError):
        ops.resize_u8_ragged([torch.zeros(20, 30, 4, dtype=torch.uint8, device=gpu)], 8)
    with pytest.raises(ValueError):
        ops.resize_u8_ragged([ok], 10)
    with pytest.raises(ValueError):
        ops.resize_u8_ragged([ok.permute(1, 0, 2)], 8)  # not contiguous


def test_node_with_resize_antialias_answers_like_the_engine(gpu, tmp_path):
    """A mixed-size JPEG query (the sizes of test_node_gpu.py's ragged test)
    to a `--executor gpu --resize-antialias` node: the member's answer is the
    in-process engine's on `ops.resize_u8_ragged(decoded, antialias=True)`.
    Same decoder, same resize kernel, same engine at the same batch size, so
    the classes are equal; the probabilities are compared at 2 % relative,
    several times the bf16 step (0.4 %) a differently scheduled forward may
    move a logit by."""
    from dmlc.runtime import InferenceEngine
    from dmlc.serve import rpc
    from dmlc.serve.cluster import LocalCluster
    from dmlc.utils.dataset import make_synthetic_dataset, synthetic_labels, write_labels
    from dmlc.utils.ot import write_random_checkpoint
    labels = synthetic_labels(1000)
    lab = write_labels(str(tmp_path / "synset_words.txt"), labels)
    sizes = [(224, 224), (375, 500), (500, 333), (256, 300), (480, 640), (199, 211), (224, 300), (640, 427)]
    ds = make_synthetic_dataset(str(tmp_path / "ragged"), labels[:16], size=sizes, seed=9)
    ckpt = write_random_checkpoint("resnet18", str(tmp_path / "resnet18.ot"), seed=6, randomize_bn=True)
    port = 19950
    cl = LocalCluster(1, port, str(tmp_path / "c"), lab, n_leaders=1, executor="gpu", dataset=ds,
                      models=f"resnet18={ckpt}", extra=["--jobs", "resnet18", "--max-batch", "16", "--resize-antialias"])
    ids = [w for w, _ in labels[:16]]
    with cl:
        nd = cl.nodes[0]
        info = nd.cmd("info")
        assert "executor gpu:0" in info and "resize antialias" in info, info
        payload = rpc.s("resnet18") + struct.pack("<I", len(ids)) + b"".join(rpc.s(i) for i in ids)
        status, body = rpc.call("127.0.0.1", port + 2, rpc.M_PREDICT, payload, timeout=120)
    assert status == 0 and body[0] == 1, (status, body[:64])
    (n,) = struct.unpack_from("<I", body, 1)
    assert n == 16
    off, got = 5, []
    for _ in range(n):
        (p,) = struct.unpack_from("<d", body, off)
        (ln,) = struct.unpack_from("<I", body, off + 8)
        got.append((p, body[off + 12:off + 12 + ln].decode()))
        off += 12 + ln
    nat = dmlc.native()
    decoded = []
    for w in ids:
        d = os.path.join(ds, w)
        with open(os.path.join(d, sorted(os.listdir(d))[0]), "rb") as f:
            decoded.append(torch.from_numpy(nat.decode_jpeg(f.read())).to(gpu))
    eng = InferenceEngine("resnet18", ckpt, device=0, max_batch=16)
    idx, prob = eng.predict(ops.resize_u8_ragged(decoded, 224, antialias=True))
    torch.cuda.synchronize()
    idx, prob = idx.cpu().tolist(), prob.cpu().tolist()
    texts = [t for _, t in labels]
    assert [t for _, t in got] == [texts[i] for i in idx]
    for (p, _), q in zip(got, prob):
        assert abs(p - q) <= 0.02 * q, (p, q)

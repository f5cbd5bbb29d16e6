"""The antialiased serving resize on the host: the native `resize_u8_host`
(what the CPU executor and `decode_resize` use) against an fp64 transcription
of the rule (dmlc.utils.resize_ref), the oracle itself against torch, and
`dmlc-node classify --resize-antialias` end to end.

The bar is tests/_resize_bar.py's. One case cannot meet its input condition as
it stands: the two-tap rule at scale 10 (160x200 -> 16) samples at fractions
of exactly one half, so a quarter of its exact values are ties whatever the
pixels. Where every filter weight is a multiple of 1/16 (that case, 96x64 -> 8
and the copy) fp32 is exact, so there a tie is not excluded: it must round to
even like every other value, which asks more of the code, not less."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dmlc
from dmlc.serve.cluster import NODE_BIN
from dmlc.utils.resize_ref import resize_exact, resized_dims

from _resize_bar import assert_bar, sixteenths

# (h, w, S): a plain shrink, the copy case, wide, tall, enlarging, scale 10,
# scale 1.25, S = 8, a query-sized image at the serving size, and an S that is
# no multiple of the kernel's 8-row strip
SHAPES = [(37, 53, 16), (16, 16, 16), (9, 40, 16), (131, 17, 16), (12, 10, 16), (160, 200, 16), (20, 28, 16),
          (96, 64, 8), (375, 500, 224), (30, 41, 12)]


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(0)
    return {s: rng.integers(0, 256, (s[0], s[1], 3), dtype=np.uint8) for s in SHAPES}


def _torch_aa(img, S):
    h, w, _ = img.shape
    x = torch.from_numpy(img).permute(2, 0, 1)[None].double()
    rh, rw = resized_dims(h, w, S)
    r = F.interpolate(x, size=(rh, rw), mode="bilinear", antialias=True, align_corners=False)
    oy, ox = (rh - S) // 2, (rw - S) // 2
    return r[0, :, oy:oy + S, ox:ox + S].permute(1, 2, 0).numpy()


def _checkerboard():
    y, x = np.mgrid[0:48, 0:48]
    return np.repeat((((x + y) % 2) * 254).astype(np.uint8)[:, :, None], 3, axis=2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_agrees_with_torch_antialias(images, shape):
    err = np.abs(resize_exact(images[shape], shape[2], True) - _torch_aa(images[shape], shape[2])).max()
    assert err < 1e-6, err


@pytest.mark.parametrize("antialias", [True, False], ids=["aa", "plain"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resize_u8_host_meets_the_bar(images, shape, antialias):
    got = dmlc.native().resize_u8_host(images[shape], shape[2], antialias)
    assert got.dtype == np.uint8 and got.shape == (shape[2], shape[2], 3)
    assert_bar(got, resize_exact(images[shape], shape[2], antialias), f"{shape} antialias={antialias}",
               sixteenths(*shape, antialias))


def test_checkerboard_is_averaged_only_with_the_flag():
    """A one-pixel 0 / 254 checkerboard, 48 x 48 -> 16: the two-tap rule lands
    on single source pixels (the result is itself a checkerboard), the
    antialiased filter averages them (exact values 125.4 and 128.6)."""
    cb = _checkerboard()
    nat = dmlc.native()
    aa = nat.resize_u8_host(cb, 16, True).astype(int)
    assert np.abs(aa - 127).max() <= 3, (aa.min(), aa.max())
    plain = nat.resize_u8_host(cb, 16, False)
    y, x = np.mgrid[0:16, 0:16]
    want = plain[0, 0, 0] if plain[0, 0, 0] in (0, 254) else -1
    board = np.where((x + y) % 2 == 0, want, 254 - want)
    assert want != -1 and (plain == board[:, :, None]).all()


def test_decode_resize_antialias_is_the_host_resize(tmp_path):
    from PIL import Image
    from dmlc.utils.shards import decode_resize
    rng = np.random.default_rng(3)
    files = []
    for i, (h, w) in enumerate([(90, 70), (64, 64), (50, 120)]):
        p = str(tmp_path / f"{i}.JPEG")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p, quality=92)
        files.append(p)
    nat = dmlc.native()
    got = decode_resize(files, 32, antialias=True)
    assert got.shape == (3, 32, 32, 3) and got.dtype == np.uint8
    differs = False
    for i, p in enumerate(files):
        img = nat.decode_jpeg(open(p, "rb").read())
        assert (got[i] == nat.resize_u8_host(img, 32, True)).all()
        differs |= bool((got[i] != nat.resize_u8_host(img, 32, False)).any())
    assert differs


@pytest.mark.slow
def test_classify_cpu_with_resize_antialias_matches_reference(tmp_path):
    """`classify --executor cpu --resize-antialias` on one non-square noise
    JPEG: the class of the torch fp32 reference model on the oracle-resized
    image (the check of test_classify_cpu_matches_reference), and its
    probability as printed (two decimals of a percentage: +-0.005, plus the
    fp32 forward's own error, far below that). Without the flag the answer is
    the two-tap image's."""
    from PIL import Image
    from dmlc.models import build
    from dmlc.utils.dataset import synthetic_labels, write_labels
    from dmlc.utils.ot import write_random_checkpoint
    if not os.path.exists(NODE_BIN):
        pytest.fail("dmlc-node not built (python tools/build.py)")
    labels = write_labels(str(tmp_path / "synset_words.txt"), synthetic_labels(1000))
    ckpt = write_random_checkpoint("alexnet", str(tmp_path / "alexnet.ot"), seed=2)
    img_path = str(tmp_path / "noise.JPEG")
    Image.fromarray(np.random.default_rng(5).integers(0, 256, (375, 500, 3), dtype=np.uint8)).save(img_path, quality=95)
    rgb = dmlc.native().decode_jpeg(open(img_path, "rb").read())
    model = build("alexnet", seed=2)
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    for flag in (True, False):
        r = subprocess.run([NODE_BIN, "classify", "--model", "alexnet", "--weights", ckpt, "--labels", labels,
                            "--image", img_path, "--executor", "cpu"] + (["--resize-antialias"] if flag else []),
                           capture_output=True, text=True, timeout=120, env={**os.environ, "OMP_NUM_THREADS": "4"})
        assert r.returncode == 0, r.stderr
        m = re.search(r"\((\d+\.\d+)%\) class=(\d+)", r.stdout)
        assert m, r.stdout
        u8 = np.clip(np.rint(resize_exact(rgb, 224, flag)), 0, 255).astype(np.float32)
        x = (torch.from_numpy(u8).permute(2, 0, 1)[None] / 255 - mean) / std
        with torch.no_grad():
            p = torch.softmax(model(x), -1)[0]
        print(f"antialias={flag}: node class {m.group(2)} {m.group(1)} %, reference {int(p.argmax())} "
              f"{float(p.max()) * 100:.4f} %")
        assert int(m.group(2)) == int(p.argmax())
        assert abs(float(m.group(1)) - float(p.max()) * 100) <= 0.01

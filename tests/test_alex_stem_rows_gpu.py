"""ops.alex_stem_rows (alex_stem_rows.hip) on test_alex_stem's kind of images: bit for bit ops.alex_stem's
output, and against float64 on preprocess_u8's values under the pooled bar with K = 363 (_kernel_bar.py)."""
import pytest
import torch

from dmlc import ops

import _kernel_bar as kb

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", [1, 3])
def test_alex_stem_rows(gpu, B):
    g = torch.Generator().manual_seed(80 + B)
    img = torch.randint(0, 256, (B + 1, 224, 224, 3), generator=g, dtype=torch.uint8)
    img[B, 2:-2, 2:-2] = 0  # one more image, 255 on its outermost two rows and columns only: the padding taps
    img[B, :2], img[B, -2:], img[B, :, :2], img[B, :, -2:] = 255, 255, 255, 255
    w = (torch.randn(64, 3, 11, 11, generator=g) / 363 ** 0.5).bfloat16().double()
    bias = (torch.randn(64, generator=g) * 0.1).float().double()
    imd, wp, bd = img.to(gpu), ops.pack_alex_stem_weight(w.float(), device=gpu), bias.float().to(gpu)
    y = ops.alex_stem_rows(imd, wp, bd)
    assert y.shape == (B + 1, 27, 27, 64)
    assert torch.equal(y, ops.alex_stem(imd, wp, bd))
    x = kb.nchw(ops.preprocess_u8(imd, 224, 0).cpu()).double()
    ref, mag = kb.conv_ref(x, w, bias, 4, 2)
    r = torch.relu(ref)
    cb = kb.bound(r, mag, 363)
    y = kb.nchw(y.cpu())
    kb.assert_close_pooled(y, r, cb, f"alex_stem_rows B={B + 1}")
    # a seam: conv row 2 (the last of pooled row 0, the first of pooled row 1) loses its kh = 0 taps (image row 6)
    wrong = ref.clone()
    wrong[:, :, 2:3, :] -= torch.nn.functional.conv2d(x[:, :, 6:7, :], w[:, :, 0:1, :], None, (1, 4), (0, 2))
    for name, wr in (("seam taps", wrong), ("batch shift", kb.fault_batch_shift(ref))):
        kb.assert_rejects(y, kb.maxpool(torch.relu(wr)), kb.maxpool(cb), name)
    with pytest.raises(ValueError):
        ops.alex_stem_rows(imd[:, :220, :220].contiguous(), wp, bd)

"""pack_alex_stem_weight: the [64][ALEX_STEM_K] layout alex_stem.hip reads (the
engine builds the same layout in C++ when it packs features.0)."""
import torch

import dmlc
from dmlc import ops


def test_pack_alex_stem_weight_layout():
    C = dmlc.native()
    K = C.ALEX_STEM_K
    assert K == 544
    g = torch.Generator().manual_seed(11)
    # distinct non-zero bf16 values, so a misplaced or missing weight cannot hide
    w = (torch.randperm(64 * 363, generator=g).float().view(64, 3, 11, 11) % 251 + 1) / 256
    assert bool((w.bfloat16().float() == w).all()) and bool((w != 0).all())
    p = ops.pack_alex_stem_weight(w)
    assert p.shape == (64, K) and p.dtype == torch.bfloat16
    used = torch.zeros(K, dtype=torch.bool)
    for kh in range(11):
        for kw in range(11):
            for c in range(3):
                k = C.alex_stem_k(kh, kw, c)
                assert k == (kh * 6 + kw // 2) * 8 + (kw % 2) * 3 + c
                assert 0 <= k < K and not used[k]
                used[k] = True
                assert torch.equal(p[:, k].float(), w[:, c, kh, kw]), (kh, kw, c)
    assert int(used.sum()) == 363
    assert bool((p[:, ~used].float() == 0).all()) and int((~used).sum()) == K - 363


def test_pack_alex_stem_weight_scale_and_shape():
    w = torch.ones(64, 3, 11, 11)
    s = torch.arange(64).float()
    p = ops.pack_alex_stem_weight(w, scale=s)
    k = dmlc.native().alex_stem_k(10, 10, 2)
    assert torch.equal(p[:, k].float(), s)
    for bad in (torch.zeros(64, 3, 7, 7), torch.zeros(32, 3, 11, 11)):
        try:
            ops.pack_alex_stem_weight(bad)
        except ValueError:
            continue
        raise AssertionError("a wrong weight shape must raise")

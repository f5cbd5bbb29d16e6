"""resnet18_fp8 / resnet34_fp8 (layers 3-4 in e4m3, the 3x3 convs on
conv3x3_stream8's basic-block forms from B = 64 on a 256-CU device, on the
e4m3 implicit GEMM below) against fp32 torch on calibrated models.

The bar is the project's e4m3 rule (test_engine_gpu.py's _fp8_bar), from an
ideal e4m3 rounding of the same network (calibrated.e4m3_emulated_logits):
relative L2 <= max(6 %, 1.25 x the emulation's), top-1 agreement >= max(0.3,
the emulation's - 0.15). The emulation rounds every conv input after the
stem, the engine only layers 3-4, so the floor is conservative. B = 3 and 32
run the e4m3 implicit GEMMs; B = 64 (resnet18) the stream8 forms.
"""
import pytest
import torch

from dmlc.models import state_dict_f32
from dmlc.models.calibrated import calibrated, e4m3_emulated_logits, mixed_images, normalize
from dmlc.runtime import InferenceEngine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("arch,B", [("resnet18", 3), ("resnet18", 32), ("resnet18", 64), ("resnet34", 3),
                                    ("resnet34", 32)])
def test_engine_basic_block_fp8(gpu, arch, B):
    model = calibrated(arch, seed=11)
    sd = state_dict_f32(model)
    img = mixed_images(B, seed=12)
    with torch.no_grad():
        ref = model(normalize(img))
    emu = e4m3_emulated_logits(model, img)
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()
    floor, emu_agree = rel(emu, ref), (emu.argmax(-1) == ref.argmax(-1)).float().mean().item()
    bar, min_agree = max(6e-2, 1.25 * floor), max(0.3, emu_agree - 0.15)

    eng = InferenceEngine(arch + "_fp8", sd, max_batch=B)
    x = img.to(gpu)
    idx, prob, logits = eng.predict(x, return_logits=True, use_graph=False)
    torch.cuda.synchronize()
    got, agree = rel(logits.cpu(), ref), (idx.cpu().long() == ref.argmax(-1)).float().mean().item()
    print(f"{arch}_fp8 B={B}: rel {got:.4f} (emulation {floor:.4f}, bar {bar:.4f}), top-1 agreement {agree:.3f} "
          f"(emulation {emu_agree:.3f}, bar {min_agree:.3f})")
    assert torch.isfinite(logits).all()
    assert got <= bar and agree >= min_agree
    if B >= 32:
        assert ref.argmax(-1).unique().numel() >= 12
    # graph replay gives the same answer
    i2, _ = eng.predict(x, use_graph=True)
    assert torch.equal(i2.cpu(), idx.cpu())
    # embeddings: finite [B, 512], within the same bar of the bf16 engine's
    feat = eng.embed(x)
    base = InferenceEngine(arch, sd, max_batch=B).embed(x)
    torch.cuda.synchronize()
    frel = rel(feat.cpu(), base.cpu())
    print(f"{arch}_fp8 B={B}: features rel {frel:.4f} vs the bf16 engine")
    assert tuple(feat.shape) == (B, 512) and torch.isfinite(feat).all() and frel <= bar

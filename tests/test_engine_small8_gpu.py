"""The fp8 ResNets at query batches with EngineOptions::small_conv8 (every
e4m3 3x3 conv on conv_small8.hip) against fp32 torch on calibrated models under
the project's e4m3 rule (test_engine_resnet18_fp8_gpu.py), and against the
engine with default options: the two read the same codes and scales and differ
only in fp32 summation order, so they are closer to each other than to fp32.
"""
import pytest
import torch

from dmlc.models import state_dict_f32
from dmlc.models.calibrated import calibrated, e4m3_emulated_logits, mixed_images, normalize
from dmlc.runtime import InferenceEngine

pytestmark = pytest.mark.gpu

_models = {}


def _model(arch):
    if arch not in _models:
        m = calibrated(arch, seed=11)
        _models[arch] = (m, state_dict_f32(m))
    return _models[arch]


@pytest.mark.parametrize("arch,B", [("resnet18", 1), ("resnet18", 4), ("resnet34", 3), ("resnet50", 1),
                                    ("resnet50", 4)])
def test_engine_small8(gpu, arch, B):
    model, sd = _model(arch)
    img = mixed_images(B, seed=12)
    with torch.no_grad():
        ref = model(normalize(img))
    emu = e4m3_emulated_logits(model, img)
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()
    floor, emu_agree = rel(emu, ref), (emu.argmax(-1) == ref.argmax(-1)).float().mean().item()
    bar, min_agree = max(6e-2, 1.25 * floor), max(0.3, emu_agree - 0.15)

    x = img.to(gpu)
    on = InferenceEngine(arch + "_fp8", sd, max_batch=B, options={"small_conv8": True})
    off = InferenceEngine(arch + "_fp8", sd, max_batch=B)
    idx, _, logits = on.predict(x, return_logits=True, use_graph=False)
    _, _, base = off.predict(x, return_logits=True, use_graph=False)
    torch.cuda.synchronize()
    logits, base = logits.cpu(), base.cpu()
    got, agree = rel(logits, ref), (idx.cpu().long() == ref.argmax(-1)).float().mean().item()
    on_off, off_ref = rel(logits, base), rel(base, ref)
    print(f"{arch}_fp8 B={B} small_conv8: rel {got:.4f} vs fp32 (emulation {floor:.4f}, bar {bar:.4f}), off engine "
          f"{off_ref:.4f} vs fp32, on vs off {on_off:.2e}; top-1 agreement {agree:.3f} (emulation {emu_agree:.3f}, "
          f"bar {min_agree:.3f})")
    assert torch.isfinite(logits).all()
    assert got <= bar and agree >= min_agree
    assert on_off < off_ref
    # graph capture and replays give the eager answer
    for _ in range(3):
        i2, _ = on.predict(x, use_graph=True)
        assert torch.equal(i2.cpu(), idx.cpu())

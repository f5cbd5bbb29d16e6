"""ResNet50 at query batches with EngineOptions::small_1x1 (its 1x1 convs on
conv1x1_small.hip, layer1 unfused) on calibrated models against fp32 torch:
the bf16 model under test_engine_gpu.py's bar (3e-2 relative L2, as
test_engine_small_alex_gpu.py takes it), resnet50_fp8 (with small_conv8) under
test_engine_small8_gpu.py's emulation-derived bar and top-1 agreement rule.
The engine with the option off reads the same weights and scales and differs
in summation order (and in layer1's fused intermediates), so on and off are
closer to each other than off is to fp32.
"""
import pytest
import torch

from dmlc.models import state_dict_f32
from dmlc.models.calibrated import calibrated, e4m3_emulated_logits, mixed_images, normalize
from dmlc.runtime import InferenceEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    m = calibrated("resnet50", seed=11)
    return m, state_dict_f32(m)


@pytest.mark.parametrize("arch,B", [("resnet50", 1), ("resnet50", 4), ("resnet50_fp8", 1), ("resnet50_fp8", 4)])
def test_engine_small1x1(gpu, model, arch, B):
    m, sd = model
    fp8 = arch.endswith("_fp8")
    img = mixed_images(B, seed=12)
    with torch.no_grad():
        ref = m(normalize(img))
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()
    bar, min_agree = 3e-2, None
    if fp8:
        emu = e4m3_emulated_logits(m, img)
        floor, emu_agree = rel(emu, ref), (emu.argmax(-1) == ref.argmax(-1)).float().mean().item()
        bar, min_agree = max(6e-2, 1.25 * floor), max(0.3, emu_agree - 0.15)

    x = img.to(gpu)
    base_opts = {"small_conv8": True} if fp8 else {}
    on = InferenceEngine(arch, sd, max_batch=B, options={**base_opts, "small_1x1": True})
    off = InferenceEngine(arch, sd, max_batch=B, options=base_opts)
    kernels = [k for k, _, _, _ in on._e.plan(B, 224, 224)]
    assert kernels.count("Small1x1") >= 30 and not any(k.startswith("Bottleneck56") for k in kernels)
    idx, _, logits = on.predict(x, return_logits=True, use_graph=False)
    bidx, _, base = off.predict(x, return_logits=True, use_graph=False)
    torch.cuda.synchronize()
    logits, base, idx, bidx = logits.cpu(), base.cpu(), idx.cpu(), bidx.cpu()
    got, on_off, off_ref = rel(logits, ref), rel(logits, base), rel(base, ref)
    agree = (idx.long() == ref.argmax(-1)).float().mean().item()
    print(f"{arch} B={B} small_1x1: rel {got:.4f} vs fp32 (bar {bar:.4f}), off engine {off_ref:.4f} vs fp32, "
          f"on vs off {on_off:.2e}; top-1 agreement {agree:.3f}")
    assert torch.isfinite(logits).all() and got <= bar
    assert on_off < off_ref
    if fp8:
        assert agree >= min_agree
    else:  # test_engine_small_alex_gpu.py's rule: the clear top-1s agree with fp32 and with the default engine
        top2 = torch.softmax(ref, -1).topk(2, -1).values
        clear = (top2[:, 0] - top2[:, 1]) >= 1e-2
        assert torch.all(((idx == bidx) & (idx.long() == ref.argmax(-1))) | ~clear)
    for _ in range(3):  # graph capture and replays give the eager answer
        assert torch.equal(on.predict(x, use_graph=True)[0].cpu(), idx)

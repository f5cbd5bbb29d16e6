"""AlexNet at query batches with EngineOptions::small_alex on a calibrated model: under test_engine_gpu.py's
bf16 bar against fp32 torch (3e-2 relative L2), and closer to the default engine (same stem bits and bf16
products, another summation order) than to fp32; alexnet_fp8 under test_engine_alexnet_fp8_gpu.py's bar (b)."""
import pytest
import torch

from dmlc.models import state_dict_f32
from dmlc.models.calibrated import calibrated, mixed_images, normalize
from dmlc.runtime import InferenceEngine

from test_engine_alexnet_fp8_gpu import _act, _packed, _rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    m = calibrated("alexnet", seed=11)
    return m, state_dict_f32(m)


def _run(arch, sd, x, B, opts):
    eng = InferenceEngine(arch, sd, max_batch=B, options=opts)
    kernels = [k for k, _, _, _ in eng._e.plan(B, 224, 224)]
    assert kernels.count("SmallK") == (4 if opts else 0) and ("AlexStemRows" in kernels) == bool(opts)
    idx, _, logits = eng.predict(x, return_logits=True, use_graph=False)
    for _ in range(3):  # graph capture and replays give the eager answer
        assert torch.equal(eng.predict(x, use_graph=True)[0].cpu(), idx.cpu())
    return eng, idx.cpu(), logits.cpu()


@pytest.mark.parametrize("B", [1, 4])
def test_engine_small_alex(gpu, model, B):
    m, sd = model
    img = mixed_images(B, seed=40 + B)
    with torch.no_grad():
        ref = m(normalize(img))
    _, idx, logits = _run("alexnet", sd, img.to(gpu), B, {"small_alex": True})
    _, bidx, base = _run("alexnet", sd, img.to(gpu), B, {})
    got, off_ref, on_off = _rel(logits, ref), _rel(base, ref), _rel(logits, base)
    print(f"alexnet B={B} small_alex: rel L2 {got:.4f} vs fp32, off {off_ref:.4f} vs fp32, on vs off {on_off:.2e}")
    assert torch.isfinite(logits).all() and got < 3e-2 and on_off < off_ref
    top2 = torch.softmax(ref, -1).topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) >= 1e-2
    assert torch.all(((idx == bidx) & (idx.long() == ref.argmax(-1))) | ~clear)


def test_engine_small_alex_fp8(gpu, model):
    m, sd = model
    img = mixed_images(1, seed=45)
    with torch.no_grad():
        ref = m(normalize(img))
    eng, _, logits = _run("alexnet_fp8", sd, img.to(gpu), 1, {"small_alex": True})
    sx, s1 = (_act(eng, n, 1, torch.uint8, gpu)[1][1] for n in ("classifier.quant", "classifier.1"))
    q = lambda t, s: (t / s).clamp(-448, 448).to(torch.float8_e4m3fn).float() * s
    with torch.no_grad():
        f = torch.flatten(m.avgpool(m.features(normalize(img))), 1)
        e1 = torch.relu(q(f, sx) @ _packed(sd["classifier.1.weight"]).float().t() + sd["classifier.1.bias"])
        e4 = torch.relu(q(e1, s1) @ _packed(sd["classifier.4.weight"]).float().t() + sd["classifier.4.bias"])
        emu = e4 @ sd["classifier.6.weight"].t() + sd["classifier.6.bias"]
    floor, own, got = _rel(emu, ref), _rel(_run("alexnet", sd, img.to(gpu), 1, {})[2], ref), _rel(logits, ref)
    print(f"alexnet_fp8 B=1 small_alex vs fp32: rel L2 {got:.4f} (ideal e4m3 {floor:.4f} + bf16 engine {own:.4f})")
    assert torch.isfinite(logits).all() and got <= floor + own

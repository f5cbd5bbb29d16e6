"""alexnet_fp8 on a calibrated AlexNet: fc_small8 at B = 2, fc_gemm8 at B = 32.

(a) against options fc8 = False (the e4m3 implicit GEMM on the same codes).
Both stored classifier.1 outputs lie within `kb.e4m3_bound` of the float64
layer, so they differ by d1 <= 2 e4m3_bound; classifier.4's bf16 outputs then
by d4 <= |W4| d1 + 2 kb.bound, the logits by |W6| d4 + 2 kb.bound (fp32).
(b) against the fp32 model by relative L2: the bar is an ideal rounding of the
same e4m3 tensors in torch (the engine's scales) plus the bf16 engine's own
deviation. Measured on an MI355X (profiles/fc8.txt): B = 2: 0.1166 against
0.1192 + 0.0232; B = 32: 0.1194 against 0.1187 + 0.0243; the rolled control
1.37 / 1.39. In (a) the logits came out bit-equal at both batches.
(c) embed() returns the stored bf16 classifier.4 row, widened.
"""
import pytest
import torch

from dmlc import ops
from dmlc.models import state_dict_f32
from dmlc.models.calibrated import calibrated, mixed_images, normalize
from dmlc.runtime import InferenceEngine

import _kernel_bar as kb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    m = calibrated("alexnet", seed=11)
    return m, state_dict_f32(m)


def _act(eng, name, B, dtype, gpu):
    """The stored output activation of op `name` after an eager forward, [B, elems], and its (e4m3, scale)."""
    out = {n: o for n, _, o, _ in eng._e.op_list()}[name]
    H, W, C, _ = eng._e.activation_shape(out)
    t = torch.empty(B, H * W * C, dtype=dtype, device=gpu)
    eng._e.read_activation(out, B, t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return t.cpu(), eng._e.activation_quant(out)


def _packed(w):
    """The engine's e4m3 rows of a linear weight [N, K]: bf16-rounded, per-row scale amax / 448 -> dequantised float64."""
    q, s = ops.pack_conv_weight_fp8(w.bfloat16().float()[:, :, None, None])
    n = w.shape[0]
    return q[:n].double() * s[:n].double()[:, None]


_rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("B", [2, 32])
def test_alexnet_fp8(gpu, model, B):
    m, sd = model
    img = mixed_images(B, seed=30 + B)
    x = img.to(gpu)
    with torch.no_grad():
        ref = m(normalize(img))
    eng = InferenceEngine("alexnet_fp8", sd, max_batch=B)
    kernels = [k for k, _, _, _ in eng._e.plan(B, 224, 224)]
    assert ("FcSmall8" if B <= 16 else "FcGemm8") in kernels and "QuantE4m3" in kernels
    logits = eng.predict(x, return_logits=True, use_graph=False)[2].cpu()
    xq, (x8, sx) = _act(eng, "classifier.quant", B, torch.uint8, gpu)
    h1, (h8, s1) = _act(eng, "classifier.1", B, torch.uint8, gpu)
    h4, (h4_8, _) = _act(eng, "classifier.4", B, torch.bfloat16, gpu)
    assert x8 and h8 and not h4_8

    # ---- (a) the e4m3 implicit GEMM on the same codes
    base = InferenceEngine("alexnet_fp8", sd, max_batch=B, options={"fc8": False})
    assert "Igemm" in [k for k, _, _, _ in base._e.plan(B, 224, 224)]
    blogits = base.predict(x, return_logits=True, use_graph=False)[2].cpu()
    assert torch.equal(_act(base, "classifier.quant", B, torch.uint8, gpu)[0], xq)
    w1 = sd["classifier.1.weight"].view(4096, 256, 36).permute(0, 2, 1).reshape(4096, 9216)  # NHWC: k = hw C + c
    xd = xq.view(torch.float8_e4m3fn).double() * sx
    r1, mag1 = kb.fc_ref(xd, _packed(w1), sd["classifier.1.bias"])
    # (past the calibrated range both engines saturate at 448: the bar at the top of the range)
    d1 = 2 * kb.e4m3_bound(torch.relu(r1).clamp(max=447.0 * s1), mag1, 9216, kb.f32(1.0 / s1)) * s1
    w4 = _packed(sd["classifier.4.weight"])
    r4, mag4 = kb.fc_ref(h1.view(torch.float8_e4m3fn).double() * s1, w4, sd["classifier.4.bias"])
    d4 = d1 @ w4.abs().t() + 2 * kb.bound(torch.relu(r4), mag4, 4096)
    w6 = sd["classifier.6.weight"].bfloat16().double()
    r6, mag6 = kb.fc_ref(h4.double(), w6, sd["classifier.6.bias"])
    bar_a = d4 @ w6.abs().t() + 2 * kb.bound(r6, mag6, 4096, out_bf16=False)
    ratio, rel_a = kb.worst(logits, blogits, bar_a)
    print(f"alexnet_fp8 B={B} vs fc8=False: worst |diff|/bar {ratio:.3f}, rel L2 {rel_a:.2e}")
    assert ratio <= 1.0

    # ---- (b) the fp32 model: ideal e4m3 rounding of the same tensors + the bf16 engine's own deviation
    def q(t, s):
        return (t / s).clamp(-448, 448).to(torch.float8_e4m3fn).float() * s
    with torch.no_grad():
        f = torch.flatten(m.avgpool(m.features(normalize(img))), 1)
        e1 = torch.relu(q(f, sx) @ _packed(sd["classifier.1.weight"]).float().t() + sd["classifier.1.bias"])
        e4 = torch.relu(q(e1, s1) @ w4.float().t() + sd["classifier.4.bias"])
        emu = e4 @ sd["classifier.6.weight"].t() + sd["classifier.6.bias"]
    bf16 = InferenceEngine("alexnet", sd, max_batch=B)
    l16 = bf16.predict(x, return_logits=True, use_graph=False)[2].cpu()
    floor, own, got = _rel(emu, ref), _rel(l16, ref), _rel(logits, ref)
    print(f"alexnet_fp8 B={B} vs fp32: rel L2 {got:.4f} (ideal e4m3 {floor:.4f} + bf16 engine {own:.4f} = bar "
          f"{floor + own:.4f}), rolled {_rel(logits.roll(1, 0), ref):.3f}")
    assert torch.isfinite(logits).all() and got <= floor + own
    assert _rel(logits.roll(1, 0), ref) > floor + own  # the permuted-image control misses the bar
    for _ in range(3):  # graph replays give the eager answer
        assert torch.equal(eng.predict(x, use_graph=True)[0].cpu(), logits.argmax(-1).int())

    # ---- (c) embed(): the stored bf16 classifier.4 row, widened
    if B == 2:
        feat = eng.embed(x, use_graph=False)
        torch.cuda.synchronize()
        assert torch.equal(feat.cpu(), _act(eng, "classifier.4", B, torch.bfloat16, gpu)[0].float())

"""Float tensors as engine input: the pack kernel (csrc/kernels/pack_tensor.hip,
ops.pack_tensor) and the engine path (Engine::forward_tensor,
InferenceEngine.predict on a float tensor).

Op level: the reference is ops.stem_image / ops.paired_image of
x.permute(0,2,3,1).to(bfloat16), built on the CPU. Conversion (round to nearest
even) and placement are exact, so the comparison is torch.equal on the int16
views, into a buffer pre-filled with 0x7F7F so that padding left unwritten
shows.

Engine level: bit-equality with the u8 path on the tensor its preprocess
computes, and the whole-model bar of test_engine_gpu.py::
test_engine_matches_reference (relative L2 < 3e-2 against fp32 torch.nn) on
the very tensor the fp32 model reads.
"""
import numpy as np
import pytest
import torch

from dmlc import native, ops
from dmlc.models import state_dict_f32
from dmlc.models.calibrated import calibrated, mixed_images, noise_images, normalize
from dmlc.runtime import InferenceEngine

pytestmark = pytest.mark.gpu

BAR = 3e-2  # test_engine_gpu.py::test_engine_matches_reference
RTOL, ATOL = 1e-4, 1e-6  # test_topk_gpu.py
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
FILL = 0x7F7F

# common.h imagenet_norm: one fma with these float32 constants
SC = [np.float32(1) / (np.float32(255) * np.float32(s)) for s in (0.229, 0.224, 0.225)]
SH = [-np.float32(m) / np.float32(s) for m, s in ((0.485, 0.229), (0.456, 0.224), (0.406, 0.225))]


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _planted(dtype):
    """+-0, +-1, two values halfway between bf16 neighbours (1 + 2^-8 must go
    down to 1.0, 1 + 3 * 2^-8 up to 1.015625: ties to even), a large and a tiny
    normal value of the dtype."""
    big, tiny = (6e4, -1e-4) if dtype == torch.float16 else (1e30, -1e-30)
    return [0.0, -0.0, 1.0, -1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), big, tiny]


def _input(B, S, dtype, seed):
    """[B,3,S,S] of `dtype` on the CPU: randn * 3 with the planted values at both ends of the storage."""
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(seed)) * 3
    v = torch.tensor(_planted(dtype))
    flat = x.view(-1)
    flat[:len(v)] = v
    flat[-len(v):] = v
    x = x.to(dtype)
    assert torch.isfinite(x.float()).all()
    return x


def _reference(x, pad, Wr, paired):
    img = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    return ops.paired_image(img, pad, Wr // 2) if paired else ops.stem_image(img, pad, Wr)


def _pack_into_filled(xg, pad, Wr, paired):
    """The native launcher on a buffer pre-filled with 0x7F7F."""
    C = native()
    B, _, S, _ = xg.shape
    dt, cl = ops.tensor_input(xg)
    shape = (B, S + 2 * pad, Wr // 2, 8) if paired else (B, S + 2 * pad, Wr, 3)
    y = torch.full(shape, FILL, dtype=torch.int16, device=xg.device)
    C.pack_tensor(xg.data_ptr(), dt, cl, y.data_ptr(), B, S, pad, Wr, paired, torch.cuda.current_stream().cuda_stream)
    return y


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


# S = 12 and 20: the last 8-pixel group of a row straddles image and padding;
# S = 8: every group is a border group; 224: the engine's size, many workgroups
SHAPES = [(8, 3, 7, 2), (12, 3, 7, 2), (20, 2, 11, 4), (224, 3, 7, 2)]
OP_CASES = [(s, p, kw, st, paired) for s, p, kw, st in SHAPES for paired in ((False, True) if p == 3 else (False,))]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S,pad,KW,stride,paired", OP_CASES,
                         ids=[f"S{s}-p{p}-{'paired' if q else 'plain'}" for s, p, _, _, q in OP_CASES])
def test_pack_tensor_matches_reference(gpu, S, pad, KW, stride, paired, B):
    Wr = ops.stem_row_width(S, pad, KW, stride)
    # the reference's own conversion sends the planted ties to even
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)])
    assert ties.to(torch.bfloat16).tolist() == [1.0, 1.015625, -1.0]
    assert ties.half().to(torch.bfloat16).tolist() == [1.0, 1.015625, -1.0]
    for dtype in DTYPES:
        x = _input(B, S, dtype, seed=S * 10 + B)
        ref = _bits(_reference(x, pad, Wr, paired))
        for channels_last in (False, True):
            xg = x.to(gpu)
            if channels_last:
                xg = xg.contiguous(memory_format=torch.channels_last)
            what = (dtype, channels_last)
            assert ops.tensor_input(xg)[1] == (channels_last and S > 1), what
            y = _pack_into_filled(xg, pad, Wr, paired)
            z = ops.pack_tensor(xg, pad, Wr, paired)
            torch.cuda.synchronize()
            assert z.dtype == torch.bfloat16 and z.shape == y.shape, what
            got = _bits(y)
            assert torch.equal(got, ref), (what, (got != ref).sum().item())
            assert torch.equal(_bits(z), ref), what
            # every padding byte was written as zero, none kept the fill
            mask = _bits(_reference(torch.ones_like(x, dtype=torch.float32), pad, Wr, paired)) == 0
            assert (got[mask] == 0).all() and not (got == FILL).any(), what


def test_pack_tensor_default_row_width(gpu):
    x = _input(2, 12, torch.float32, seed=1)
    y = ops.pack_tensor(x.to(gpu), 3)
    torch.cuda.synchronize()
    assert y.shape == (2, 18, 24, 3)
    assert torch.equal(_bits(y), _bits(_reference(x, 3, 24, False)))


@pytest.mark.parametrize("paired", [False, True])
def test_pack_tensor_layout_is_detected(gpu, paired):
    """A tensor whose value names its own (b, c, y, x) lands identically as
    NCHW and as its channels_last copy: |v| = (c*8 + y)*8 + x <= 191 is exact
    in bf16 and the sign is b."""
    S, pad = 8, 3
    Wr = ops.stem_row_width(S, pad, 7, 2)
    v = torch.arange(3 * S * S, dtype=torch.float32).view(1, 3, S, S)
    x = torch.cat([v, -v])
    ref = _bits(_reference(x, pad, Wr, paired))
    xg = x.to(gpu)
    xl = xg.contiguous(memory_format=torch.channels_last)
    assert xl.stride() != xg.stride() and torch.equal(xl, xg)
    a = _pack_into_filled(xg, pad, Wr, paired)
    b = _pack_into_filled(xl, pad, Wr, paired)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), ref)
    assert torch.equal(_bits(b), ref)


def test_pack_tensor_argument_checks(gpu):
    x = torch.ones(2, 3, 12, 12, device=gpu)
    bad = [
        lambda: ops.pack_tensor(x.double(), 3),
        lambda: ops.pack_tensor(x[:, :, :, ::2], 3),  # a non-contiguous slice
        lambda: ops.pack_tensor(x[:, :, 2:10, 2:10], 3),
        lambda: ops.pack_tensor(torch.zeros(2, 4, 12, 12, device=gpu), 3),
        lambda: ops.pack_tensor(x[0], 3),
        lambda: ops.pack_tensor(x, 3, row_width=20),  # no multiple of 8
        lambda: ops.pack_tensor(x, 3, row_width=16),  # < S + 2 pad = 18
        lambda: ops.pack_tensor(x.cpu(), 3),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    # the native checks, past the Python ones: nothing is launched
    C = native()
    y = torch.zeros(2, 18, 24, 3, dtype=torch.bfloat16, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    F32 = C.TensorDType.F32
    for args in [(x.data_ptr(), F32, False, y.data_ptr(), 2, 12, 3, 20, False, s),
                 (x.data_ptr(), F32, False, y.data_ptr(), 2, 12, 3, 16, False, s),
                 (0, F32, False, y.data_ptr(), 2, 12, 3, 24, False, s),
                 (x.data_ptr(), F32, False, 0, 2, 12, 3, 24, False, s),
                 (x.data_ptr(), F32, False, y.data_ptr() + 2, 2, 12, 3, 24, False, s),
                 (x.data_ptr() + 2, F32, False, y.data_ptr(), 2, 12, 3, 24, False, s),
                 (x.data_ptr() + 1, C.TensorDType.F16, False, y.data_ptr(), 2, 12, 3, 24, False, s)]:
        with pytest.raises(ValueError):
            C.pack_tensor(*args)
    torch.cuda.synchronize()
    assert (y == 0).all()


def _imagenet_tensor(u8):
    """u8 [B,S,S,3] -> float32 [B,3,S,S] with preprocess_u8's bits: v * sc + sh
    is exact in fp64 (an 8-bit by a 24-bit factor, plus a 24-bit term within a
    few binades), so its float32 rounding is the kernel's single fma."""
    sc = torch.tensor([float(v) for v in SC], dtype=torch.float64)
    sh = torch.tensor([float(v) for v in SH], dtype=torch.float64)
    return (u8.double() * sc + sh).float().permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("paired", [False, True])
def test_imagenet_recipe_reproduces_preprocess_u8(gpu, paired):
    """All 256 x 3 (value, channel) pairs, and an image batch."""
    S, pad = 16, 3
    Wr = ops.stem_row_width(S, pad, 7, 2)
    u8 = torch.arange(256, dtype=torch.uint8).view(1, S, S, 1).expand(1, S, S, 3).contiguous()
    u8 = torch.cat([u8, noise_images(2, seed=3, size=S)])
    a = ops.preprocess_u8(u8.to(gpu), S, pad, Wr, paired)
    b = ops.pack_tensor(_imagenet_tensor(u8).to(gpu), pad, Wr, paired)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(arch):
        if arch not in cache:
            cache[arch] = calibrated(arch, seed=11)
        return cache[arch]
    return get


@pytest.fixture(scope="module")
def engines(models):
    cache = {}

    def get(arch, fused_preprocess=True):
        key = (arch, fused_preprocess)
        if key not in cache:
            opts = {} if fused_preprocess else {"fused_preprocess": False}
            cache[key] = InferenceEngine(arch, state_dict_f32(models(arch)), max_batch=8, options=opts)
        return cache[key]
    return get


def _fp32(model, x):
    with torch.no_grad():
        return model(x.float().cpu())


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("arch,B", [("resnet18", 3), ("resnet18", 1), ("alexnet", 3)])
def test_engine_tensor_bit_equal_to_u8(gpu, engines, arch, B, use_graph):
    """With the fused u8 stems off, u8 input goes Preprocess -> the stem and
    tensor input PackTensor -> the same stem: on the tensor preprocess_u8
    computes, the packed bytes are equal, so everything after them is."""
    eng = engines(arch, fused_preprocess=False)
    u8_plan = [k for k, _, _, _ in eng._e.plan(B, 224, 224)]
    t_plan = [k for k, _, _, _ in eng._e.plan(B, 224, 224, tensor_in=True)]
    assert u8_plan[0] == "Preprocess" and t_plan[0] == "PackTensor" and t_plan[1:] == u8_plan[1:]
    u8 = mixed_images(B, seed=70 + B)
    x = _imagenet_tensor(u8).to(gpu)
    ui, up, ul = eng.predict(u8.to(gpu), return_logits=True, use_graph=use_graph)
    ti, tp, tl = eng.predict(x, return_logits=True, use_graph=use_graph)
    torch.cuda.synchronize()
    assert tl.shape == (B, 1000) and ti.shape == (B,) and ti.dtype == torch.int32 and tp.dtype == torch.float32
    assert torch.equal(tl, ul), (tl - ul).abs().max().item()
    assert torch.equal(ti, ui) and torch.equal(tp, up)


@pytest.mark.parametrize("arch,variant", [("resnet18", "nchw"), ("alexnet", "nchw"), ("resnet18", "channels_last"),
                                          ("resnet18", "fp16"), ("resnet18", "images"), ("alexnet", "images")])
def test_engine_tensor_matches_fp32_on_the_same_tensor(gpu, engines, models, arch, variant):
    """randn mapped affinely onto the range of the calibrated images'
    normalised values (its min to theirs, its max to theirs), so every value is
    one an image can take; "images": the normalised images themselves.

    Measured on an MI355X (relative L2 against fp32, bar 3e-2): randn on the
    range 0.019 (AlexNet) / 0.008 (ResNet18); the images 0.026 / 0.015. White
    noise with the images' mean and std instead (a twentieth of its values
    outside their range) is past the bar on AlexNet for every bf16 forward:
    0.031 here, 0.030 for the u8 path on uniform-noise images, 0.033 for
    torch's own bf16 forward of the model (ResNet18: 0.016 / 0.015 / 0.022).
    That is AlexNet's bf16 floor on white noise, not the input path's error,
    which is none: tensor and u8 input agree bit for bit above."""
    cal = normalize(mixed_images(8, seed=12))
    if variant == "images":
        x = cal.contiguous()
    else:
        g = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(81))
        x = (g - g.min()) / (g.max() - g.min()) * (cal.max() - cal.min()) + cal.min()
    xg = x.to(gpu)
    if variant == "channels_last":
        xg = xg.contiguous(memory_format=torch.channels_last)
    elif variant == "fp16":
        xg = xg.half()
    ref = _fp32(models(arch), xg)  # fp16: the fp32 model on x.half().float()
    idx, prob, logits = engines(arch).predict(xg, return_logits=True)
    torch.cuda.synchronize()
    rel = _rel(logits.cpu(), ref)
    print(f"{arch} {variant}: rel {rel:.4f} (bar {BAR})")
    assert rel < BAR, rel
    assert torch.equal(idx.cpu().long(), logits.cpu().argmax(-1))


@pytest.mark.parametrize("arch", ["resnet18", "alexnet"])
def test_engine_honours_another_normalisation(gpu, engines, models, arch):
    u8 = mixed_images(8, seed=12)
    x2 = (u8.permute(0, 3, 1, 2).float() / 255 - 0.5) / 0.5
    _, _, logits = engines(arch).predict(x2.contiguous().to(gpu), return_logits=True)
    torch.cuda.synchronize()
    rel = _rel(logits.cpu(), _fp32(models(arch), x2))
    rel_imagenet = _rel(logits.cpu(), _fp32(models(arch), normalize(u8)))
    print(f"{arch}: rel {rel:.4f} against fp32 on mean/std 0.5, {rel_imagenet:.4f} on the ImageNet tensor (bar {BAR})")
    assert rel < BAR, rel
    assert rel_imagenet > BAR, rel_imagenet  # the engine did not normalise by itself


@pytest.mark.parametrize("arch", ["resnet18", "alexnet"])
def test_engine_tensor_graph_key(gpu, engines, arch):
    """One buffer, one pair of outputs, one batch size: u8 images, an fp32
    tensor and an fp16 tensor at the same address each replay their own graph.
    Expected: the eager forward of the same input from another buffer (idx
    equal; prob to rtol 1e-5, as test_topk_gpu compares two forwards)."""
    eng = engines(arch)
    B, S = 3, 224
    u8 = mixed_images(B, seed=90).to(gpu)
    x32 = normalize(mixed_images(B, seed=91)).contiguous().to(gpu)
    x16 = normalize(mixed_images(B, seed=92)).contiguous().to(gpu).half()
    want = {}
    for name, t in (("u8", u8), ("f32", x32), ("f16", x16)):
        i, p = eng.predict(t, use_graph=False)
        want[name] = (i.clone(), p.clone())
    torch.cuda.synchronize()
    assert len({tuple(i.tolist()) for i, _ in want.values()}) == 3  # the three inputs have different answers
    raw = torch.zeros(B * 3 * S * S * 4, dtype=torch.uint8, device=gpu)
    views = {"u8": raw[:B * S * S * 3].view(B, S, S, 3),
             "f32": raw.view(torch.float32).view(B, 3, S, S),
             "f16": raw.view(torch.float16)[:B * 3 * S * S].view(B, 3, S, S)}
    src = {"u8": u8, "f32": x32, "f16": x16}
    out = (torch.empty(B, dtype=torch.int32, device=gpu), torch.empty(B, dtype=torch.float32, device=gpu))
    for name in ("u8", "f32", "f16", "f32", "u8", "f16"):
        v = views[name]
        assert v.data_ptr() == raw.data_ptr()
        v.copy_(src[name])
        out[0].fill_(-1)
        idx, prob = eng.predict(v, out=out)
        torch.cuda.synchronize()
        assert torch.equal(idx, want[name][0]), name
        torch.testing.assert_close(prob, want[name][1], rtol=1e-5, atol=0)


def _topk_reference(logits, k):
    x = logits.detach().cpu()
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :k]
    return order, torch.softmax(x.double(), -1).gather(1, order)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("arch", ["alexnet", "resnet18"])
def test_engine_tensor_topk(gpu, engines, arch, use_graph):
    """Rank 0 is the topk = 1 answer: idx always; prob bit for bit where the
    tail is the softmax_top1 kernel (AlexNet: softmax_topk's contract), and to
    rtol 1e-5 after ResNet18's fused head, whose own softmax sums in another
    order (the bar test_topk_gpu.py::test_engine_topk sets for that tail)."""
    eng = engines(arch)
    B = 4
    assert [k for k, _, _, _ in eng._e.plan(B, 224, 224, topk=5, tensor_in=True)][-1] == "SoftmaxTopK"
    x = normalize(mixed_images(B, seed=95)).contiguous().to(gpu)
    idx, prob, logits = eng.predict(x, topk=5, return_logits=True, use_graph=use_graph)
    i1, p1 = eng.predict(x, use_graph=use_graph)
    torch.cuda.synchronize()
    assert idx.shape == (B, 5) and idx.dtype == torch.int32 and prob.shape == (B, 5) and prob.dtype == torch.float32
    ridx, rprob = _topk_reference(logits, 5)
    assert torch.equal(idx.cpu().long(), ridx)
    torch.testing.assert_close(prob.cpu().double(), rprob, rtol=RTOL, atol=ATOL)
    assert i1.shape == (B,) and torch.equal(idx[:, 0], i1)
    if arch == "alexnet":
        assert torch.equal(prob[:, 0], p1)
    else:
        torch.testing.assert_close(prob[:, 0], p1, rtol=1e-5, atol=0)


def test_engine_tensor_argument_checks(gpu, engines):
    eng = engines("alexnet")
    bad = [
        torch.zeros(2, 3, 200, 200, device=gpu),
        torch.zeros(2, 224, 224, 3, device=gpu),
        torch.zeros(2, 3, 224, 224, device=gpu, dtype=torch.float64),
        torch.zeros(2, 3, 224, 224),  # on the CPU
        torch.zeros(2, 3, 224, 448, device=gpu)[:, :, :, ::2],
        torch.zeros(3, 224, 224, device=gpu),
    ]
    for t in bad:
        with pytest.raises(ValueError):
            eng.predict(t)
    with pytest.raises(ValueError):
        eng.predict(torch.zeros(2, 3, 224, 224, device=gpu), topk=17)
    with pytest.raises(ValueError):  # the native check: more images than reserved
        eng.predict(torch.zeros(9, 3, 224, 224, device=gpu))
    torch.cuda.synchronize()

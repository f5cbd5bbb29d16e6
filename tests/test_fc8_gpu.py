"""fc8.hip (quant_e4m3, fc_small8, fc_gemm8) against float64 on the dequantised
codes (`kb.fc_ref`): only the fp32 accumulation, the alpha / bias step and the
output rounding separate the two. Bars: `kb.bound` (bf16 / fp32) and
`kb.e4m3_bound` (the out scale puts the largest value at 400 of 448). Control:
the reference without its last K block of 128 must miss the same bar.
Measured on an MI355X (profiles/fc8.txt), worst |err| / bar: fc_small8 0.90
(e4m3), 0.89 (bf16), 0.016 (fp32); fc_gemm8 0.93 (e4m3), 0.001 (fp32); the
weakest control 2.5.
"""
import pytest
import torch

from dmlc import native, ops

import _kernel_bar as kb

pytestmark = pytest.mark.gpu

_OPERANDS = {}

def _operands(M, K, N, npad):
    """Shared per shape (do not modify): e4m3 codes, alpha = s_x s_w, bias, dequantised x / w, (ref64, mag)."""
    key = (M, K, N, npad)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(800 + K % 89 + N)
        xv = torch.randn(M, K, generator=g)
        sx = kb.f32(float(xv.abs().max()) / kb.E4M3_MAX)
        x8 = ops.quantize_fp8(xv, sx)
        w8, sw = ops.pack_conv_weight_fp8((torch.randn(N, K, 1, 1, generator=g) / K ** 0.5))
        w8, sw = w8[:npad].contiguous(), sw[:npad].contiguous()
        bias = (torch.randn(N, generator=g) * 0.1).float()
        o = {"x8": x8, "w8": w8, "alpha": (sx * sw).float(), "bias": bias}
        o["x"], o["w"] = x8.double() * sx, w8[:N].double() * sw[:N].double()[:, None]
        o["ref"] = kb.fc_ref(o["x"], o["w"], bias)
        _OPERANDS[key] = o
    return _OPERANDS[key]


KINDS = ("e4m3", "bf16", "f32")  # e4m3 with ReLU

def _check(call, o, M, K, N, kind, shape, what, gpu):
    """call(out=, relu=, out_scale=, out_f32=) into a sentinel-filled tensor of `shape`; out[:M, :N] is judged."""
    ref, mag = o["ref"][0][:M], o["ref"][1][:M]
    relu = kind == "e4m3"
    r = torch.relu(ref) if relu else ref
    if kind == "e4m3":
        scale = float(torch.relu(o["ref"][0]).max()) / 400.0
        inv = kb.f32(1.0 / scale)
        out = torch.full(shape, 0x7F, dtype=torch.uint8, device=gpu)
        exp, bnd, l2, sentinel = r * inv, kb.e4m3_bound(r, mag, K, inv), kb.L2_E4M3, 0x7F
    else:
        scale, inv = None, 1.0
        out = torch.full(shape, 768.0, dtype=torch.float32 if kind == "f32" else torch.bfloat16, device=gpu)
        exp, bnd, l2, sentinel = r, kb.bound(r, mag, K, out_bf16=kind == "bf16"), kb.L2_BF16, 768.0
    y = call(out=out, relu=relu, out_scale=scale, out_f32=kind == "f32")
    assert tuple(y.shape) == (M, N)
    got = y.view(torch.float8_e4m3fn).float().cpu() if kind == "e4m3" else y.float().cpu()
    kb.assert_close(got, exp, bnd, what, l2=l2)
    whole = out.cpu().float()
    assert bool((whole[M:] == sentinel).all()) and bool((whole[:, N:] == sentinel).all()), "wrote outside [M, N]"
    short, _ = kb.fc_ref(o["x"][:M, :K - 128], o["w"][:, :K - 128], o["bias"])
    kb.assert_rejects(got, (torch.relu(short) if relu else short) * inv, bnd, what + ": last K block dropped")
    return y.clone()


# K 128: one step, 7 idle waves; 1152: 9 steps, an uneven split with empty waves; 9216: 9 a wave, past the unroll of 8
SMALL = [(B, K, N) for B in (1, 5, 16) for K in (128, 1152, 9216) for N in (16, 40)]


@pytest.mark.parametrize("B,K,N", SMALL)
def test_fc_small8(gpu, B, K, N):
    kind = KINDS[SMALL.index((B, K, N)) % 3]
    o = _operands(16, K, N, (N + 15) // 16 * 16)
    x8, w8, al, bi = o["x8"][:B].to(gpu), o["w8"].to(gpu), o["alpha"].to(gpu), o["bias"].to(gpu)
    call = lambda **kw: ops.fc_small8(x8, w8, N, al, bi, **kw)
    y = _check(call, o, B, K, N, kind, (B + 2, N + 8), f"fc_small8 B={B} K={K} N={N} {kind}", gpu)
    y2 = _check(call, o, B, K, N, kind, (B + 2, N + 8), "again", gpu)
    assert torch.equal(y.view(torch.uint8), y2.view(torch.uint8)), "a second call gives other bits"


# K 512: one slice of 4 blocks, the 3-slot ring wraps once; 9216: the rule's split, 3 (plain dealing), 8 (XCD dealing)
GEMM = [(M, N, K, s) for M in (1, 100, 256) for N in (128, 200) for K, s in ((512, 1), (9216, 0), (9216, 3), (9216, 8))]


@pytest.mark.parametrize("M,N,K,splits", GEMM)
def test_fc_gemm8(gpu, M, N, K, splits):
    kind = ("e4m3", "f32")[GEMM.index((M, N, K, splits)) % 2]
    o = _operands(256, K, N, kb.npad(N))
    x8, w8, al, bi = o["x8"][:M].to(gpu), o["w8"].to(gpu), o["alpha"].to(gpu), o["bias"].to(gpu)
    call = lambda **kw: ops.fc_gemm8(x8, w8, N, al, bi, splits=splits, **kw)
    _check(call, o, M, K, N, kind, (256, N), f"fc_gemm8 M={M} N={N} K={K} splits={splits} {kind}", gpu)


@pytest.mark.parametrize("scale", [0.25, 0.0371])
@pytest.mark.parametrize("B", [1, 7])
def test_quant_e4m3(gpu, B, scale):
    K = 9216
    x = torch.randn(B, K, generator=torch.Generator().manual_seed(B)).bfloat16()
    planted = torch.tensor([448.0, -448.0, 449.0, -1000.0, 0.0, 2.0 ** -7, -3 * 2.0 ** -9, 2.0 ** -10, 2.0 ** -11])
    x[-1, 5:5 + planted.numel()] = (planted * scale).bfloat16()
    got = ops.quant_e4m3(x.to(gpu), scale).cpu()
    # the kernel's rule: the product with fp32(1 / scale); a power-of-two scale makes it quantize_fp8(x, scale) itself
    want = ops.quantize_fp8(x.float() * torch.tensor(1.0 / scale, dtype=torch.float32), 1.0)
    if scale == 0.25:
        assert torch.equal(want.view(torch.uint8), ops.quantize_fp8(x, scale).view(torch.uint8))
    assert got.dtype == ops.FP8 and torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    assert got[-1, 5:9].float().tolist() == [448.0, -448.0, 448.0, -448.0]


def test_bad_shapes(gpu):
    z8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=gpu)
    f = torch.zeros(256, device=gpu)
    x, w, y = z8(2, 256), z8(16, 256), torch.zeros(2, 16, dtype=torch.bfloat16, device=gpu)
    st = torch.cuda.current_stream().cuda_stream
    raw = lambda wp, ldw: native().fc_small8(x.data_ptr(), 256, wp, ldw, f.data_ptr(), f.data_ptr(), y.data_ptr(), 16,
                                             False, False, 1.0, 2, 128, 16, 16, False, st)
    for bad in (lambda: ops.fc_small8(z8(17, 128), z8(16, 128), 16, f, f),   # more than 16 rows
                lambda: ops.fc_small8(z8(2, 192), z8(16, 192), 16, f, f),    # K not a multiple of 128
                lambda: ops.fc_gemm8(z8(2, 192), z8(128, 192), 128, f, f),
                lambda: ops.fc_gemm8(z8(257, 128), z8(128, 128), 128, f, f),  # more than 256 rows
                lambda: raw(w.data_ptr(), 136),                              # ldw not a multiple of 16
                lambda: raw(w.data_ptr() + 8, 256),                          # w not 16-B aligned
                lambda: ops.quant_e4m3(torch.zeros(2, 12, dtype=torch.bfloat16, device=gpu), 1.0)):
        with pytest.raises(ValueError):
            bad()

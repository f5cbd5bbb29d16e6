"""Op-level tests of the kernels that carry ResNet18's throughput and query
paths: conv3x3_rows, conv3x3_s2rows (with its 128-channel shape, ResNet50's
conv3x3_s2rows128), conv3x3_rows28, conv3x3_stream (stride 1,
stride 2 + fused downsample), conv_small, stem_pool (paired bf16 input, and the
u8 dense-K role-split form) and conv3x3_block.

As in test_kernels_fused_gpu.py each output is compared element-wise with a
float64 reference on the same bf16-rounded operands under the bar of
tests/_kernel_bar.py (derived from the arithmetic: threshold 1.0 everywhere),
keeps the project's relative-L2 bar, and carries negative controls: a
reference with one modelled kernel fault must be rejected. The direct convs
also get impulse tests with exact equality, at pixels picked from each
kernel's constants (ring wraps, strip seams, slot orders).

Forms that only the engine reached before: conv3x3_rows28 with the block's
downsample as 2 more K steps (`downsample=`, the DSX template) and with an
e4m3 output (`out_inv_scale=`, OUT8), and conv3x3_s2rows without its
downsample (the DS = false template).

Recorded on an MI355X (worst |err| / bar over a kernel's cases; its weakest
control ratio and which control), not thresholds:
  conv3x3_rows                 0.92   1132 (border taps)
  conv3x3_s2rows y             0.90   1174 (chunk swap); the conv alone 0.90, 1085
  conv3x3_s2rows yd            0.99   7168 (chunk swap)
  conv3x3_s2rows128            0.77    594 (border taps)
  conv3x3_s2rows128 e4m3       0.92    627 (chunk swap)
  conv3x3_rows28               0.83    408 (chunk swap)
  conv3x3_rows28 downsample=   0.80    233 (chunk swap)
  conv3x3_rows28 e4m3          0.92    212 (chunk swap)
  conv3x3_stream s1            0.93     44 (chunk swap)
  conv3x3_stream s2 y / yd     0.91 / 0.99   142 / 844 (chunk swap)
  conv_small y / yd            0.93 / 0.99   74 (border taps) / 1545
  stem_conv_pool               0.98    158 (chunk swap)
  stem_conv_pool_u8 dense K    0.98    477 (chunk swap)
  conv3x3_block                0.57     15 (conv1 chunk swap)
The 1x1 downsample outputs (K = 64 and up, no ReLU) and the stem (K = 147)
have almost no summation slack, so they sit closest to 1: the bar's rounding
term is bf16's first-order worst case. Largest relative L2 of a bf16 output
1.7e-3 (e4m3: 2.6e-2).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import dmlc
from dmlc import ops

import _kernel_bar as kb

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- operands and references (computed once, never modified)
@functools.lru_cache(maxsize=None)
def _operands(B, Cin, Cout, H, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, H, generator=g).bfloat16().double()
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).bfloat16().double()
    bias = (torch.randn(Cout, generator=g) * 0.1).float().double()
    return x, w, bias


@functools.lru_cache(maxsize=None)
def _residual(B, C, H, seed):
    return torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(seed)).bfloat16().double()


@functools.lru_cache(maxsize=None)
def _downsample_weights(Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    wd = (torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5).bfloat16().double()
    bd = (torch.randn(Cout, generator=g) * 0.1).float().double()
    return wd, bd


@functools.lru_cache(maxsize=None)
def _ref(B, Cin, Cout, H, stride, seed, res_seed=None):
    x, w, bias = _operands(B, Cin, Cout, H, 3, seed)
    res = None if res_seed is None else _residual(B, Cout, H // stride, res_seed)
    return kb.conv_ref(x, w, bias, stride, 1, res)


@functools.lru_cache(maxsize=None)
def _ref_ds(B, Cin, Cout, H, seed):
    x, _, _ = _operands(B, Cin, Cout, H, 3, seed)
    wd, bd = _downsample_weights(Cin, Cout, seed + 1000)
    return kb.conv_ref(x, wd, bd, 2, 0)


def _dev(x_nchw, gpu):
    return kb.nhwc(x_nchw).bfloat16().to(gpu)


def _pack(w, gpu):
    return ops.pack_conv_weight(w.float(), device=gpu)


def _check(y_nhwc, ref, mag, K, relu, controls, what):
    """y against relu?(ref) under kb.bound with the kernel's K; every control
    (a faulty ref before the ReLU) must be rejected."""
    act = torch.relu if relu else (lambda t: t)
    r = act(ref)
    bnd = kb.bound(r, mag, K)
    y = kb.nchw(y_nhwc.cpu())
    kb.assert_close(y, r, bnd, what)
    for name, wrong in controls:
        kb.assert_rejects(y, act(wrong), bnd, f"{what} [{name}]")


def _swap(ref, B):
    return kb.fault_chunk_swap(ref, b=B - 1, h=ref.shape[2] - 1, w=ref.shape[3] - 2, chunk=3)


def _controls_s1(ref, x, w, B, seam=None):
    out = [("border taps", kb.fault_border_taps(ref, x, w, 1)), ("chunk swap", _swap(ref, B))]
    if seam is not None:
        out.append(("seam taps", kb.fault_border_taps(ref, x, w, 1, at=seam)))
    if B > 1:
        out.append(("batch shift", kb.fault_batch_shift(ref)))
    return out


def _controls_s2(ref, x, w, B, col):
    out = [("border taps", kb.fault_border_taps_s2(ref, x, w)), ("chunk swap", _swap(ref, B)),
           ("strided parity", kb.fault_strided_parity(ref, x, w, col, 1))]
    if B > 1:
        out.append(("batch shift", kb.fault_batch_shift(ref)))
    return out


def _controls_ds(ref, x, wd, B, col):
    out = [("chunk swap", _swap(ref, B)), ("strided parity", kb.fault_strided_parity(ref, x, wd, col, 0))]
    if B > 1:
        out.append(("batch shift", kb.fault_batch_shift(ref)))
    return out


# ---------------------------------------------------------------- impulses
def _impulse_expected(w, pix, chans, Hin, Win, pad, stride=1):
    """[n, Cout, Ho, Wo] float64 for a k x k conv of stride `stride`: image i
    holds w[:, c_i, kh, kw] at the output pixel whose tap (kh, kw) lies on the
    input pixel pix_i = (row, col), zero elsewhere."""
    Cout, _, k, _ = w.shape
    Ho, Wo = (Hin + 2 * pad - k) // stride + 1, (Win + 2 * pad - k) // stride + 1
    out = torch.zeros(len(pix), Cout, Ho, Wo, dtype=torch.float64)
    for i, ((r, col), c) in enumerate(zip(pix, chans)):
        for kh in range(k):
            for kw in range(k):
                orow, ocol = r + pad - kh, col + pad - kw
                if orow % stride or ocol % stride:
                    continue
                orow, ocol = orow // stride, ocol // stride
                if 0 <= orow < Ho and 0 <= ocol < Wo:
                    out[i, :, orow, ocol] = w[:, c, kh, kw]
    return out


def _chans(Cin):
    """Channel 0, the last one, one in an interior 8-channel chunk, one in the
    last 32-channel K tile."""
    return [0, Cin - 1, 8 * 3 + 5, Cin - 32 + 9]


def _impulse_batches(pixels, chans, n=8):
    combos = [(p, c) for p in pixels for c in chans]
    return [combos[i:i + n] for i in range(0, len(combos), n)]


def _impulse_input(batch, Cin, H, W, gpu):
    x = torch.zeros(len(batch), H, W, Cin, dtype=torch.bfloat16)
    for i, ((r, col), c) in enumerate(batch):
        x[i, r, col, c] = 1.0
    return x.to(gpu)


def _equal(y_nhwc, want, what):
    got = kb.nchw(y_nhwc.cpu()).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} elements differ"


def _run_impulses(run, w, pixels, Cin, H, stride, gpu, what, wd=None):
    """run(x) -> y or (y, yd) with zero biases and no ReLU: every output is one
    bf16 weight or zero."""
    for batch in _impulse_batches(pixels, _chans(Cin)):
        pix, ch = [p for p, _ in batch], [c for _, c in batch]
        out = run(_impulse_input(batch, Cin, H, H, gpu))
        y, yd = out if isinstance(out, tuple) else (out, None)
        _equal(y, _impulse_expected(w, pix, ch, H, H, 1, stride), f"{what} {batch}")
        if wd is not None:
            _equal(yd, _impulse_expected(wd, pix, ch, H, H, 0, 2), f"{what} yd {batch}")


# ---------------------------------------------------------------- conv3x3_rows (layer1, 56x56x64)
ROWS_RING = kb.kernel_const("conv3x3_rows.hip", "RING")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("strip", [None, 4])
@pytest.mark.parametrize("use_res", [False, True])
def test_conv3x3_rows(gpu, B, strip, use_res):
    x, w, bias = _operands(B, 64, 64, 56, 3, 200 + B)
    ref, mag = _ref(B, 64, 64, 56, 1, 200 + B, 7 if use_res else None)
    rd = _dev(_residual(B, 64, 56, 7), gpu) if use_res else None
    xd, wp, bd = _dev(x, gpu), _pack(w, gpu), bias.float().to(gpu)
    y = ops.conv3x3_rows(xd, wp, bd, rd, True, strip)
    controls = _controls_s1(ref, x, w, B, seam=3) + [("ring row", kb.fault_ring_row(ref, x, w, ROWS_RING - 1, ROWS_RING))]
    _check(y, ref, mag, 576, True, controls, f"conv3x3_rows B={B} strip={strip} res={use_res}")
    # the register-weight variant: same MFMA order per output
    assert torch.equal(ops.conv3x3_rows(xd, wp, bd, rd, True, strip, frag=True), y)


@pytest.mark.parametrize("strip", [None, 4])
def test_conv3x3_rows_impulse(gpu, strip):
    # corners and edges; rows 4 | 7: a 4-row strip's first and last row; 9 | 10: the 10-row ring's wrap
    pixels = [(0, 0), (4, 55), (7, 30), (55, 55), (9, 0), (10, 17), (27, 28)]
    _, w, _ = _operands(1, 64, 64, 56, 3, 201)
    wp, zero = _pack(w, gpu), torch.zeros(64, device=gpu)
    for frag in (False, True):
        _run_impulses(lambda x: ops.conv3x3_rows(x, wp, zero, None, False, strip, frag=frag), w, pixels, 64, 56, 1, gpu,
                      f"conv3x3_rows strip={strip} frag={frag}")


# ---------------------------------------------------------------- conv3x3_s2rows (layer2.0 conv1 (+ downsample))
S2_RING = kb.kernel_const("conv3x3_s2rows.hip", "kRing")


@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_s2rows(gpu, B):
    """With the downsample (y: K = 576, yd: K = 64, no ReLU), and the conv
    alone (the DS = false template): its 18 K steps run the same MFMAs in the
    same order into the same accumulators, started from the same bias (the
    downsample's 2 K steps go to accumulators of their own), so its y is
    bit-equal to the downsample form's."""
    x, w, bias = _operands(B, 64, 128, 56, 3, 210 + B)
    wd, bd = _downsample_weights(64, 128, 1210 + B)
    ref, mag = _ref(B, 64, 128, 56, 2, 210 + B)
    refd, magd = _ref_ds(B, 64, 128, 56, 210 + B)
    xd, wp, wdp = _dev(x, gpu), _pack(w, gpu), _pack(wd, gpu)
    y, yd = ops.conv3x3_s2rows(xd, wp, bias.float().to(gpu), wdp, bd.float().to(gpu))
    ring_row = S2_RING // 2  # the first output row whose newest input row, 2 row + 1, is a ring length from row 0
    controls = _controls_s2(ref, x, w, B, col=13) + [("ring row", kb.fault_ring_row(ref, x, w, ring_row, S2_RING, 2))]
    _check(y, ref, mag, 576, True, controls, f"conv3x3_s2rows y B={B}")
    _check(yd, refd, magd, 64, False, _controls_ds(refd, x, wd, B, col=14), f"conv3x3_s2rows yd B={B}")
    alone = ops.conv3x3_s2rows(xd, wp, bias.float().to(gpu), None, None)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, y)
    _check(alone, ref, mag, 576, True, controls, f"conv3x3_s2rows alone B={B}")
    norelu = ops.conv3x3_s2rows(xd, wp, bias.float().to(gpu), None, None, relu=False)
    _check(norelu, ref, mag, 576, False, controls, f"conv3x3_s2rows alone relu=False B={B}")


def test_conv3x3_s2rows_impulse(gpu):
    # input rows at the 17-row ring's wrap (16 | 17, 33 | 34); columns 53, 55 (slots 27, 28: the last odd ones) and
    # 0, 2 (slots 29, 30: the first even ones); row and column 55
    pixels = [(16, 0), (17, 55), (33, 2), (34, 53), (55, 55), (0, 1), (28, 28), (55, 0)]
    _, w, _ = _operands(1, 64, 128, 56, 3, 211)
    wd, _ = _downsample_weights(64, 128, 1211)
    wp, wdp, zero = _pack(w, gpu), _pack(wd, gpu), torch.zeros(128, device=gpu)
    _run_impulses(lambda x: ops.conv3x3_s2rows(x, wp, zero, wdp, zero, relu=False), w, pixels, 64, 56, 2, gpu,
                  "conv3x3_s2rows", wd=wd)
    _run_impulses(lambda x: ops.conv3x3_s2rows(x, wp, zero, None, None, relu=False), w, pixels, 64, 56, 2, gpu,
                  "conv3x3_s2rows alone")


def test_conv3x3_s2rows_bad_args(gpu):
    x = torch.zeros(1, 56, 56, 64, dtype=torch.bfloat16, device=gpu)
    wp = torch.zeros(128, 576, dtype=torch.bfloat16, device=gpu)
    wdp = torch.zeros(128, 64, dtype=torch.bfloat16, device=gpu)
    b = torch.zeros(128, device=gpu)
    with pytest.raises(ValueError):
        ops.conv3x3_s2rows(x, wp, b, wdp, None)
    with pytest.raises(ValueError):
        ops.conv3x3_s2rows(x, wp, b, None, b)
    with pytest.raises(ValueError):
        ops.conv3x3_s2rows(x, wp, b, wdp[:, :32].contiguous(), b)
    C, P = dmlc.native(), ops._ptr
    wf, zero = ops.stream_weight_frag(wp), ops._zero_page(gpu)
    with pytest.raises(ValueError):  # in place
        C.conv3x3_s2rows(P(x), P(wf), P(b), 0, 0, P(x), 0, P(zero), 1, True, ops._stream())
    torch.cuda.synchronize()


# ---------------------------------------------------------------- conv3x3_s2rows128 (ResNet50 layer2.0 conv2)
S2_128_RING = kb.kernel_const("conv3x3_s2rows.hip", "kRing128")


def _controls_s2rows128(ref, x, w, B):
    ring_row = S2_128_RING // 2  # the first output row whose newest input row, 2 row + 1, is a ring length from row 0
    return _controls_s2(ref, x, w, B, col=13) + [("ring row", kb.fault_ring_row(ref, x, w, ring_row, S2_128_RING, 2))]


@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_s2rows128(gpu, B):
    """The 128-channel shape's bf16 output, K = 1152, with and without ReLU."""
    x, w, bias = _operands(B, 128, 128, 56, 3, 290 + B)
    ref, mag = _ref(B, 128, 128, 56, 2, 290 + B)
    xd, wp, bg = _dev(x, gpu), _pack(w, gpu), bias.float().to(gpu)
    controls = _controls_s2rows128(ref, x, w, B)
    for relu in (True, False):
        y = ops.conv3x3_s2rows128(xd, wp, bg, relu=relu)
        _check(y, ref, mag, 1152, relu, controls, f"conv3x3_s2rows128 B={B} relu={relu}")


def test_conv3x3_s2rows128_e4m3(gpu):
    """The OUT8 template: e4m3(relu(conv + b) inv_scale), nothing saturating,
    under conv3x3_rows28's e4m3 bar."""
    B = 2
    x, w, bias = _operands(B, 128, 128, 56, 3, 292)
    ref, mag = _ref(B, 128, 128, 56, 2, 292)
    r = torch.relu(ref)
    inv = 400.0 / r.max().item()
    y8 = ops.conv3x3_s2rows128(_dev(x, gpu), _pack(w, gpu), bias.float().to(gpu), out_inv_scale=inv)
    assert y8.dtype == torch.uint8 and y8.shape == (B, 28, 28, 128)
    y = kb.nchw(y8.view(torch.float8_e4m3fn).float().cpu())
    bnd = kb.e4m3_bound(r, mag, 1152, inv)
    what = "conv3x3_s2rows128 e4m3"
    kb.assert_close(y, r * inv, bnd, what, l2=4e-2)  # 2^-4 / sqrt(3) = 3.6e-2: e4m3's own rms roundoff at worst
    for name, wrong in _controls_s2rows128(ref, x, w, B):
        kb.assert_rejects(y, torch.relu(wrong) * inv, bnd, f"{what} [{name}]")


def test_conv3x3_s2rows128_impulse(gpu):
    # input rows at the 9-row ring's wrap (row yy in slot (yy + 1) % 9: 7 | 8 early, 43 | 44 and 52 | 53 late); columns
    # 53, 55 (slots 27, 28: the last odd ones) and 0, 2 (slots 29, 30: the first even ones); (11, 47): output rows 5, 6
    # x columns 23, 24, row 5 being the second row of its step, pixels 51, 52 of it: live lanes of the clamped 4th
    # fragment; (53, 55) reaches its last live lane (output (27, 27) too); row and column 55
    pixels = [(7, 0), (8, 55), (43, 2), (44, 53), (52, 20), (53, 55), (11, 47), (55, 55), (0, 1)]
    _, w, _ = _operands(1, 128, 128, 56, 3, 291)
    wp, zero = _pack(w, gpu), torch.zeros(128, device=gpu)
    _run_impulses(lambda x: ops.conv3x3_s2rows128(x, wp, zero, relu=False), w, pixels, 128, 56, 2, gpu,
                  "conv3x3_s2rows128")


def test_conv3x3_s2rows128_bad_args(gpu):
    x = torch.zeros(1, 56, 56, 128, dtype=torch.bfloat16, device=gpu)
    wp = torch.zeros(128, 1152, dtype=torch.bfloat16, device=gpu)
    b = torch.zeros(128, device=gpu)
    with pytest.raises(ValueError):  # the 64-channel shape's input
        ops.conv3x3_s2rows128(x[..., :64].contiguous(), wp, b)
    with pytest.raises(ValueError):  # wrong weights
        ops.conv3x3_s2rows128(x, wp[:, :576].contiguous(), b)
    C, P = dmlc.native(), ops._ptr
    wf = ops.stream_weight_frag(wp)
    y = torch.empty(1, 28, 28, 128, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError):  # in place
        C.conv3x3_s2rows128(P(x), P(wf), P(b), P(x), 1, True, 0.0, ops._stream())
    with pytest.raises(ValueError):  # misaligned
        C.conv3x3_s2rows128(P(x) + 2, P(wf), P(b), P(y), 1, True, 0.0, ops._stream())
    with pytest.raises(ValueError):
        C.conv3x3_s2rows128(P(x), P(wf), P(b), P(y) + 8, 1, True, 0.0, ops._stream())
    with pytest.raises(ValueError):  # null
        C.conv3x3_s2rows128(P(x), 0, P(b), P(y), 1, True, 0.0, ops._stream())
    with pytest.raises(ValueError):  # a batch whose element count overflows int
        C.conv3x3_s2rows128(P(x), P(wf), P(b), P(y), 5350, True, 0.0, ops._stream())
    torch.cuda.synchronize()


# ---------------------------------------------------------------- conv3x3_rows28 (layer2's stride-1 convs)
R28_RING = kb.kernel_const("conv3x3_rows28.hip", "kRing")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("use_res", [False, True])
def test_conv3x3_rows28(gpu, B, use_res):
    x, w, bias = _operands(B, 128, 128, 28, 3, 220 + B)
    ref, mag = _ref(B, 128, 128, 28, 1, 220 + B, 8 if use_res else None)
    rd = _dev(_residual(B, 128, 28, 8), gpu) if use_res else None
    y = ops.conv3x3_rows28(_dev(x, gpu), _pack(w, gpu), bias.float().to(gpu), rd, True)
    controls = _controls_s1(ref, x, w, B, seam=3) + [("ring row", kb.fault_ring_row(ref, x, w, R28_RING - 1, R28_RING))]
    _check(y, ref, mag, 1152, True, controls, f"conv3x3_rows28 B={B} res={use_res}")


@functools.lru_cache(maxsize=None)
def _rows28_ds_case(B):
    x, w, bias = _operands(B, 128, 128, 28, 3, 220 + B)
    x56, _, _ = _operands(B, 64, 128, 56, 3, 210 + B)
    wd, bd = _downsample_weights(64, 128, 1220 + B)
    c, cm = _ref(B, 128, 128, 28, 1, 220 + B)
    d, dm = kb.conv_ref(x56, wd, bd, 2, 0)
    return x, w, bias, x56, wd, bd, c + d, cm + dm  # one float64 sum, the downsample not rounded


@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_rows28_downsample(gpu, B):
    """The DSX template: relu(conv3x3(x) + b + conv1x1_s2(x56) + bd), K = 1152 + 64."""
    x, w, bias, x56, wd, bd, ref, mag = _rows28_ds_case(B)
    y = ops.conv3x3_rows28(_dev(x, gpu), _pack(w, gpu), bias.float().to(gpu), None, True,
                           downsample=(_dev(x56, gpu), _pack(wd, gpu), bd.float().to(gpu)))
    controls = _controls_s1(ref, x, w, B) + [
        ("ring row", kb.fault_ring_row(ref, x, w, R28_RING - 1, R28_RING)),
        ("ds missing", kb.fault_ds_missing(ref, x56, wd, b=B - 1, frag=48)),  # the last fragment of an image
        ("ds missing, step 1", kb.fault_ds_missing(ref, x56, wd, b=0, frag=7)),  # the second buffer's first fragment
        ("ds strided parity", kb.fault_strided_parity(ref, x56, wd, 27, 0))]
    _check(y, ref, mag, 1216, True, controls, f"conv3x3_rows28 downsample B={B}")


def test_conv3x3_rows28_e4m3(gpu):
    """The OUT8 template: e4m3(relu(conv + b) inv_scale), nothing saturating."""
    B = 2
    x, w, bias = _operands(B, 128, 128, 28, 3, 222)
    ref, mag = _ref(B, 128, 128, 28, 1, 222)
    r = torch.relu(ref)
    inv = 400.0 / r.max().item()
    y8 = ops.conv3x3_rows28(_dev(x, gpu), _pack(w, gpu), bias.float().to(gpu), None, True, out_inv_scale=inv)
    assert y8.dtype == torch.uint8 and y8.shape == (B, 28, 28, 128)
    y = kb.nchw(y8.view(torch.float8_e4m3fn).float().cpu())
    bnd = kb.e4m3_bound(r, mag, 1152, inv)
    what = "conv3x3_rows28 e4m3"
    kb.assert_close(y, r * inv, bnd, what, l2=4e-2)  # 2^-4 / sqrt(3) = 3.6e-2: e4m3's own rms roundoff at worst
    for name, wrong in _controls_s1(ref, x, w, B, seam=3) + [
            ("ring row", kb.fault_ring_row(ref, x, w, R28_RING - 1, R28_RING))]:
        kb.assert_rejects(y, torch.relu(wrong) * inv, bnd, f"{what} [{name}]")


def test_conv3x3_rows28_impulse(gpu):
    # rows 3 | 4: a 4-row step; 9 | 10 and 19 | 20: the 10-row ring's wrap; row 27
    pixels = [(3, 0), (4, 27), (9, 13), (10, 14), (19, 5), (20, 22), (27, 27), (0, 0), (27, 0)]
    _, w, _ = _operands(1, 128, 128, 28, 3, 221)
    wd, _ = _downsample_weights(64, 128, 1221)
    wp, wdp, zero = _pack(w, gpu), _pack(wd, gpu), torch.zeros(128, device=gpu)
    _run_impulses(lambda x: ops.conv3x3_rows28(x, wp, zero, None, False), w, pixels, 128, 28, 1, gpu, "conv3x3_rows28")

    def with_ds(x):
        x56 = torch.zeros(x.shape[0], 56, 56, 64, dtype=torch.bfloat16, device=gpu)
        return ops.conv3x3_rows28(x, wp, zero, None, False, downsample=(x56, wdp, zero))

    _run_impulses(with_ds, w, pixels, 128, 28, 1, gpu, "conv3x3_rows28 downsample, zero x56")
    # an impulse in x56: at an even / even pixel the wd column, at an odd row or column nothing
    pix56 = [(0, 0), (6, 8), (8, 54), (18, 20), (54, 54), (40, 2), (7, 8), (8, 7), (55, 55), (1, 1), (54, 55)]
    for batch in _impulse_batches(pix56, _chans(64)):
        x56 = _impulse_input(batch, 64, 56, 56, gpu)
        x = torch.zeros(len(batch), 28, 28, 128, dtype=torch.bfloat16, device=gpu)
        y = ops.conv3x3_rows28(x, wp, zero, None, False, downsample=(x56, wdp, zero))
        want = _impulse_expected(wd, [p for p, _ in batch], [c for _, c in batch], 56, 56, 0, 2)
        for i, ((r, c), _) in enumerate(batch):
            assert bool(want[i].any()) == (r % 2 == 0 and c % 2 == 0)
        _equal(y, want, f"conv3x3_rows28 x56 impulse {batch}")


def test_conv3x3_rows28_bad_args(gpu):
    x = torch.zeros(1, 28, 28, 128, dtype=torch.bfloat16, device=gpu)
    x56 = torch.zeros(1, 56, 56, 64, dtype=torch.bfloat16, device=gpu)
    wp = torch.zeros(128, 1152, dtype=torch.bfloat16, device=gpu)
    wdp = torch.zeros(128, 64, dtype=torch.bfloat16, device=gpu)
    b = torch.zeros(128, device=gpu)
    with pytest.raises(ValueError):  # a residual together with the downsample
        ops.conv3x3_rows28(x, wp, b, x, True, downsample=(x56, wdp, b))
    with pytest.raises(ValueError):  # a wrong x56 shape
        ops.conv3x3_rows28(x, wp, b, None, True, downsample=(x56[:, :28].contiguous(), wdp, b))
    with pytest.raises(ValueError):
        ops.conv3x3_rows28(x, wp, b, None, True, downsample=(torch.zeros(2, 56, 56, 64, dtype=torch.bfloat16, device=gpu), wdp, b))
    with pytest.raises(ValueError):  # wrong downsample weights
        ops.conv3x3_rows28(x, wp, b, None, True, downsample=(x56, wp, b))
    with pytest.raises(ValueError):  # an e4m3 output with a residual
        ops.conv3x3_rows28(x, wp, b, x, True, out_inv_scale=1.0)
    with pytest.raises(ValueError):  # ... or with the downsample
        ops.conv3x3_rows28(x, wp, b, None, True, downsample=(x56, wdp, b), out_inv_scale=1.0)


# ---------------------------------------------------------------- conv3x3_stream
# seam: the row above the second workgroup of an image (half images of 28 rows, 8-row strips of 56)
@pytest.mark.parametrize("HW,C,seam", [(28, 128, 13), (14, 256, None), (7, 512, None), (56, 64, 7)])
@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_stream(gpu, HW, C, seam, B):
    x, w, bias = _operands(B, C, C, HW, 3, 230 + B + HW)
    xd, wp, bd = _dev(x, gpu), _pack(w, gpu), bias.float().to(gpu)
    frag = dmlc.native().conv3x3_stream_uses_frag(HW, HW, C, C, 1)
    for use_res in (False, True):
        ref, mag = _ref(B, C, C, HW, 1, 230 + B + HW, 9 if use_res else None)
        rd = _dev(_residual(B, C, HW, 9), gpu) if use_res else None
        controls = _controls_s1(ref, x, w, B, seam)
        for relu in (False, True):
            y = ops.conv3x3_stream(xd, wp, bd, rd, relu)
            _check(y, ref, mag, 9 * C, relu, controls, f"conv3x3_stream {HW}x{HW}x{C} B={B} res={use_res} relu={relu}")
            if frag:  # the register-weight variant: same MFMA order per output
                assert torch.equal(ops.conv3x3_stream(xd, wp, bd, rd, relu, frag=True), y)


@pytest.mark.parametrize("HW,Cin,col", [(56, 64, 13), (28, 128, 7), (14, 256, 6)])
@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_stream_stride2_downsample(gpu, HW, Cin, col, B):
    Cout = 2 * Cin
    x, w, bias = _operands(B, Cin, Cout, HW, 3, 240 + B + HW)
    wd, bd = _downsample_weights(Cin, Cout, 1240 + B + HW)
    ref, mag = _ref(B, Cin, Cout, HW, 2, 240 + B + HW)
    refd, magd = _ref_ds(B, Cin, Cout, HW, 240 + B + HW)
    xd, wp, wdp = _dev(x, gpu), _pack(w, gpu), _pack(wd, gpu)
    bg, bdg = bias.float().to(gpu), bd.float().to(gpu)
    y, yd = ops.conv3x3_stream(xd, wp, bg, None, True, stride=2, downsample=(wdp, bdg))
    what = f"conv3x3_stream s2 {HW}x{HW}x{Cin}"
    _check(y, ref, mag, 9 * Cin, True, _controls_s2(ref, x, w, B, col), f"{what} y B={B}")
    _check(yd, refd, magd, Cin, False, _controls_ds(refd, x, wd, B, col - 1), f"{what} yd B={B}")
    if dmlc.native().conv3x3_stream_uses_frag(HW, HW, Cin, Cout, 2):
        y2, yd2 = ops.conv3x3_stream(xd, wp, bg, None, True, stride=2, downsample=(wdp, bdg), frag=True)
        assert torch.equal(y2, y) and torch.equal(yd2, yd)


@pytest.mark.parametrize("HW,C,pixels", [
    (28, 128, [(13, 0), (14, 27), (0, 0), (27, 27), (13, 14), (14, 13)]),  # rows 13 | 14: the half-image seam
    (14, 256, [(0, 0), (13, 13), (6, 7), (7, 0)]),
    (7, 512, [(0, 0), (6, 6), (3, 3), (0, 6)]),
    (56, 64, [(7, 0), (8, 55), (47, 30), (48, 31), (0, 55), (55, 0)])])  # rows 7 | 8, 47 | 48: strip seams
def test_conv3x3_stream_impulse(gpu, HW, C, pixels):
    _, w, _ = _operands(1, C, C, HW, 3, 231)
    wp, zero = _pack(w, gpu), torch.zeros(C, device=gpu)
    _run_impulses(lambda x: ops.conv3x3_stream(x, wp, zero, None, False), w, pixels, C, HW, 1, gpu,
                  f"conv3x3_stream {HW}x{HW}x{C}")
    if dmlc.native().conv3x3_stream_uses_frag(HW, HW, C, C, 1):
        _run_impulses(lambda x: ops.conv3x3_stream(x, wp, zero, None, False, frag=True), w, pixels, C, HW, 1, gpu,
                      f"conv3x3_stream {HW}x{HW}x{C} frag")


@pytest.mark.parametrize("HW,Cin,pixels", [
    # quarter images: output rows 6 | 7, 13 | 14, 20 | 21 meet on input rows 13, 27, 41
    (56, 64, [(12, 0), (13, 55), (14, 2), (27, 28), (28, 29), (41, 54), (42, 1), (55, 55), (0, 0)]),
    (28, 128, [(12, 0), (13, 27), (14, 14), (27, 27), (0, 1), (15, 26)]),  # half images: input row 13
    (14, 256, [(0, 0), (13, 13), (6, 7), (7, 6), (13, 0)])])
def test_conv3x3_stream_stride2_impulse(gpu, HW, Cin, pixels):
    Cout = 2 * Cin
    _, w, _ = _operands(1, Cin, Cout, HW, 3, 241)
    wd, _ = _downsample_weights(Cin, Cout, 1241)
    wp, wdp, zero = _pack(w, gpu), _pack(wd, gpu), torch.zeros(Cout, device=gpu)
    _run_impulses(lambda x: ops.conv3x3_stream(x, wp, zero, None, False, stride=2, downsample=(wdp, zero)), w, pixels,
                  Cin, HW, 2, gpu, f"conv3x3_stream s2 {HW}x{HW}x{Cin}", wd=wd)


# ---------------------------------------------------------------- conv_small (the query path)
SMALL_SHAPES = [(56, 64, 64, 1), (56, 64, 128, 2), (28, 128, 128, 1), (28, 128, 256, 2), (14, 256, 256, 1),
                (14, 256, 512, 2), (7, 512, 512, 1)]


@pytest.mark.parametrize("HW,Cin,Cout,stride", SMALL_SHAPES)
@pytest.mark.parametrize("B,mf", [(1, 1), (1, 4), (3, None)])
def test_conv_small(gpu, HW, Cin, Cout, stride, B, mf):
    """Stride 1 with a residual, stride 2 with the fused downsample. The four
    waves' partial sums meet in LDS: a summation in another order, inside the
    bar's K 2^-23 mag as it stands."""
    seed = 250 + B + HW
    x, w, bias = _operands(B, Cin, Cout, HW, 3, seed)
    xd, wp, bg = _dev(x, gpu), _pack(w, gpu), bias.float().to(gpu)
    what = f"conv_small {HW}x{HW}x{Cin}->{Cout} s{stride} B={B} mf={mf}"
    if stride == 1:
        ref, mag = _ref(B, Cin, Cout, HW, 1, seed, 10)
        y = ops.conv_small(xd, wp, bg, _dev(_residual(B, Cout, HW, 10), gpu), True, mf=mf)
        _check(y, ref, mag, 9 * Cin, True, _controls_s1(ref, x, w, B), what)
    else:
        wd, bd = _downsample_weights(Cin, Cout, 1000 + seed)
        ref, mag = _ref(B, Cin, Cout, HW, 2, seed)
        refd, magd = _ref_ds(B, Cin, Cout, HW, seed)
        y, yd = ops.conv_small(xd, wp, bg, None, True, stride=2, wd_packed=_pack(wd, gpu), bd=bd.float().to(gpu), mf=mf)
        _check(y, ref, mag, 9 * Cin, True, _controls_s2(ref, x, w, B, HW // 4), what + " y")
        _check(yd, refd, magd, Cin, False, _controls_ds(refd, x, wd, B, HW // 4 - 1), what + " yd")


@pytest.mark.parametrize("HW,Cin,Cout,stride", SMALL_SHAPES)
def test_conv_small_impulse(gpu, HW, Cin, Cout, stride):
    _, w, _ = _operands(1, Cin, Cout, HW, 3, 251)
    wd = _downsample_weights(Cin, Cout, 1251)[0] if stride == 2 else None
    wp, zero = _pack(w, gpu), torch.zeros(Cout, device=gpu)
    wdp = _pack(wd, gpu) if stride == 2 else None
    Wo = HW // stride if stride == 2 else HW
    P = Wo * Wo
    for mf in (1, 2, 4):
        # output pixels: the last of a 16-pixel fragment and the first of the next, the same for an mf-fragment
        # tile, the image's last pixel (the tail of a partial tile)
        outs = sorted({p for p in (15, 16, 16 * mf - 1, 16 * mf, P - 1) if p < P})
        pixels = [(stride * (p // Wo), stride * (p % Wo)) for p in outs]
        if stride == 1:
            run = lambda x: ops.conv_small(x, wp, zero, None, False, mf=mf)
        else:
            pixels.append((HW - 1, HW - 1))  # an odd / odd pixel: the downsample sees nothing
            run = lambda x: ops.conv_small(x, wp, zero, None, False, stride=2, wd_packed=wdp, bd=zero, mf=mf)
        _run_impulses(run, w, pixels, Cin, HW, stride, gpu, f"conv_small {HW}x{HW}x{Cin} s{stride} mf={mf}", wd=wd)


# ---------------------------------------------------------------- the fused stem (conv7x7/s2/p3 + ReLU + maxpool3x3/s2/p1)
def _stem_weights(seed):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5).bfloat16().double()
    bias = (torch.randn(64, generator=g) * 0.1).float().double()
    return w, bias


def _stem_controls(ref, x, w, b):
    # conv row 1 (image rows -1 .. 5) loses its kh = 1 taps, the ones on image row 0
    lost = F.conv2d(x[:, :, 0:1, :], w[:, :, 1:2, :], None, (1, 2), (0, 3))
    wrong = ref.clone()
    wrong[:, :, 1:2, :] -= lost
    return [("border taps", wrong), ("chunk swap", kb.fault_chunk_swap_at_max(ref, b=b, chunk=5)),
            ("batch shift", kb.fault_batch_shift(ref))]


def _check_stem(y, x, w, bias, K, what, b):
    ref, mag = kb.conv_ref(x, w, bias, 2, 3)
    r = torch.relu(ref)
    cb = kb.bound(r, mag, K)
    y = kb.nchw(y.cpu())
    kb.assert_close_pooled(y, r, cb, what, pad=1)
    for name, wrong in _stem_controls(ref, x, w, b):
        kb.assert_rejects(y, kb.maxpool(torch.relu(wrong), pad=1), kb.maxpool(cb, pad=1), f"{what} [{name}]")


@pytest.mark.parametrize("S", [224, 128])
@pytest.mark.parametrize("B,strip", [(3, None), (2, 2), (1, 56)], ids=["B3", "B2-strip2", "B1-whole"])
def test_stem_conv_pool(gpu, S, B, strip):
    """The paired-bf16-input stem, K = 147; strip 56 stands for one workgroup
    per image (S / 4 pooled rows). One more image is 0 inside and large on its
    outer 3 rows and columns: the padding taps dominate the border outputs."""
    if strip == 56:
        strip = S // 4
    g = torch.Generator().manual_seed(260 + B + S)
    x = torch.randn(B + 1, 3, S, S, generator=g).bfloat16().double()
    x[B] = 2.5
    x[B, :, 3:-3, 3:-3] = 0
    w, bias = _stem_weights(261)
    xp = ops.paired_image(kb.nhwc(x).float(), 3).bfloat16().to(gpu)
    y = ops.stem_conv_pool(xp, ops.pack_stem_pool_weight(w.float(), device=gpu), bias.float().to(gpu), S, strip)
    assert y.shape == (B + 1, S // 4, S // 4, 64)
    _check_stem(y, x, w, bias, 147, f"stem_conv_pool S={S} B={B + 1} strip={strip}", B - 1)


@pytest.mark.parametrize("B", [1, 3])
def test_stem_conv_pool_u8_dense(gpu, B):
    """The u8 one-image-per-workgroup stem with dense K (K = 7 windows of 22 =
    154 products, 7 of them on zero weights) on the values preprocess_u8 gives."""
    g = torch.Generator().manual_seed(270 + B)
    img = torch.randint(0, 256, (B + 1, 224, 224, 3), generator=g, dtype=torch.uint8).to(gpu)
    w, bias = _stem_weights(271)
    x = kb.nchw(ops.preprocess_u8(img, 224, 0).cpu()).double()
    assert x.shape == (B + 1, 3, 224, 224)
    wp = ops.pack_stem_pool_weight(w.float(), device=gpu)
    wdn = ops.pack_stem_dense_weight(w.float(), device=gpu)
    C = dmlc.native()
    C.stem_conv_pool_set_dbg(512)
    try:
        y = ops.stem_conv_pool_u8(img, wp, bias.float().to(gpu), None, w_dense=wdn)
        torch.cuda.synchronize()
    finally:
        C.stem_conv_pool_set_dbg(0)
    _check_stem(y, x, w, bias, 154, f"stem_conv_pool_u8 dense B={B + 1}", B)


@pytest.mark.parametrize("S,strip", [(224, 2), (224, None), (128, None)])
def test_stem_conv_pool_impulse(gpu, S, strip):
    # image rows / columns 0, 1, 2 (inside the 3-pixel padding reach) and S - 1; rows 7 | 8: conv rows 3 | 4 | 5,
    # the seam of 2-pooled-row strips; an odd and an even column of a pixel pair
    pixels = [(0, 0), (1, 2), (2, 1), (S - 1, S - 1), (7, 8), (8, 7), (0, S - 1), (S - 1, 0), (S // 2 + 1, S // 2)]
    w, _ = _stem_weights(262)
    wp, zero = ops.pack_stem_pool_weight(w.float(), device=gpu), torch.zeros(64, device=gpu)
    for batch in _impulse_batches(pixels, [0, 1, 2], n=9):  # each of r, g, b
        x = torch.zeros(len(batch), S, S, 3)
        for i, ((r, col), c) in enumerate(batch):
            x[i, r, col, c] = 1.0
        y = ops.stem_conv_pool(ops.paired_image(x, 3).bfloat16().to(gpu), wp, zero, S, strip)
        want = _impulse_expected(w, [p for p, _ in batch], [c for _, c in batch], S, S, 3, 2)
        _equal(y, kb.maxpool(torch.relu(want), pad=1), f"stem_conv_pool S={S} strip={strip} {batch}")


# ---------------------------------------------------------------- conv3x3_block (layer1's fused basic block)
BLOCK_RING = kb.kernel_const("conv3x3_block.hip", "kRing")


@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_block(gpu, B):
    """Under the chained bar (kb.chained); controls on conv1's output and on
    conv2's (test_kernel_bar_cpu.py checks on these operands that the bar's
    delta term leaves every control above 1)."""
    x, w1, b1, w2, b2 = kb.block_operands(B, seed=130 + B)
    ref, bnd, _, _ = kb.chained(x, w1, b1, w2, b2)
    y = ops.conv3x3_block(_dev(x, gpu), _pack(w1, gpu), b1.float().to(gpu), _pack(w2, gpu), b2.float().to(gpu))
    y = kb.nchw(y.cpu())
    what = f"conv3x3_block B={B}"
    kb.assert_close(y, torch.relu(ref), bnd, what)
    for name, wrong in kb.block_controls(x, w1, b1, w2, b2, BLOCK_RING):
        kb.assert_rejects(y, torch.relu(wrong), bnd, f"{what} [{name}]")


def _identity3x3(C):
    w = torch.zeros(C, C, 3, 3, dtype=torch.float64)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    return w


@pytest.mark.parametrize("role", ["consumer", "producer"])
def test_conv3x3_block_impulse(gpu, role):
    """One role at a time, the other conv the centre-tap identity, zero
    biases, weights multiples of 2^-8 in [-1, 1): every sum is exact in fp32.
    consumer: x >= 0 passes conv1 unchanged, y = bf16(relu(conv2(x) + x)) pins
    the consumer waves and their reads of the LDS ring. producer: conv2 passes
    t = relu(conv1(x)) on, y = bf16(t + x) pins the producer waves."""
    g = torch.Generator().manual_seed(132)
    w = torch.randint(-256, 256, (64, 64, 3, 3), generator=g).double() / 256
    ident = _identity3x3(64)
    w1, w2 = (ident, w) if role == "consumer" else (w, ident)
    wp1, wp2, zero = _pack(w1, gpu), _pack(w2, gpu), torch.zeros(64, device=gpu)
    # rows 9 | 10, 19 | 20, 49 | 50: the 10-row rings' wraps (row r in slot r % 10); the image's corners
    pixels = [(9, 0), (10, 55), (19, 27), (20, 28), (49, 1), (50, 54), (0, 0), (55, 55), (0, 55)]
    for batch in _impulse_batches(pixels, _chans(64), n=9):
        x = _impulse_input(batch, 64, 56, 56, gpu)
        y = ops.conv3x3_block(x, wp1, zero, wp2, zero)
        conv = _impulse_expected(w, [p for p, _ in batch], [c for _, c in batch], 56, 56, 1)
        xi = kb.nchw(x.cpu()).double()
        want = kb.bf16r(torch.relu(conv + xi)) if role == "consumer" else kb.bf16r(torch.relu(conv) + xi)
        _equal(y, want, f"conv3x3_block {role} {batch}")


# ---------------------------------------------------------------- workgroup start stagger
def _staggered(family, run):
    C = dmlc.native()
    y0 = run()
    C.kernel_stagger_set(family, 4)
    try:
        assert C.kernel_stagger(family) == 4
        y1 = run()
        torch.cuda.synchronize()
    finally:
        C.kernel_stagger_set(family, -1)
    assert torch.equal(y0, y1), "the start stagger changed the result"


def test_stagger_stream(gpu):
    """56x56x64 in 8-row strips: B = 3 is the smallest batch with 16 or more
    workgroups (21); those with (blockIdx.x >> 3) & 1 start late."""
    B = 3
    x, w, bias = _operands(B, 64, 64, 56, 3, 203)
    xd, wp, bg, rd = _dev(x, gpu), _pack(w, gpu), bias.float().to(gpu), _dev(_residual(B, 64, 56, 7), gpu)
    _staggered(dmlc.native().STAG_STREAM, lambda: ops.conv3x3_stream(xd, wp, bg, rd, True))


def test_stagger_rows28(gpu):
    """One workgroup per image: B = 16, workgroups 8 .. 15 start late."""
    B = 16
    g = torch.Generator().manual_seed(280)
    xd = torch.randn(B, 28, 28, 128, generator=g).bfloat16().to(gpu)
    rd = torch.randn(B, 28, 28, 128, generator=g).bfloat16().to(gpu)
    _, w, bias = _operands(1, 128, 128, 28, 3, 221)
    wp, bg = _pack(w, gpu), bias.float().to(gpu)
    _staggered(dmlc.native().STAG_ROWS28, lambda: ops.conv3x3_rows28(xd, wp, bg, rd, True))

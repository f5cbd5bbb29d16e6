"""Op-level tests of the fused / shape-specialised kernels that the engine
tests reach only through whole-model logits: alex_stem, conv5x5_27,
conv3x3_13, fc_small, the fused and pooled classifier heads and
conv3x3_stream's average-pool epilogue.

Each is compared element-wise with a float64 reference on the same
bf16-rounded operands under the bar of tests/_kernel_bar.py (derived from the
arithmetic, see there), keeps the project's relative-L2 bar, and carries a
negative control: a reference with one modelled kernel fault must be rejected.
The direct convs also get impulse tests with exact equality (one 1.0 in the
input: every output is one bf16 weight or zero).

Measured on an MI355X, worst |err| / bar over a kernel's cases and its largest
relative L2: conv3x3_13 0.69, 1.7e-3 (fused pool 0.57); conv5x5_27 0.73,
1.7e-3 (fused pool 0.73); alex_stem 0.95, 1.6e-3 (K = 363: almost no
summation slack, and the bar's rounding term is bf16's first-order worst
case); fc_small 0.87, 1.7e-3; conv3x3_stream y 0.50, its pool 0.12, 1.8e-3;
head_fused 0.08, 3.3e-3 (e4m3 input 0.04); head_pooled < 0.001, 2.8e-7 (its
input is already bf16). The weakest negative control sits at 1.9 times the
bar (the stream conv's pool with its last pixel left out).

ResNet50's layer1 kernels (bottleneck56_head, bottleneck56), conv1x1's block
loop and conv1x1_chain have theirs in test_kernels_resnet50_gpu.py.
"""
import pytest
import torch
import torch.nn.functional as F

import dmlc
from dmlc import ops

import _kernel_bar as kb

pytestmark = pytest.mark.gpu


def _conv_operands(B, Cin, Cout, H, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, H, generator=g).bfloat16().double()
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).bfloat16().double()
    bias = (torch.randn(Cout, generator=g) * 0.1).float().double()
    return x, w, bias


def _dev(x_nchw, gpu):
    return kb.nhwc(x_nchw).bfloat16().to(gpu)


def _controls(ref, x, w, pad, B, pooled=False):
    swap = kb.fault_chunk_swap_at_max(ref, b=B - 1, chunk=3) if pooled else \
        kb.fault_chunk_swap(ref, b=B - 1, h=ref.shape[2] - 1, w=ref.shape[3] - 2, chunk=3)
    out = [("border taps", kb.fault_border_taps(ref, x, w, pad)), ("chunk swap", swap)]
    if B > 1:
        out.append(("batch shift", kb.fault_batch_shift(ref)))
    return out


# ---------------------------------------------------------------- impulse tests
def _impulse_expected(w, pix, chans, H, pad):
    """[B, Cout, H, H] float64: image i holds w[:, c_i, kh, kw] at the pixel
    the tap (kh, kw) displaces pixel p_i to, zero elsewhere."""
    Cout, _, k, _ = w.shape
    out = torch.zeros(len(pix), Cout, H, H, dtype=torch.float64)
    for i, (p, c) in enumerate(zip(pix, chans)):
        r, col = divmod(p, H)
        for kh in range(k):
            for kw in range(k):
                orow, ocol = r + pad - kh, col + pad - kw
                if 0 <= orow < H and 0 <= ocol < H:
                    out[i, :, orow, ocol] = w[:, c, kh, kw]
    return out


def _impulse_batches(pixels, chans):
    combos = [(p, c) for p in pixels for c in chans]
    return [combos[i:i + 5] for i in range(0, len(combos), 5)]


def _impulse_input(batch, Cin, H, gpu):
    x = torch.zeros(len(batch), H, H, Cin, dtype=torch.bfloat16)
    for i, (p, c) in enumerate(batch):
        x[i, p // H, p % H, c] = 1.0
    return x.to(gpu)


@pytest.mark.parametrize("Cin,Cout", [(192, 384), (384, 256), (256, 256)])
def test_conv3x3_13_impulse(gpu, Cin, Cout):
    # corners, an edge midpoint, the centre; 168 is also the last pixel (the partial fragment of 9)
    pixels = [0, 12, 156, 168, 6, 84]
    chans = [0, Cin - 1, 8 * 5 + 3] + ([8 * 19 + 4] if Cin == 192 else [8 * (Cin // 8 - 2) + 5])
    _, w, _ = _conv_operands(1, Cin, Cout, 13, 3, seed=20)
    wp = ops.pack_conv_weight(w.float(), device=gpu)[:Cout].contiguous()
    zero = torch.zeros(Cout, device=gpu)
    for batch in _impulse_batches(pixels, chans):
        x = _impulse_input(batch, Cin, 13, gpu)
        want = _impulse_expected(w, [p for p, _ in batch], [c for _, c in batch], 13, 1)
        y = ops.conv3x3_13(x, wp, zero, relu=False)
        assert torch.equal(kb.nchw(y.cpu()).double(), want), batch
        if ops.native().conv3x3_13_pool_supported(Cin, Cout):
            yp = ops.conv3x3_13(x, wp, zero, relu=True, pool=True)
            assert yp.shape == (len(batch), 6, 6, Cout)
            assert torch.equal(kb.nchw(yp.cpu()).double(), kb.maxpool(torch.relu(want))), batch


def test_conv5x5_27_impulse(gpu):
    # corners, an edge midpoint, the centre; 728 is also the last pixel (duplicated by the last wave's spare fragments)
    pixels = [0, 26, 702, 728, 13, 364]
    chans = [0, 63, 8 * 4 + 3]
    _, w, _ = _conv_operands(1, 64, 192, 27, 5, seed=21)
    wp = ops.pack_conv_weight(w.float(), device=gpu)
    zero = torch.zeros(192, device=gpu)
    for batch in _impulse_batches(pixels, chans):
        x = _impulse_input(batch, 64, 27, gpu)
        want = torch.relu(_impulse_expected(w, [p for p, _ in batch], [c for _, c in batch], 27, 2))
        y = ops.conv5x5_27(x, wp, zero)
        assert torch.equal(kb.nchw(y.cpu()).double(), want), batch
        yp = ops.conv5x5_27(x, wp, zero, pool=True)
        assert yp.shape == (len(batch), 13, 13, 192)
        assert torch.equal(kb.nchw(yp.cpu()).double(), kb.maxpool(want)), batch


# ---------------------------------------------------------------- random inputs under the bar
@pytest.mark.parametrize("Cin,Cout", [(192, 384), (384, 256), (256, 256)])
@pytest.mark.parametrize("B", [1, 3])
def test_conv3x3_13(gpu, Cin, Cout, B):
    x, w, bias = _conv_operands(B, Cin, Cout, 13, 3, seed=30 + B)
    ref, mag = kb.conv_ref(x, w, bias, 1, 1)
    wp = ops.pack_conv_weight(w.float(), device=gpu)[:Cout].contiguous()
    xd, bd = _dev(x, gpu), bias.float().to(gpu)
    for relu in (False, True):
        r = torch.relu(ref) if relu else ref
        bnd = kb.bound(r, mag, 9 * Cin)
        y = kb.nchw(ops.conv3x3_13(xd, wp, bd, relu=relu).cpu())
        kb.assert_close(y, r, bnd, f"conv3x3_13 {Cin}->{Cout} B={B} relu={relu}")
        for name, wrong in _controls(ref, x, w, 1, B):
            kb.assert_rejects(y, torch.relu(wrong) if relu else wrong, bnd, name)
    if (Cin, Cout) == (256, 256):
        bnd = kb.maxpool(kb.bound(torch.relu(ref), mag, 9 * Cin))
        yp = ops.conv3x3_13(xd, wp, bd, relu=True, pool=True)
        assert yp.shape == (B, 6, 6, 256)
        yp = kb.nchw(yp.cpu())
        kb.assert_close_pooled(yp, torch.relu(ref), kb.bound(torch.relu(ref), mag, 9 * Cin), f"conv3x3_13 + pool B={B}")
        for name, wrong in _controls(ref, x, w, 1, B, pooled=True):
            kb.assert_rejects(yp, kb.maxpool(torch.relu(wrong)), bnd, name)
        with pytest.raises(ValueError):
            ops.conv3x3_13(xd, wp, bd, relu=False, pool=True)
    else:
        with pytest.raises(ValueError):
            ops.conv3x3_13(xd, wp, bd, relu=True, pool=True)


def test_conv3x3_13_bad_shapes(gpu):
    x = torch.zeros(1, 14, 14, 256, dtype=torch.bfloat16, device=gpu)
    wp = torch.zeros(256, 9 * 256, dtype=torch.bfloat16, device=gpu)
    b = torch.zeros(256, device=gpu)
    with pytest.raises(ValueError):
        ops.conv3x3_13(x, wp, b, relu=True)
    with pytest.raises(ValueError):
        ops.conv3x3_13(x[:, :13, :13, :128].contiguous(), wp, b, relu=True)
    with pytest.raises(ValueError):
        ops.conv5x5_27(x, wp, b)


def test_direct_conv_bad_operands(gpu):
    """The launchers refuse a bias they cannot read as float4 and an output
    that overlaps the input (another workgroup's image would be overwritten
    while it is staged). Every operand is a view into an allocation large
    enough for a launch that wrongly went ahead."""
    C = ops.native()
    zero, s = ops._ptr(ops._zero_page(torch.device(gpu))), ops._stream()
    bias = torch.zeros(256 + 8, device=gpu)
    # 13x13, 256 -> 256: x and y have the same size
    x13 = torch.zeros(1, 13, 13, 256, dtype=torch.bfloat16, device=gpu)
    wp13 = torch.zeros(256, 9 * 256, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError):
        ops.conv3x3_13(x13, wp13, bias[1:257], relu=True)
    wf13 = ops.stream_weight_frag(wp13, 256)
    y13 = torch.empty_like(x13)
    for relu, ypool in ((True, 0), (True, ops._ptr(x13))):
        with pytest.raises(ValueError):
            C.conv3x3_13(ops._ptr(x13), ops._ptr(wf13), ops._ptr(bias), ops._ptr(x13) if not ypool else ops._ptr(y13),
                         zero, 1, 256, 256, relu, s, ypool)
    # 27x27, 64 -> 192: x is the head of an allocation of y's size
    buf = torch.zeros(1, 27, 27, 192, dtype=torch.bfloat16, device=gpu)
    x27 = buf.view(-1)[:27 * 27 * 64].view(1, 27, 27, 64)
    wp27 = torch.zeros(192, 1600, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError):
        ops.conv5x5_27(x27, wp27, bias[1:193])
    wf27 = ops.stream_weight_frag(wp27, 192)
    with pytest.raises(ValueError):
        C.conv5x5_27(ops._ptr(x27), ops._ptr(wf27), ops._ptr(bias), ops._ptr(buf), zero, 1, s, 0)
    with pytest.raises(ValueError):
        C.conv5x5_27(ops._ptr(x27), ops._ptr(wf27), ops._ptr(bias), 0, zero, 1, s, ops._ptr(buf))
    torch.cuda.synchronize()


@pytest.mark.parametrize("B", [1, 2])
def test_conv5x5_27(gpu, B):
    x, w, bias = _conv_operands(B, 64, 192, 27, 5, seed=40 + B)
    ref, mag = kb.conv_ref(x, w, bias, 1, 2)
    r = torch.relu(ref)
    wp = ops.pack_conv_weight(w.float(), device=gpu)
    xd, bd = _dev(x, gpu), bias.float().to(gpu)
    bnd = kb.bound(r, mag, 1600)
    y = ops.conv5x5_27(xd, wp, bd)
    assert y.shape == (B, 27, 27, 192)
    y = kb.nchw(y.cpu())
    kb.assert_close(y, r, bnd, f"conv5x5_27 B={B}")
    controls = _controls(ref, x, w, 2, B)
    for name, wrong in controls:
        kb.assert_rejects(y, torch.relu(wrong), bnd, name)
    yp = ops.conv5x5_27(xd, wp, bd, pool=True)
    assert yp.shape == (B, 13, 13, 192)
    yp = kb.nchw(yp.cpu())
    pb = kb.maxpool(bnd)
    kb.assert_close_pooled(yp, r, bnd, f"conv5x5_27 + pool B={B}")
    for name, wrong in _controls(ref, x, w, 2, B, pooled=True):
        kb.assert_rejects(yp, kb.maxpool(torch.relu(wrong)), pb, name)


@pytest.mark.parametrize("B", [1, 3])
def test_alex_stem(gpu, B):
    g = torch.Generator().manual_seed(50 + B)
    img = torch.randint(0, 256, (B + 1, 224, 224, 3), generator=g, dtype=torch.uint8)
    img[B] = 0  # 255 on the outermost two rows and columns: the padding taps dominate the border outputs
    img[B, :2] = 255
    img[B, -2:] = 255
    img[B, :, :2] = 255
    img[B, :, -2:] = 255
    w = (torch.randn(64, 3, 11, 11, generator=g) / 363 ** 0.5).bfloat16().double()
    bias = (torch.randn(64, generator=g) * 0.1).float().double()
    imd = img.to(gpu)
    xin = ops.preprocess_u8(imd, 224, 0)  # the kernel's input values (test_preprocess_identity pins them to torch)
    assert xin.shape == (B + 1, 224, 224, 3)
    x = kb.nchw(xin.cpu()).double()
    ref, mag = kb.conv_ref(x, w, bias, 4, 2)
    r = torch.relu(ref)
    cb = kb.bound(r, mag, 363)
    bnd = kb.maxpool(cb)
    y = ops.alex_stem(imd, ops.pack_alex_stem_weight(w.float(), device=gpu), bias.float().to(gpu))
    assert y.shape == (B + 1, 27, 27, 64)
    y = kb.nchw(y.cpu())
    kb.assert_close_pooled(y, r, cb, f"alex_stem B={B + 1}")
    # the top padding rows' neighbours: conv row 1 (kh = 0, 1 reach image rows 2, 3) loses its kh = 0 taps
    lost = F.conv2d(x[:, :, 2:3, :], w[:, :, 0:1, :], None, (1, 4), (0, 2))
    wrong = ref.clone()
    wrong[:, :, 1:2, :] -= lost
    for name, wr in (("border taps", wrong), ("chunk swap", kb.fault_chunk_swap_at_max(ref, b=B - 1, chunk=5)),
                     ("batch shift", kb.fault_batch_shift(ref))):
        kb.assert_rejects(y, kb.maxpool(torch.relu(wr)), bnd, name)
    with pytest.raises(ValueError):
        ops.alex_stem(imd[:, :220, :220].contiguous(), ops.pack_alex_stem_weight(w.float(), device=gpu),
                      bias.float().to(gpu))


FC_SMALL_CASES = [
    # B, K, N, relu, out_f32, ldx
    (1, 32, 16, False, False, 32),        # 1 K step: 7 idle waves
    (3, 64, 24, True, False, 64),         # 2 K steps, N not a multiple of 16
    (16, 544, 1000, True, False, 544),    # 17 K steps: a ragged wave split
    (5, 4128, 1000, False, False, 4128),  # 129 K steps, 17 per wave: across the unroll of 16
    (16, 4096, 1000, False, True, 4096),  # fp32 output
    (1, 9216, 4096, True, False, 9216),
    (5, 544, 1000, True, False, 1088),    # a column slice of a wider activation
]


@pytest.mark.parametrize("case", FC_SMALL_CASES, ids=[str(c) for c in FC_SMALL_CASES])
def test_fc_small(gpu, case):
    B, K, N, relu, f32, ldx = case
    g = torch.Generator().manual_seed(60 + K % 97)
    wide = torch.randn(B, ldx, generator=g).bfloat16()
    off = (ldx - K) // 2 // 8 * 8
    w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().double()
    bias = (torch.randn(N, generator=g) * 0.1).float().double()
    x = wide[:, off:off + K].double()
    ref, mag = kb.fc_ref(x, w, bias)
    r = torch.relu(ref) if relu else ref
    npad = (N + 15) // 16 * 16
    wp = torch.zeros(npad, K, dtype=torch.bfloat16)
    wp[:N] = w.bfloat16()
    dt = torch.float32 if f32 else torch.bfloat16
    canary = 768.0  # exact in bf16
    out = torch.full((B + 2, N + 9), canary, dtype=dt, device=gpu)
    xd = wide.to(gpu)[:, off:off + K]
    y = ops.fc_small(xd, wp.to(gpu), N, bias.float().to(gpu), relu=relu, out_f32=f32, out=out)
    assert y.shape == (B, N) and y.dtype == dt
    bnd = kb.bound(r, mag, K, out_bf16=not f32)
    kb.assert_close(y.cpu(), r, bnd, f"fc_small {case}")
    o = out.cpu().float()
    assert bool((o[B:] == canary).all()) and bool((o[:, N:] == canary).all()), "wrote outside [B, N]"
    if B > 1:
        kb.assert_rejects(y.cpu(), kb.fault_batch_shift(r), bnd, "batch shift")
    if K >= 256:  # one wave's K range left out of the sum
        per = -(-(K // 32) // 8) * 32
        short, _ = kb.fc_ref(x[:, per:], w[:, per:], bias)
        kb.assert_rejects(y.cpu(), torch.relu(short) if relu else short, bnd, "a wave's K range")
    else:  # the bias left out
        nob, _ = kb.fc_ref(x, w, torch.zeros_like(bias))
        kb.assert_rejects(y.cpu(), torch.relu(nob) if relu else nob, bnd, "no bias")
    # without out=: a fresh [B, N]
    y2 = ops.fc_small(xd, wp.to(gpu), N, bias.float().to(gpu), relu=relu, out_f32=f32)
    assert torch.equal(y2, y)


def test_fc_small_bad_shapes(gpu):
    w = torch.zeros(16, 64, dtype=torch.bfloat16, device=gpu)
    b = torch.zeros(16, device=gpu)
    with pytest.raises(ValueError):  # more than 16 rows
        ops.fc_small(torch.zeros(17, 64, dtype=torch.bfloat16, device=gpu), w, 16, b)
    with pytest.raises(ValueError):  # K not a multiple of 32
        ops.fc_small(torch.zeros(2, 48, dtype=torch.bfloat16, device=gpu), w, 16, b)
    with pytest.raises(ValueError):  # more classes than weight rows
        ops.fc_small(torch.zeros(2, 64, dtype=torch.bfloat16, device=gpu), w, 17, b)
    with pytest.raises(ValueError):  # K wider than the weights
        ops.fc_small(torch.zeros(2, 96, dtype=torch.bfloat16, device=gpu), w, 16, b)


@pytest.mark.parametrize("B", [1, 3, 4])
@pytest.mark.parametrize("use_res", [False, True])
@pytest.mark.parametrize("frag", [False, True])
def test_conv3x3_stream_pool(gpu, B, use_res, frag):
    x, w, bias = _conv_operands(B, 512, 512, 7, 3, seed=70 + B)
    g = torch.Generator().manual_seed(7)
    res = torch.randn(B, 512, 7, 7, generator=g).bfloat16().double() if use_res else None
    ref, mag = kb.conv_ref(x, w, bias, 1, 1, res)
    r = torch.relu(ref)
    wp = ops.pack_conv_weight(w.float(), device=gpu)
    xd, bd = _dev(x, gpu), bias.float().to(gpu)
    rd = _dev(res, gpu) if use_res else None
    y0 = ops.conv3x3_stream(xd, wp, bd, res=rd, relu=True, frag=frag)
    y1, pool = ops.conv3x3_stream(xd, wp, bd, res=rd, relu=True, frag=frag, pool=True)
    assert torch.equal(y0, y1), "pool changed y"
    ybnd = kb.bound(r, mag, 9 * 512)
    kb.assert_close(kb.nchw(y1.cpu()), r, ybnd, f"conv3x3_stream y B={B} res={use_res} frag={frag}")
    yr = kb.nhwc(r).reshape(B, 49, 512)
    bnd = kb.avgpool_bound(yr, kb.nhwc(ybnd).reshape(B, 49, 512))
    assert pool.shape == (B, 512)
    kb.assert_close(pool.cpu(), yr.mean(1), bnd, f"conv3x3_stream pool B={B} res={use_res} frag={frag}")
    wrong = kb.nhwc(torch.relu(kb.fault_border_taps(ref, x, w, 1))).reshape(B, 49, 512).mean(1)
    kb.assert_rejects(pool.cpu(), wrong, bnd, "border taps")
    kb.assert_rejects(pool.cpu(), yr[:, :48].sum(1) / 49, bnd, "last pixel left out")
    if B > 1:
        kb.assert_rejects(pool.cpu(), kb.fault_batch_shift(yr.mean(1)), bnd, "batch shift")
    canary = torch.full_like(y0, 768.0)
    y2, pool2 = ops.conv3x3_stream(xd, wp, bd, res=rd, relu=True, frag=frag, pool=True, store_y=False, out=canary)
    torch.cuda.synchronize()
    assert bool((canary == 768.0).all()), "store_y=False wrote y"
    assert torch.equal(pool2, pool)


def test_conv3x3_stream_pool_unsupported(gpu):
    assert not ops.native().conv3x3_stream_pool_supported(14, 14, 256, 256, 1)
    x = torch.zeros(1, 14, 14, 256, dtype=torch.bfloat16, device=gpu)
    wp = torch.zeros(256, 9 * 256, dtype=torch.bfloat16, device=gpu)
    b = torch.zeros(256, device=gpu)
    with pytest.raises(ValueError):
        ops.conv3x3_stream(x, wp, b, pool=True)
    with pytest.raises(ValueError):
        ops.conv3x3_stream(x, wp, b, pool=True, store_y=False)


# ---------------------------------------------------------------- classifier heads
def _head_operands(B, HW, C, N, seed, ties=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HW, C, generator=g).bfloat16()
    w = (torch.randn(N, C, generator=g) / C ** 0.5).bfloat16()
    bias = (torch.randn(N, generator=g) * 0.1).float()
    if ties is not None:  # identical, dominant rows: bit-equal logits
        a, b = ties
        w[b] = w[a]
        bias[a] = bias[b] = 40.0
    npad = (N + 15) // 16 * 16
    wp = torch.zeros(npad, C, dtype=torch.bfloat16)
    wp[:N] = w
    return x, w, bias, wp


def _check_head(out, x64_mean, xabs_mean, w, bias, C, what, B):
    logits, idx, prob = (t.cpu() for t in out)
    ref, _ = kb.fc_ref(x64_mean, w, bias)
    _, mag = kb.fc_ref(xabs_mean, w, bias)
    bnd = kb.head_bound(mag, C)
    kb.assert_close(logits, ref, bnd, what)
    if B > 1:
        kb.assert_rejects(logits, kb.fault_batch_shift(ref), bnd, "batch shift")
    else:
        kb.assert_rejects(logits, torch.roll(ref, 1, 1), bnd, "class shift")
    assert torch.equal(idx.long(), logits.argmax(-1)), what
    want = torch.softmax(logits, -1).max(-1).values
    assert torch.allclose(prob, want, rtol=1e-4, atol=1e-6), what
    N = logits.shape[1]
    if N >= 32:  # a split's classes left out of the sum (one not holding the top class)
        lo = 0 if int(idx.min()) >= 16 else N - 16
        if not bool(((idx >= lo) & (idx < lo + 16)).any()):
            assert not torch.allclose(prob, kb.prob_without_split(logits, lo, lo + 16).float(), rtol=1e-4, atol=1e-6)
    return logits, idx, prob


def _check_top1_kernel(out):
    idx1, prob1 = ops.softmax_top1(out[0])
    assert torch.equal(idx1, out[1])
    assert torch.allclose(prob1, out[2], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("C", [32, 256, 512, 1024, 2048])
@pytest.mark.parametrize("N", [10, 17, 1000])
def test_head_fused(gpu, C, N):
    for B in (1, 4, 5, 9):
        x, w, bias, wp = _head_operands(B, 49, C, N, seed=80 + B)
        out = ops.head(x.to(gpu), wp.to(gpu), N, bias.to(gpu))
        assert out[0].shape == (B, N) and out[1].shape == (B,) and out[2].shape == (B,)
        _check_head(out, x.double().mean(1), x.double().abs().mean(1), w, bias, C, f"head_fused C={C} N={N} B={B}", B)
        _check_top1_kernel(out)


@pytest.mark.parametrize("B", [1, 5])
def test_head_fused_fp8(gpu, B):
    C, N = 2048, 1000
    x, w, bias, wp = _head_operands(B, 49, C, N, seed=90 + B)
    scale = float(x.float().abs().max()) / ops.FP8_MAX
    x8 = ops.quantize_fp8(x.float().abs(), scale)  # a post-ReLU activation
    xv = x8.float().double() * scale
    out = ops.head(x8.to(gpu), wp.to(gpu), N, bias.to(gpu), in_fp8_scale=scale)
    _check_head(out, xv.mean(1), xv.abs().mean(1), w, bias, C, f"head_fused e4m3 B={B}", B)
    x512 = ops.quantize_fp8(torch.rand(B, 49, 512), 1.0).to(gpu)
    with pytest.raises(ValueError):
        ops.head(x512, wp[:, :512].contiguous().to(gpu), N, bias.to(gpu), in_fp8_scale=1.0)


@pytest.mark.parametrize("C", [512, 2048])
@pytest.mark.parametrize("splits", [0, 1, 2, 8, 16])
def test_head_pooled(gpu, C, splits):
    N = 1000
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    for B in (1, 16, 17, 33):
        ns = splits or dmlc.native().head_pooled_splits(B, N, cus)
        print(f"head_pooled C={C} B={B}: {ns} class splits")
        x, w, bias, wp = _head_operands(B, 1, C, N, seed=100 + B)
        p = x[:, 0]
        out = ops.head(p.to(gpu), wp.to(gpu), N, bias.to(gpu), pooled=True, splits=splits)
        _check_head(out, p.double(), p.double().abs(), w, bias, C, f"head_pooled C={C} B={B} splits={ns}", B)
        _check_top1_kernel(out)


@pytest.mark.parametrize("ties", [(3, 7), (3, 900)], ids=["one tile", "across splits"])
def test_head_ties_go_to_the_lower_class(gpu, ties):
    N, C = 1000, 512
    a, b = ties
    for B in (1, 5, 17):
        x, w, bias, wp = _head_operands(B, 49, C, N, seed=110 + B, ties=ties)
        outs = [("fused", ops.head(x.to(gpu), wp.to(gpu), N, bias.to(gpu)))]
        pooled = x.float().mean(1).bfloat16()
        for splits in (0, 1, 2, 8, 16):
            outs.append((f"pooled splits={splits}",
                         ops.head(pooled.to(gpu), wp.to(gpu), N, bias.to(gpu), pooled=True, splits=splits)))
        for what, (logits, idx, prob) in outs:
            lg = logits.cpu()
            assert torch.equal(lg[:, a], lg[:, b]), f"{what}: the tied logits are not bit-equal"
            assert bool((lg[:, a] > lg.clone().index_fill_(1, torch.tensor([a, b]), -1e30).max(-1).values + 10).all())
            assert idx.cpu().tolist() == [a] * B, f"{what} B={B}: top-1 {idx.cpu().tolist()}"
            assert torch.allclose(prob.cpu(), torch.softmax(lg, -1)[:, a], rtol=1e-4, atol=1e-6), what
            i1, _ = ops.softmax_top1(logits)
            assert torch.equal(i1, idx), what


def test_head_workspace_reuse(gpu):
    N, C = 1000, 512
    for pooled in (False, True):
        outs = {}
        for B in (9, 9, 33, 2, 9):  # the same call twice, then other batch sizes on the same workspace
            x, w, bias, wp = _head_operands(B, 49, C, N, seed=120 + B)
            xin = x.float().mean(1).bfloat16() if pooled else x
            out = ops.head(xin.to(gpu), wp.to(gpu), N, bias.to(gpu), pooled=pooled)
            xm = xin.double() if pooled else x.double().mean(1)
            xa = xin.double().abs() if pooled else x.double().abs().mean(1)
            _check_head(out, xm, xa, w, bias, C, f"head pooled={pooled} B={B} (workspace reuse)", B)
            got = tuple(t.cpu() for t in out)
            if B in outs:
                assert all(torch.equal(p, q) for p, q in zip(outs[B], got)), f"B={B}: a repeated call differs"
            outs[B] = got

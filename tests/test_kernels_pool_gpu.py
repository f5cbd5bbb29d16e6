"""pool.hip's kernels at the op level.

avgpool_global (two kernels, switched at B = 32, each with a bf16 and an e4m3
input form): bit-equal to _pool_ref._pool_emulated, which performs the
kernels' stated order literally in torch fp32 (part p = pixels p, p + 8, ...
summed in order onto 0, the parts combined as ((0+1)+(2+3))+((4+5)+(6+7)), one
multiply by (scale or 1) / HW, rounded to bf16). The cases reach both kernels
in both input types, the 8-lane kernel's second trip of its 64-pixel loop
(HW = 81, 100), the rows kernel's third and later 24-pixel blocks with a
partial last one (HW = 81: 24 + 24 + 24 + 9), a second x-block with one live
lane (C = 2056) and a part-filled wave. e4m3 inputs are random bytes (their
sums are exact in any order) and are also bit-equal to ops.embed_rows, which
promises this arithmetic; bf16 inputs carry a cancelling pixel pair, so the
order shows: the same mean summed in plain pixel order differs (the negative
control). Every output is written into a buffer with a sentinel tail.

maxpool2d: equal to F.max_pool2d on the bf16 values (a maximum is exact):
the ResNet stem's pool, AlexNet's three, a non-square image, a 2x2 window, an
all-negative input whose zero-padded reference must differ (the kernel pads
with -inf), and one shape of 2 227 200 work items, more than the grid's
8192 x 256 threads and no multiple of them, which enters the grid-stride loop.

avgpool_adaptive: bit-equal to a torch fp32 emulation of the kernel's stated
arithmetic (bins [floor(i H / Ho), ceil((i + 1) H / Ho)), pixels added in
(h, w) order onto 0, one multiply by fp32(1 / n), rounded to bf16), and
within 2^-8 |ref| + n 2^-23 mean|x| of float64 F.adaptive_avg_pool2d
(_kernel_bar's rounding argument: the bf16 rounding of the output, an n-term
fp32 sum, and the two roundings of the factor 1 / n and its product, 2 2^-24,
inside the doubled summation term). 13 -> 6, the identity 6 -> 6 (the input's
bits), 7 -> 3, 5 -> 6 (overlapping bins) and 13x9 -> 6x6. The control: bins
[floor, floor), which leave out the ceil row, miss the bar at 13 -> 6.

Measured on an MI355X: every avgpool_global, maxpool2d and avgpool_adaptive
case is bit-equal to its reference; 75 % of avgpool_global's elements differ
from the plain-pixel-order control at HW = 81; avgpool_adaptive's worst
|err| / bar against float64 is 0.996 (the output's bf16 rounding just above a
power of two), and its control misses the bar by more than 10^5 x.
"""
import pytest
import torch
import torch.nn.functional as F

from _kernel_bar import EPS_OUT, EPS_SUM, assert_close, assert_rejects
from _pool_ref import _input, _pool_emulated, _widen
from dmlc import native, ops

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PAD = 64  # sentinel elements past the output
BF16 = torch.bfloat16


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------- avgpool_global
# (B, HW, C, e4m3 scale or None)
AVG_CASES = [
    (3, 49, 2048, 0.37),       # the 8-lane kernel, e4m3
    (33, 49, 2048, 0.37),      # the rows kernel, e4m3
    (40, 36, 512, 1.0 / 7),    # a partial 24-pixel block
    (5, 81, 512, None),        # the 8-lane kernel's second 64-pixel trip
    (5, 81, 512, 0.37),
    (32, 81, 512, None),       # the rows kernel's fourth, partial block, at the switch
    (32, 81, 512, 0.37),
    (32, 49, 2056, None),      # 257 channel groups: a second x-block with one live lane
    (31, 100, 64, None),       # a part-filled wave, below the switch
]


def _avg_id(c):
    B, HW, C, scale = c
    return f"b{B}-hw{HW}-c{C}" + ("-e4m3" if scale is not None else "")


def _avgpool_with_tail(x, scale):
    """avgpool_global of x [B, HW, C] (bf16, or e4m3 bytes) into a buffer with a sentinel tail, which must stay
    untouched; ops.avgpool_global returns the same bits."""
    B, HW, C = x.shape
    buf = torch.full((B * C + PAD,), SENTINEL, dtype=BF16, device=x.device)
    native().avgpool_global(x.data_ptr(), buf.data_ptr(), B, HW, C, torch.cuda.current_stream(x.device).cuda_stream,
                            in_fp8=scale is not None, scale=1.0 if scale is None else scale)
    torch.cuda.synchronize()
    assert torch.equal(buf[B * C:].cpu(), torch.full((PAD,), SENTINEL, dtype=BF16))
    y = ops.avgpool_global((x.view(ops.FP8) if scale is not None else x).view(B, HW, 1, C), scale=scale)
    torch.cuda.synchronize()
    assert y.shape == (B, C) and y.dtype == BF16
    assert torch.equal(_bits(y), _bits(buf[:B * C].view(B, C)))
    return y


@pytest.mark.parametrize("case", AVG_CASES, ids=_avg_id)
def test_avgpool_global(gpu, case):
    B, HW, C, scale = case
    x_cpu = _input(B, HW, C, scale, seed=1000 * B + HW + C, cancelling=True)
    want = _pool_emulated(_widen(x_cpu), scale)
    assert bool(torch.isfinite(want).all())
    x = x_cpu.to(gpu)
    y = _avgpool_with_tail(x, scale)
    differ = int((_bits(y.cpu()) != _bits(want.bfloat16())).sum())
    assert differ == 0, f"{differ} of {want.numel()} elements differ from the emulated order"
    if scale is not None:  # embed.hip's promise
        e = ops.embed_rows(x, scale=scale)
        torch.cuda.synchronize()
        assert torch.equal(e, y.float()) and torch.equal(_bits(e.bfloat16()), _bits(y))


@pytest.mark.parametrize("B", [5, 32])
def test_avgpool_global_rejects_sequential_order(gpu, B):
    """The negative control of the bit comparison, for both kernels: the same
    mean summed in plain pixel order differs at HW = 81."""
    HW, C = 81, 512
    x_cpu = _input(B, HW, C, None, seed=1000 * B + HW + C, cancelling=True)
    seq = _pool_emulated(x_cpu.float(), None, sequential=True)
    share = (seq != _pool_emulated(x_cpu.float(), None)).float().mean().item()
    print(f"avgpool_global B={B}: {share:.2f} of the elements differ in plain pixel order")
    assert share > 0.5, share
    y = _avgpool_with_tail(x_cpu.to(gpu), None)
    assert (y.float().cpu() != seq).float().mean().item() > 0.5


def test_avgpool_global_argument_checks(gpu):
    bf = torch.zeros(2, 3, 3, 16, dtype=BF16, device=gpu)
    with pytest.raises(ValueError):  # e4m3 without its scale
        ops.avgpool_global(torch.zeros(2, 3, 3, 16, dtype=torch.uint8, device=gpu).view(ops.FP8))
    with pytest.raises(ValueError):  # a scale with bf16
        ops.avgpool_global(bf, scale=0.5)
    with pytest.raises(ValueError):
        ops.avgpool_global(bf.float())
    with pytest.raises(ValueError):  # C % 8
        ops.avgpool_global(torch.zeros(2, 3, 3, 12, dtype=BF16, device=gpu))
    with pytest.raises(ValueError):
        ops.avgpool_global(torch.zeros(2, 3, 3, 12, dtype=torch.uint8, device=gpu).view(ops.FP8), scale=1.0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- maxpool2d
GRID_THREADS = 8192 * 256  # pool.hip's grid_for: at most 8192 blocks of 256


def _maxpool_check(gpu, x, k, s, p):
    """x: NHWC bf16 on the CPU. Returns (the kernel's output, the reference), NHWC bf16 on the CPU."""
    assert not bool(((x == 0) & (_bits(x) != 0)).any())  # no -0.0: fmaxf does not order the zeros
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1).contiguous()
    y = ops.maxpool2d(x.to(gpu), k, s, p)
    torch.cuda.synchronize()
    y = y.cpu()
    assert y.shape == ref.shape and y.dtype == BF16
    differ = int((_bits(y) != _bits(ref)).sum())
    assert differ == 0, f"{differ} of {ref.numel()} elements differ"
    return y, ref


# (B, H, W, C, k, stride, pad): the ResNet stem's pool, AlexNet's three, a non-square image, a 2x2 window
MAX_CASES = [(2, 112, 112, 64, 3, 2, 1), (2, 55, 55, 64, 3, 2, 0), (2, 27, 27, 192, 3, 2, 0), (2, 13, 13, 256, 3, 2, 0),
             (2, 57, 59, 8, 3, 2, 1), (2, 14, 14, 8, 2, 2, 0)]


@pytest.mark.parametrize("case", MAX_CASES, ids=["x".join(map(str, c[:4])) + "-k%ds%dp%d" % c[4:] for c in MAX_CASES])
def test_maxpool2d(gpu, case):
    B, H, W, C, k, s, p = case
    g = torch.Generator().manual_seed(H + W + C)
    _maxpool_check(gpu, torch.randn(B, H, W, C, generator=g).bfloat16(), k, s, p)


def test_maxpool2d_pads_with_minus_infinity(gpu):
    """An all-negative input with p = 1: the border windows' maxima are
    negative, which a zero padding would replace by 0 (the control)."""
    g = torch.Generator().manual_seed(11)
    x = (-torch.rand(2, 57, 59, 8, generator=g) - 0.5).bfloat16()
    y, ref = _maxpool_check(gpu, x, 3, 2, 1)
    zero_padded = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2, 0).permute(0, 2, 3, 1)
    assert bool((y < 0).all()) and not torch.equal(y, zero_padded)
    assert torch.equal(y[:, 1:-1, 1:-1], zero_padded[:, 1:-1, 1:-1]) and bool((zero_padded[:, 0] == 0).all())


def test_maxpool2d_grid_stride(gpu):
    """More work items than the grid has threads, and no multiple of them:
    some threads take a second item, some do not (the ResNet stem's pool at
    B = 256 has 6.4 M items). Integer values: quick to make; 0 is +0."""
    B, H, W, C = 10, 57, 59, 2048
    items = B * 29 * 30 * (C // 8)
    assert items > GRID_THREADS and items % GRID_THREADS != 0
    g = torch.Generator().manual_seed(12)
    x = torch.randint(-4000, 4000, (B, H, W, C), dtype=torch.int16, generator=g).to(BF16)
    y, _ = _maxpool_check(gpu, x, 3, 2, 1)
    assert y.shape == (B, 29, 30, C)


def test_maxpool2d_argument_checks(gpu):
    with pytest.raises(ValueError):
        ops.maxpool2d(torch.zeros(1, 8, 8, 12, dtype=BF16, device=gpu), 3, 2, 1)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- avgpool_adaptive
def _bins(n_in, n_out, ceil=True):
    return [(i * n_in // n_out, -(-(i + 1) * n_in // n_out) if ceil else (i + 1) * n_in // n_out) for i in range(n_out)]


def _adaptive(x, Ho, Wo, dtype, ceil=True):
    """The kernel's stated arithmetic in `dtype` on x [B, H, W, C]: (the result [B, Ho, Wo, C] in dtype, before any
    output rounding; the pixel counts [Ho, Wo])."""
    B, H, W, C = x.shape
    x = x.to(dtype)
    out, n = torch.zeros(B, Ho, Wo, C, dtype=dtype), torch.zeros(Ho, Wo, dtype=torch.float64)
    for i, (hs, he) in enumerate(_bins(H, Ho, ceil)):
        for j, (ws, we) in enumerate(_bins(W, Wo, ceil)):
            s = torch.zeros(B, C, dtype=dtype)
            for h in range(hs, he):
                for w in range(ws, we):
                    s = s + x[:, h, w]
            n[i, j] = (he - hs) * (we - ws)
            out[:, i, j] = s * (torch.tensor(1.0, dtype=dtype) / torch.tensor(float(n[i, j]), dtype=dtype))
    return out, n


# (H, W, Ho, Wo, C): AlexNet's 13 -> 6, the identity, 7 -> 3, overlapping bins (H < Ho), a non-square image
ADAPTIVE_CASES = [(13, 13, 6, 6, 256), (6, 6, 6, 6, 256), (7, 7, 3, 3, 256), (5, 5, 6, 6, 8), (13, 9, 6, 6, 256)]


@pytest.mark.parametrize("case", ADAPTIVE_CASES, ids=["%dx%d-%dx%d-c%d" % c for c in ADAPTIVE_CASES])
def test_avgpool_adaptive(gpu, case):
    H, W, Ho, Wo, C = case
    B = 2
    g = torch.Generator().manual_seed(100 * H + 10 * W + Ho)
    x = torch.randn(B, H, W, C, generator=g).bfloat16()
    y = ops.avgpool_adaptive(x.to(gpu), Ho, Wo)
    torch.cuda.synchronize()
    y = y.cpu()
    emu, n = _adaptive(x, Ho, Wo, torch.float32)
    assert y.shape == emu.shape and y.dtype == BF16
    differ = int((_bits(y) != _bits(emu.bfloat16())).sum())
    assert differ == 0, f"{differ} of {emu.numel()} elements differ from the emulated arithmetic"
    if (H, W) == (Ho, Wo):
        assert torch.equal(_bits(y), _bits(x))
    x64 = x.double().permute(0, 3, 1, 2)
    ref = F.adaptive_avg_pool2d(x64, (Ho, Wo)).permute(0, 2, 3, 1)
    bnd = EPS_OUT * ref.abs() + n.view(1, Ho, Wo, 1) * EPS_SUM * F.adaptive_avg_pool2d(x64.abs(), (Ho, Wo)).permute(0, 2, 3, 1)
    assert_close(y.double(), ref, bnd, f"avgpool_adaptive {H}x{W} -> {Ho}x{Wo}")
    if (H, Ho) == (13, 6):  # the control: bins without their ceil row (and column)
        assert_rejects(y.double(), _adaptive(x, Ho, Wo, torch.float64, ceil=False)[0], bnd,
                       f"avgpool_adaptive {H}x{W} -> {Ho}x{Wo} [floor bins]")


def test_avgpool_adaptive_argument_checks(gpu):
    with pytest.raises(ValueError):
        ops.avgpool_adaptive(torch.zeros(1, 13, 13, 12, dtype=BF16, device=gpu), 6, 6)
    torch.cuda.synchronize()

"""Op-level tests of the kernels that carry resnet50_fp8 and that the engine
tests reach only through whole-model logits: bottleneck56, bottleneck56_head,
conv1x1's block loop at several blocks per workgroup, its concatenated-K form
and conv1x1_chain.

As in test_kernels_resnet_gpu.py every output is compared element-wise with a
float64 reference on the same (bf16 / e4m3) operands under the derived bar of
tests/_kernel_bar.py (threshold 1.0), keeps the project's relative-L2 bar
(5e-3 bf16, 0.04 e4m3), and carries negative controls: a reference with one
modelled kernel fault must be rejected. Every output tensor is pre-filled
with NaN (e4m3 0x7f, bf16 0x7fc0), so an element that the kernel never wrote
fails. test_kernel_bar_cpu.py checks the bars and the controls on these
operands without a GPU.

The two fused bottleneck kernels also get an exact test: small integer
operands for which every fp32 value inside the kernel is exact
(kb.bottleneck_exact_operands), so the output bytes must equal the float64
result rounded to e4m3 / bf16, ties and the saturation at 448 included.

conv1x1's block loop runs on a grid sized for 8 and for 4 compute units, so a
workgroup walks 43 blocks with stride 8 (6 or 5 blocks each: the stage ring
wraps for S = 2 and S = 3, the residual's two register sets alternate with an
even and an odd tail). The 4-wave forms put two workgroups on a compute unit
and reach stride 8 at 4 units, the 8-wave forms at 8 (and at 4); a pixel's
bits do not depend on the grid, which the test asserts against the launch at
the device's own size.

Recorded on an MI355X (worst |err| / bar over a kernel's cases; its weakest
control ratio and which control), not thresholds:
  bottleneck56                 0.89     10 (t1 padding columns); exact: 0 bytes differ
  bottleneck56_head            0.89    706 (t1 padding rows); exact: 0 values differ
  conv1x1 loop, bf16 out       0.99    985 (stale stage slot, e4m3 in, 1-KB rows)
  conv1x1 loop, e4m3 out       0.94    863 (residual of the other register set, 1-KB rows)
  conv1x1 1 / 8 / 9 / 17       0.98 bf16, 0.94 e4m3   5941 (residual, 17 blocks)
  conv1x1 concatenated K       0.98  24457 (x2's K block read from x, 1 block)
  conv1x1_chain y / y2         0.94 / 0.94   3374 (stale ybuf, 9 blocks)
Largest relative L2 1.7e-3 (bf16 outputs), 2.7e-2 (e4m3). The control ratios
of the 1x1 forms are large because a ReLU zero has a bar of its summation
slack alone. bottleneck56's are the smallest: its bar carries the delta terms
of two bf16 intermediates (up to all of the bar on single elements, 0.39 of
it on average) and e4m3's 2^-4; each of its controls also changes bytes of
the exact test's expectation (test_kernel_bar_cpu.py).
"""
import pytest
import torch

import dmlc
from dmlc import ops

import _kernel_bar as kb

pytestmark = pytest.mark.gpu

RING = kb.kernel_const("bottleneck56.hip", "kRing")
FP8 = torch.float8_e4m3fn


def _nan_e4m3(shape, gpu):
    return torch.full(shape, 0x7F, dtype=torch.uint8, device=gpu).view(FP8)


def _nan_bf16(shape, gpu):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=gpu)


def _codes(t_nchw, gpu):
    """NCHW float64 e4m3 code values -> NHWC e4m3 on the device (exact)."""
    return kb.nhwc(t_nchw).float().to(FP8).to(gpu)


def _bf16(t_nchw, gpu):
    return kb.nhwc(t_nchw).bfloat16().to(gpu)


def _pack(w, gpu):
    return ops.pack_conv_weight(w.float(), device=gpu)


def _w1_e4m3(o, gpu):
    """conv1's e4m3 codes and a1 on the device. The random operands hold what
    ops.pack_conv_weight_fp8 produces (kb.e4m3_weights, compared with it
    below); the exact test gives integer codes and its own a1."""
    return o["w1"].reshape(64, 256).float().to(FP8).to(gpu), o["a1"].float().to(gpu)


# ---------------------------------------------------------------- bottleneck56
def _run_bottleneck(o, gpu):
    B = o["x"].shape[0]
    w1q, a1 = _w1_e4m3(o, gpu)
    y = _nan_e4m3((B, 56, 56, 256), gpu)
    out = ops.bottleneck56(_codes(o["x"], gpu), w1q, a1, o["b1"].float().to(gpu), _pack(o["w2"], gpu),
                           o["b2"].float().to(gpu), _pack(o["w3"], gpu), o["b3"].float().to(gpu), o["res_scale"],
                           o["out_scale"], out=y)
    assert out.data_ptr() == y.data_ptr()
    torch.cuda.synchronize()
    return kb.nchw(y.cpu())


@pytest.mark.parametrize("B", [1, 3])
def test_bottleneck56_exact(gpu, B):
    """Integer operands, every intermediate exact: the output bytes equal the
    float64 value rounded to e4m3 (test_kernel_bar_cpu.py asserts the
    exactness conditions and that every control changes a byte)."""
    o = kb.bottleneck_exact_operands(B)
    want = kb.e4m3_bytes(kb.bottleneck_ref(o, bar=False)[0])
    got = _run_bottleneck(o, gpu).view(torch.uint8)
    bad = int((got != want).sum())
    print(f"bottleneck56 exact B={B}: {bad} of {want.numel()} bytes differ")
    assert torch.equal(got, want), f"{bad} bytes differ, first at {(got != want).nonzero()[:4].tolist()}"


def test_bottleneck56_pack_fp8_is_the_reference_quantiser(gpu):
    """kb.e4m3_weights (the operands' conv1 codes and scales) is
    ops.pack_conv_weight_fp8's rule."""
    w = torch.randn(64, 256, 1, 1, generator=torch.Generator().manual_seed(9)) / 32
    q, s = ops.pack_conv_weight_fp8(w)
    codes, s_ref = kb.e4m3_weights(w)
    assert torch.equal(q.double(), codes.reshape(64, 256)) and torch.equal(s, s_ref)


def test_bottleneck56(gpu):
    """Random operands at B = 2 with an output scale that is no power of two,
    under kb.chain's three-stage bar; the reference models the kernel's
    bf16(fp32(w3) fp32(1 / s_y)) weights (kernels.h)."""
    o = kb.bottleneck_operands(2, seed=156)
    ref, bnd, _, _ = kb.bottleneck_ref(o)
    y = _run_bottleneck(o, gpu).double()
    kb.assert_close(y, torch.relu(ref), bnd, "bottleneck56", l2=4e-2)
    for name, wrong in kb.bottleneck_controls(o, RING):
        kb.assert_rejects(y, torch.relu(wrong), bnd, f"bottleneck56 [{name}]")


# ---------------------------------------------------------------- bottleneck56_head
def _run_head(o, gpu):
    B = o["x"].shape[0]
    y = _nan_bf16((B, 56, 56, 64), gpu)
    ops.bottleneck56_head(_bf16(o["x"], gpu), _pack(o["w1"], gpu), o["b1"].float().to(gpu), _pack(o["w2"], gpu),
                          o["b2"].float().to(gpu), out=y)
    torch.cuda.synchronize()
    return kb.nchw(y.cpu()).double()


@pytest.mark.parametrize("B", [1, 3])
def test_bottleneck56_head_exact(gpu, B):
    o = kb.head_exact_operands(B)
    want = torch.relu(kb.head_ref(o)[0])
    got = _run_head(o, gpu)
    bad = int((got != want).sum())
    print(f"bottleneck56_head exact B={B}: {bad} of {want.numel()} values differ")
    assert torch.equal(got, want), f"{bad} values differ, first at {(got != want).nonzero()[:4].tolist()}"


def test_bottleneck56_head(gpu):
    o = kb.head_operands(2, seed=157)
    ref, bnd, _, _ = kb.head_ref(o)
    y = _run_head(o, gpu)
    kb.assert_close(y, torch.relu(ref), bnd, "bottleneck56_head")
    for name, wrong in kb.head_controls(o, RING):
        kb.assert_rejects(y, torch.relu(wrong), bnd, f"bottleneck56_head [{name}]")


# ---------------------------------------------------------------- conv1x1: the block loop
def _c1_launch(o, gpu, num_cus):
    """One CONV_1X1 launch on a NaN-filled output: [M, N] float64 in the output's units."""
    in8, out8 = o["in8"], o["out8"]
    to = (lambda t: t.float().to(FP8).to(gpu)) if in8 else (lambda t: t.bfloat16().to(gpu))
    x, w = to(o["x"]), to(o["w"])
    x2 = None if o["x2"] is None else o["x2"].bfloat16().to(gpu)
    B, N, s = x.shape[0], o["N"], o["stride"]
    Ho, Wo = x.shape[1] // s, x.shape[2] // s
    res = None
    if o["r"] is not None:
        res = (o["r"].float().to(FP8) if out8 else o["r"].bfloat16()).to(gpu).view(B, Ho, Wo, N)
    y = (_nan_e4m3 if out8 else _nan_bf16)((B, Ho, Wo, N), gpu)
    tile = dmlc.native().CONV_1X1
    bias = o["bias"].float().to(gpu)
    if in8 or out8:
        ops.conv2d_fp8(x, w, None if o["alpha"] is None else o["alpha"].float().to(gpu), N, 1, 1, s, 0, bias=bias,
                       res=res, res_scale=o["res_scale"], relu=True, out_scale=o["out_scale"], tile=tile, out=y,
                       num_cus=num_cus, x2=x2)
    else:
        ops.conv2d(x, w, N, 1, 1, s, 0, bias=bias, res=res, relu=True, tile=tile, out=y, num_cus=num_cus, x2=x2)
    torch.cuda.synchronize()
    return y.cpu().double().reshape(-1, N), y.cpu().view(torch.uint8 if out8 else torch.int16)


def _c1_check(o, gpu, what, controls):
    v, mag = kb.c1_ref(o)
    want, bnd, l2 = kb.c1_bar(o, v, mag)
    full, full_bits = _c1_launch(o, gpu, 0)
    for nc in (8, 4):  # block stride 8 for the 8-wave forms at both, for the 4-wave forms at 4 (stride 16 at 8)
        y, bits = _c1_launch(o, gpu, nc)
        kb.assert_close(y, want, bnd, f"{what} num_cus={nc}", l2=l2)
        assert torch.equal(bits, full_bits), f"{what}: num_cus={nc} and the device's grid differ in bits"
    for name, wrong in controls:
        kb.assert_rejects(full, kb.c1_bar(o, wrong, mag)[0], bnd, f"{what} [{name}]")


@pytest.mark.parametrize("form", kb.c1_forms(), ids=lambda f: "in8=%d-out8=%d-res=%d-s%d-rb%d" % f)
def test_conv1x1_block_loop(gpu, form):
    """43 blocks on 8 workgroups per channel slice: 6 or 5 blocks each."""
    o = kb.c1_operands(43, *form, seed=300 + kb.c1_forms().index(form))
    controls = kb.c1_controls(o)
    assert len(controls) == (2 if form[2] else 1)
    _c1_check(o, gpu, f"conv1x1 {form}", controls)


@pytest.mark.parametrize("nblocks", [1, 8, 9, 17])
@pytest.mark.parametrize("form", [(True, True, True, 1, 256), (False, False, True, 1, 256)],
                         ids=["e4m3", "bf16"])
def test_conv1x1_block_counts(gpu, form, nblocks):
    """Fewer blocks than workgroups, one each, one workgroup with two, and
    workgroups with three and two (S = 3: the ring's first wrap)."""
    o = kb.c1_operands(nblocks, *form, seed=340 + nblocks)
    _c1_check(o, gpu, f"conv1x1 {form} {nblocks} blocks", kb.c1_controls(o))


@pytest.mark.parametrize("nblocks", [43, 1])
def test_conv1x1_concat_k(gpu, nblocks):
    """K = 64 channels of x then 64 of x2 (layer1.0's downsample folded into
    the expand conv) against one conv over [x | x2] with [W3 | Wd]."""
    o = kb.c1_operands(nblocks, False, False, False, 1, 256, seed=350 + nblocks, cin2=64)
    _c1_check(o, gpu, f"conv1x1 concat K {nblocks} blocks", kb.c1_cat_controls(o, 64) + kb.c1_controls(o))


def test_conv2d_second_input_needs_conv1x1(gpu):
    x = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device=gpu)
    w = torch.zeros(256, 128, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError):
        ops.conv2d(x, w, 256, 1, 1, x2=x)


# ---------------------------------------------------------------- conv1x1_chain
@pytest.mark.parametrize("nblocks", [1, 9, 43])
def test_conv1x1_chain(gpu, nblocks):
    """y under the e4m3 bar; y2 against the float64 reduce of the kernel's own
    y codes (an exact input); both bit-equal to two CONV_1X1 launches. The NaN
    fill catches a skipped last-block reduce."""
    o = kb.chain_operands(nblocks, seed=360 + nblocks)
    f8 = lambda t: t.float().to(FP8).to(gpu)  # noqa: E731
    x, res = f8(o["x"]), f8(o["r"]).view(nblocks, 8, 8, 512)
    w, w2 = f8(o["w"]), f8(o["w2"])
    al, bs = o["alpha"].float().to(gpu), o["bias"].float().to(gpu)
    al2, bs2 = o["alpha2"].float().to(gpu), o["bias2"].float().to(gpu)
    y, y2 = _nan_e4m3((nblocks, 8, 8, 512), gpu), _nan_e4m3((nblocks, 8, 8, 128), gpu)
    ops.conv1x1_chain(x, w, al, bs, res, o["res_scale"], o["out_scale"], w2, al2, bs2, o["out_scale2"], num_cus=8,
                      out=y, out2=y2)
    tile = dmlc.native().CONV_1X1
    ys = ops.conv2d_fp8(x, w, al, 512, 1, 1, bias=bs, res=res, res_scale=o["res_scale"], relu=True,
                        out_scale=o["out_scale"], tile=tile, out=_nan_e4m3((nblocks, 8, 8, 512), gpu), num_cus=8)
    y2s = ops.conv2d_fp8(ys, w2, al2, 128, 1, 1, bias=bs2, relu=True, out_scale=o["out_scale2"], tile=tile,
                         out=_nan_e4m3((nblocks, 8, 8, 128), gpu), num_cus=8)
    torch.cuda.synchronize()
    what = f"conv1x1_chain {nblocks} blocks"
    yc, y2c = y.cpu().double().reshape(-1, 512), y2.cpu().double().reshape(-1, 128)
    v, mag = kb.c1_ref(o)
    want, bnd, l2 = kb.c1_bar(o, v, mag)
    kb.assert_close(yc, want, bnd, what + " y", l2=l2)
    want2, bnd2 = kb.chain_reduce_bar(o, yc)
    kb.assert_close(y2c, want2, bnd2, what + " y2", l2=l2)
    assert torch.equal(y.cpu().view(torch.uint8), ys.cpu().view(torch.uint8)), what + ": y differs from conv1x1's"
    assert torch.equal(y2.cpu().view(torch.uint8), y2s.cpu().view(torch.uint8)), what + ": y2 differs from conv1x1's"
    inv2 = kb.f32(1.0 / o["out_scale2"])
    controls = kb.chain_controls(o, yc)
    assert len(controls) == (1 if nblocks > 8 else 0)
    for name, wrong in controls:
        kb.assert_rejects(y2c, torch.relu(wrong) * inv2, bnd2, f"{what} [{name}]")
    for name, wrong in kb.c1_controls(o):
        kb.assert_rejects(yc, kb.c1_bar(o, wrong, mag)[0], bnd, f"{what} y [{name}]")

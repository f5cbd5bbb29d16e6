"""The op tests' bar (tests/_kernel_bar.py) on the CPU: the float64 reference
rounded to bf16 (what a correct kernel may return at worst, to first order)
passes against itself, and each modelled kernel fault is rejected."""
import math

import pytest
import torch
import torch.nn.functional as F

import _kernel_bar as kb


def _conv_case(B, Cin, Cout, H, k, pad, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, H, generator=g).bfloat16().double()
    w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).bfloat16().double()
    bias = (torch.randn(Cout, generator=g) * 0.1).double()
    return x, w, bias


@pytest.mark.parametrize("Cin,Cout,H,k,pad", [(192, 384, 13, 3, 1), (64, 192, 27, 5, 2)])
@pytest.mark.parametrize("relu", [False, True])
def test_conv_bar_and_controls(Cin, Cout, H, k, pad, relu):
    x, w, bias = _conv_case(2, Cin, Cout, H, k, pad)
    ref, mag = kb.conv_ref(x, w, bias, 1, pad)
    act = torch.relu if relu else (lambda t: t)
    bnd = kb.bound(act(ref), mag, k * k * Cin)
    got = kb.bf16r(act(ref))
    kb.assert_close(got, act(ref), bnd, "clean")
    for name, wrong in (("border", kb.fault_border_taps(ref, x, w, pad)), ("swap", kb.fault_chunk_swap(ref)),
                        ("batch", kb.fault_batch_shift(ref))):
        kb.assert_rejects(kb.bf16r(act(wrong)), act(ref), bnd, name)
        kb.assert_rejects(got, act(wrong), bnd, name + " (as the reference)")


def test_pooled_bar_and_controls():
    x, w, bias = _conv_case(2, 256, 256, 13, 3, 1, seed=1)
    ref, mag = kb.conv_ref(x, w, bias, 1, 1)
    r = torch.relu(ref)
    bnd = kb.maxpool(kb.bound(r, mag, 9 * 256))
    pref = kb.maxpool(r)
    assert pref.shape == (2, 256, 6, 6)
    # what a kernel computes: an fp32 conv, rounded to bf16, pooled
    got = kb.maxpool(kb.bf16r(torch.relu(torch.nn.functional.conv2d(x.float(), w.float(), bias.float(), 1, 1))))
    kb.assert_close_pooled(got, r, kb.bound(r, mag, 9 * 256), "clean")
    # faults on pixels that the 6x6 pooling windows cover (rows / columns 0..12)
    for name, wrong in (("border", kb.fault_border_taps(ref, x, w, 1)), ("swap", kb.fault_chunk_swap_at_max(ref)),
                        ("batch", kb.fault_batch_shift(ref))):
        kb.assert_rejects(got, kb.maxpool(torch.relu(wrong)), bnd, name)


def test_fc_bar_and_controls():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 4128, generator=g).bfloat16().double()
    w = (torch.randn(1000, 4128, generator=g) / 4128 ** 0.5).bfloat16().double()
    bias = (torch.randn(1000, generator=g) * 0.1).double()
    ref, mag = kb.fc_ref(x, w, bias)
    kb.assert_close(kb.bf16r(ref), ref, kb.bound(ref, mag, 4128), "bf16")
    kb.assert_close(ref.float(), ref, kb.bound(ref, mag, 4128, out_bf16=False), "fp32", l2=1e-6)
    kb.assert_rejects(kb.bf16r(kb.fault_batch_shift(ref)), ref, kb.bound(ref, mag, 4128), "batch")
    # one wave's K range (1/8 of K) left out of the sum
    short, _ = kb.fc_ref(x[:, 516:], w[:, 516:], bias)
    kb.assert_rejects(kb.bf16r(short), ref, kb.bound(ref, mag, 4128), "k range")


def test_head_bar_and_controls():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 49, 512, generator=g).bfloat16().double()
    w = (torch.randn(1000, 512, generator=g) / 512 ** 0.5).bfloat16().double()
    bias = (torch.randn(1000, generator=g) * 0.1).double()
    ref, _ = kb.fc_ref(x.mean(1), w, bias)
    _, mag = kb.fc_ref(x.abs().mean(1), w, bias)
    bnd = kb.head_bound(mag, 512)
    got, _ = kb.fc_ref(kb.bf16r(x.mean(1)), w, bias)  # the kernel's rounding point
    kb.assert_close(got.float(), ref, bnd, "clean")
    kb.assert_rejects(kb.fault_batch_shift(got).float(), ref, bnd, "batch")
    # a class split left out of the softmax sum moves the top-1 probability past rtol 1e-4
    z = got.float()
    p = torch.softmax(z, -1).max(-1).values
    lo = 0 if int(z.argmax(-1).min()) >= 63 * 4 else 63 * 8
    bad = kb.prob_without_split(z, lo, lo + 63 * 4).float()
    assert torch.allclose(p, torch.softmax(z.double(), -1).max(-1).values.float(), rtol=1e-4, atol=1e-6)
    assert not torch.allclose(p, bad, rtol=1e-4, atol=1e-6)


def test_avgpool_bar_and_control():
    x, w, bias = _conv_case(3, 512, 512, 7, 3, 1, seed=4)
    ref, mag = kb.conv_ref(x, w, bias, 1, 1)
    y = kb.nhwc(torch.relu(ref)).reshape(3, 49, 512)
    yb = kb.nhwc(kb.bound(torch.relu(ref), mag, 9 * 512)).reshape(3, 49, 512)
    bnd = kb.avgpool_bound(y, yb)
    got = kb.bf16r(kb.bf16r(y).mean(1))  # the kernel's rounding points
    kb.assert_close(got, y.mean(1), bnd, "clean")
    wrong = kb.nhwc(torch.relu(kb.fault_border_taps(ref, x, w, 1))).reshape(3, 49, 512)
    kb.assert_rejects(got, wrong.mean(1), bnd, "border")
    kb.assert_rejects(got, y[:, :48].sum(1) / 49, bnd, "last pixel left out")


def test_padded_pool_bar_and_controls():
    """The ResNet stem's pool (3x3/s2/p1) after a 7x7/s2/p3 conv + ReLU: -inf
    and zero padding agree, an fp32 conv rounded to bf16 and pooled passes,
    the faults do not."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 64, 64, generator=g).bfloat16().double()
    w = (torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5).bfloat16().double()
    bias = (torch.randn(64, generator=g) * 0.1).double()
    ref, mag = kb.conv_ref(x, w, bias, 2, 3)
    r = torch.relu(ref)
    assert torch.equal(kb.maxpool(r, pad=1), F.max_pool2d(F.pad(r, (1, 1, 1, 1)), 3, 2))
    cb = kb.bound(r, mag, 147)
    got = kb.maxpool(kb.bf16r(torch.relu(F.conv2d(x.float(), w.float(), bias.float(), 2, 3))), pad=1)
    assert got.shape == (2, 64, 16, 16)
    kb.assert_close_pooled(got, r, cb, "clean", pad=1)
    lost = F.conv2d(x[:, :, 0:1, :], w[:, :, 1:2, :], None, (1, 2), (0, 3))  # conv row 1 loses its taps on image row 0
    wrong = ref.clone()
    wrong[:, :, 1:2, :] -= lost
    for name, wr in (("border", wrong), ("swap", kb.fault_chunk_swap_at_max(ref)), ("batch", kb.fault_batch_shift(ref))):
        kb.assert_rejects(got, kb.maxpool(torch.relu(wr), pad=1), kb.maxpool(cb, pad=1), name)


def _block_fp32(x, w1, b1, w2, b2):
    """The block as a kernel computes it: fp32 convs, a bf16 intermediate, a
    bf16 output."""
    t = torch.relu(F.conv2d(x.float(), w1.float(), b1.float(), 1, 1)).bfloat16().float()
    return kb.bf16r(torch.relu(F.conv2d(t, w2.float(), b2.float(), 1, 1) + x.float()))


def test_chained_bar_and_controls():
    ring = kb.kernel_const("conv3x3_block.hip", "kRing")
    ops5 = kb.block_operands(2, seed=6)
    ref, bnd, delta, _ = kb.chained(*ops5)
    got = _block_fp32(*ops5)
    kb.assert_close(got, torch.relu(ref), bnd, "clean")
    assert 0 < (delta > 0).double().mean().item() < 0.5  # the intermediate is known exactly on most elements
    for name, wrong in kb.block_controls(*ops5, ring):
        kb.assert_rejects(got, torch.relu(wrong), bnd, name)


@pytest.mark.parametrize("B", [1, 3])
def test_chained_bar_is_not_swamped(B):
    """A condition on the GPU test's own operands (test_kernels_resnet_gpu.py,
    seed 130 + B): the delta term leaves every control above the bar."""
    ring = kb.kernel_const("conv3x3_block.hip", "kRing")
    ops5 = kb.block_operands(B, seed=130 + B)
    ref, bnd, delta, _ = kb.chained(*ops5)
    share = (F.conv2d(delta, ops5[3].abs(), None, 1, 1) / bnd).max().item()
    got = _block_fp32(*ops5)
    ratios = [kb.worst(got, torch.relu(wrong), bnd)[0] for _, wrong in kb.block_controls(*ops5, ring)]
    print(f"block B={B}: delta term at most {share:.2f} of the bar, smallest control ratio {min(ratios):.1f}")
    assert min(ratios) > 1.0, ratios


def test_e4m3_bar_and_controls():
    x, w, bias = _conv_case(2, 128, 128, 28, 3, 1, seed=7)
    ref, mag = kb.conv_ref(x, w, bias, 1, 1)
    r = torch.relu(ref)
    inv = 400.0 / r.max().item()
    bnd = kb.e4m3_bound(r, mag, 1152, inv)
    q = lambda t: (t * inv).float().to(torch.float8_e4m3fn).double()
    got = q(torch.relu(F.conv2d(x.float(), w.float(), bias.float(), 1, 1)).double())
    assert bool(((r * inv > 0) & (r * inv < 2.0 ** -6)).any()), "no value in the subnormal range"
    ratio, _ = kb.assert_close(got, r * inv, bnd, "clean", l2=4e-2)
    assert ratio > 0.5  # the bar is e4m3's own roundoff, not a loose multiple of it
    for name, wrong in (("border", kb.fault_border_taps(ref, x, w, 1)), ("swap", kb.fault_chunk_swap(ref)),
                        ("batch", kb.fault_batch_shift(ref)),
                        ("ring", kb.fault_ring_row(ref, x, w, 9, kb.kernel_const("conv3x3_rows28.hip", "kRing")))):
        kb.assert_rejects(got, torch.relu(wrong) * inv, bnd, name)
    with pytest.raises(AssertionError):
        kb.e4m3_bound(r, mag, 1152, 500.0 / r.max().item())


def test_strided_and_downsample_faults():
    """fault_ring_row and fault_strided_parity on a stride-2 conv, and
    fault_ds_missing / fault_strided_parity on a conv that takes the 1x1/s2
    downsample as extra K steps: the clean result passes, each fault does not."""
    g = torch.Generator().manual_seed(8)
    x56 = torch.randn(2, 64, 56, 56, generator=g).bfloat16().double()
    w = (torch.randn(128, 64, 3, 3, generator=g) / 24).bfloat16().double()
    bias = (torch.randn(128, generator=g) * 0.1).double()
    ref, mag = kb.conv_ref(x56, w, bias, 2, 1)
    bnd = kb.bound(torch.relu(ref), mag, 576)
    got = kb.bf16r(torch.relu(ref))
    kb.assert_close(got, torch.relu(ref), bnd, "s2 clean")
    ring = kb.kernel_const("conv3x3_s2rows.hip", "kRing")
    wrong = kb.fault_ring_row(ref, x56, w, 9, ring, stride=2)
    assert torch.equal(wrong[:, :, :9], ref[:, :, :9]) and torch.equal(wrong[:, :, 10:], ref[:, :, 10:])
    kb.assert_rejects(got, torch.relu(wrong), bnd, "ring row")
    wrong = kb.fault_strided_parity(ref, x56, w, 13, 1)
    shifted = F.conv2d(torch.roll(x56, -1, 3), w, bias, 2, 1)  # (column 13's taps stay clear of the wrapped column)
    assert torch.allclose(wrong[..., 13], shifted[..., 13], rtol=0, atol=1e-12)
    assert torch.equal(wrong[..., :13], ref[..., :13])
    kb.assert_rejects(got, torch.relu(wrong), bnd, "parity")
    # the block's conv2 with the downsample as 2 more K steps
    x, w2, b2 = _conv_case(2, 128, 128, 28, 3, 1, seed=9)
    wd = (torch.randn(128, 64, 1, 1, generator=g) / 8).bfloat16().double()
    bd = (torch.randn(128, generator=g) * 0.1).double()
    c, cm = kb.conv_ref(x, w2, b2, 1, 1)
    d, dm = kb.conv_ref(x56, wd, bd, 2, 0)
    ref, mag = c + d, cm + dm
    bnd = kb.bound(torch.relu(ref), mag, 1216)
    got = kb.bf16r(torch.relu(ref))
    kb.assert_close(got, torch.relu(ref), bnd, "conv + downsample clean")
    kb.assert_rejects(got, torch.relu(kb.fault_ds_missing(ref, x56, wd, b=1, frag=48)), bnd, "ds missing")
    kb.assert_rejects(got, torch.relu(kb.fault_strided_parity(ref, x56, wd, 27, 0)), bnd, "ds parity")


# ---------------------------------------------------------------- bottleneck56 / bottleneck56_head (kb.chain)
BN_RING = kb.kernel_const("bottleneck56.hip", "kRing")


def _bottleneck_fp32(o):
    """bottleneck56 as the kernel computes it: fp32 convs, bf16 t1 / t2,
    the last stage in the output's units (kb.bottleneck_last), e4m3 out."""
    w3s, b3s, res = kb.bottleneck_last(o)
    a1, b1 = o["a1"].float().view(1, -1, 1, 1), o["b1"].float().view(1, -1, 1, 1)
    t1 = torch.relu(F.conv2d(o["x"].float(), o["w1"].float()) * a1 + b1).bfloat16().float()
    t2 = torch.relu(F.conv2d(t1, o["w2"].float(), o["b2"].float(), 1, 1)).bfloat16().float()
    v = F.conv2d(t2, w3s.float(), b3s.float()) + res.float()
    return v.clamp(0, 448).to(torch.float8_e4m3fn).double()


def _head_fp32(o):
    t1 = torch.relu(F.conv2d(o["x"].float(), o["w1"].float(), o["b1"].float())).bfloat16().float()
    return kb.bf16r(torch.relu(F.conv2d(t1, o["w2"].float(), o["b2"].float(), 1, 1)))


def test_chain_is_chained():
    """kb.chained is the two-stage case of kb.chain, and a one-stage chain is
    the plain bar."""
    ops5 = kb.block_operands(1, seed=6)
    x, w1, b1, w2, b2 = ops5
    ref, bnd, delta, t = kb.chained(*ops5)
    r2, b2_, deltas, ts = kb.chain(x, [(w1, b1, 576, 1), (w2, b2, 576, 1)], res=x)
    assert torch.equal(ref, r2) and torch.equal(bnd, b2_) and torch.equal(delta, deltas[0]) and torch.equal(t, ts[0])
    v, mag = kb.conv_ref(x, w1, b1, 1, 1)
    r1, b1_, d1, t1 = kb.chain(x, [(w1, b1, 576, 1)])
    assert torch.equal(r1, v) and torch.equal(b1_, kb.bound(torch.relu(v), mag, 576)) and d1 == [] and t1 == []


def test_bottleneck_bar_and_controls():
    """The GPU bar test's own operands (test_kernels_resnet50_gpu.py: B = 2,
    seed 156): the fp32 model passes, no control is swamped by the delta
    terms, and the output scale is no power of two."""
    o = kb.bottleneck_operands(2, seed=156)
    inv = 1.0 / o["out_scale"]
    assert torch.frexp(torch.tensor(inv, dtype=torch.float64))[0].item() != 0.5
    w3s, _, _ = kb.bottleneck_last(o)
    assert not torch.equal(w3s, o["w3"] * kb.f32(inv))  # the re-rounding of w3 / s_y is visible
    ref, bnd, deltas, _ = kb.bottleneck_ref(o)
    got = _bottleneck_fp32(o)
    ratio, _ = kb.assert_close(got, torch.relu(ref), bnd, "bottleneck56 model", l2=4e-2)
    share = (F.conv2d(deltas[1], w3s.abs()) / bnd).max().item()
    ratios = [kb.worst(got, torch.relu(w), bnd)[0] for _, w in kb.bottleneck_controls(o, BN_RING)]
    print(f"bottleneck56: delta term at most {share:.2f} of the bar, smallest control ratio {min(ratios):.1f}")
    assert min(ratios) > 1.0, ratios
    # without the model of the re-rounded weights the reference itself is off by more than the summation slack
    plain = kb.conv_ref(kb.bf16r(torch.relu(kb.conv_ref(kb.bottleneck_ref(o)[3][0], o["w2"], o["b2"], 1, 1)[0])),
                        o["w3"] * inv, o["b3"] * inv, 1, 0, res=o["x"] * o["res_scale"] * inv)[0]
    assert (plain - ref).abs().max().item() > 64 * kb.EPS_SUM * 400


def test_bottleneck_head_bar_and_controls():
    o = kb.head_operands(2, seed=157)
    ref, bnd, deltas, _ = kb.head_ref(o)
    got = _head_fp32(o)
    kb.assert_close(got, torch.relu(ref), bnd, "bottleneck56_head model")
    share = (F.conv2d(deltas[0], o["w2"].abs(), None, 1, 1) / bnd).max().item()
    ratios = [kb.worst(got, torch.relu(w), bnd)[0] for _, w in kb.head_controls(o, BN_RING)]
    print(f"bottleneck56_head: delta term at most {share:.2f} of the bar, smallest control ratio {min(ratios):.1f}")
    assert min(ratios) > 1.0, ratios


@pytest.mark.parametrize("B", [1, 3])
def test_bottleneck_exact_operands(B):
    """The exact-integer test's conditions, on the reference alone: both
    intermediates are integers that bf16 holds, every weight tap and input
    channel is used, the output has negatives, grid ties and a few values
    past 448, and every control changes at least one expected byte."""
    o = kb.bottleneck_exact_operands(B)
    ref, _, _, (t1, t2) = kb.bottleneck_ref(o, bar=False)
    for t in (t1, t2):
        assert torch.equal(kb.bf16r(t), t) and torch.equal(t, t.round()) and float(t.max()) <= 256
    w3s, b3s, _ = kb.bottleneck_last(o)
    assert torch.equal(w3s, o["w3"] / o["out_scale"]) and torch.equal(ref.float().double(), ref)
    assert float(o["b1"].max()) >= 4 and len(set(o["a1"].tolist())) == 3
    assert bool((o["x"] != 0).all())
    for w in (o["w1"], o["w2"], o["w3"]):
        assert bool((w.abs().sum((0, 2, 3)) > 0).all()) and bool((w.abs().sum((0, 1)) > 0).all())
        assert bool((w.abs().sum((1, 2, 3)) > 0).all()) and torch.equal(w, w.round())
    over = int((ref > 448).sum())
    assert bool((ref < 0).any()) and 0 < over < ref.numel() // 100
    assert bool((ref[(ref > 16) & (ref < 32)] % 2 == 1).any())  # ties of the e4m3 grid (step 2 in [16, 32))
    want = kb.e4m3_bytes(ref)
    for name, wrong in kb.bottleneck_controls(o, BN_RING):
        assert not torch.equal(kb.e4m3_bytes(wrong), want), name


@pytest.mark.parametrize("B", [1, 3])
def test_head_exact_operands(B):
    o = kb.head_exact_operands(B)
    ref, _, _, (t1,) = kb.head_ref(o)
    t2 = torch.relu(ref)
    for t in (t1, t2):
        assert torch.equal(kb.bf16r(t), t) and torch.equal(t, t.round()) and float(t.max()) <= 256
    assert bool((ref < 0).any()) and float(o["b1"].max()) >= 4
    for w in (o["w1"], o["w2"]):
        assert bool((w.abs().sum((0, 2, 3)) > 0).all()) and bool((w.abs().sum((0, 1)) > 0).all())
        assert bool((w.abs().sum((1, 2, 3)) > 0).all())
    for name, wrong in kb.head_controls(o, BN_RING):
        assert not torch.equal(torch.relu(wrong), t2), name


@pytest.mark.parametrize("form", [(True, True, True, 1, 128), (False, False, True, 1, 512), (True, False, False, 1, 1024),
                                  (False, True, False, 1, 256), (True, True, False, 2, 256)])
def test_conv1x1_block_loop_controls(form):
    """conv1x1's block-loop controls on the GPU test's operands (43 blocks):
    the reference rounded as the kernel rounds passes, a stale stage slot and
    the other register set's residual do not."""
    o = kb.c1_operands(43, *form, seed=300 + kb.c1_forms().index(form))
    v, mag = kb.c1_ref(o)
    want, bnd, l2 = kb.c1_bar(o, v, mag)
    got = want.float().to(torch.float8_e4m3fn).double() if o["out8"] else kb.bf16r(want)
    kb.assert_close(got, want, bnd, "clean", l2=l2)
    controls = kb.c1_controls(o)
    assert len(controls) == (2 if form[2] else 1)
    for name, wrong in controls:
        kb.assert_rejects(got, kb.c1_bar(o, wrong, mag)[0], bnd, name)


def test_conv1x1_chain_and_concat_controls():
    o = kb.chain_operands(43, seed=360 + 43)
    v, mag = kb.c1_ref(o)
    want, bnd, _ = kb.c1_bar(o, v, mag)
    y = want.float().to(torch.float8_e4m3fn).double()
    want2, bnd2 = kb.chain_reduce_bar(o, y)
    y2 = want2.float().to(torch.float8_e4m3fn).double()
    kb.assert_close(y2, want2, bnd2, "chain y2", l2=4e-2)
    for name, wrong in kb.chain_controls(o, y):
        kb.assert_rejects(y2, torch.relu(wrong) * kb.f32(1.0 / o["out_scale2"]), bnd2, name)
    o = kb.c1_operands(43, False, False, False, 1, 256, seed=350 + 43, cin2=64)
    v, mag = kb.c1_ref(o)
    want, bnd, _ = kb.c1_bar(o, v, mag)
    for name, wrong in kb.c1_cat_controls(o, 64):
        kb.assert_rejects(kb.bf16r(want), torch.relu(wrong), bnd, name)


# ---------------------------------------------------------------- the general matrix family (test_kernels_gemm_gpu.py)
def _gemm_bar_and_controls(o, controls, out_f32=False, need=()):
    """The float64 reference rounded to the output type meets the bar against
    the true reference and misses it against every faulty one."""
    v, mag = o["ref"]
    want, bnd, l2 = kb.gemm_bar(o, v, mag, out_f32)
    got = kb.gemm_rounded(o, v, out_f32)
    kb.assert_close(got, want, bnd, "rounded reference", l2=l2)
    names = [n for n, _ in controls]
    assert all(n in names for n in need), (names, need)
    for name, wrong in controls:
        kb.assert_rejects(got, kb.gemm_bar(o, wrong, mag, out_f32)[0], bnd, name)


def _distinct(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


_IGEMM_DISTINCT = _distinct(kb.IGEMM_CASES, lambda c: (c[1], c[2], kb.GEMM_TILES[c[3]], c[4], c[6]))


@pytest.mark.parametrize("case", _IGEMM_DISTINCT, ids=[c[0] for c in _IGEMM_DISTINCT])
def test_igemm_bar_and_controls(case):
    name, shape, res, tile, split_k, max_blocks, out_f32 = case
    o = kb.gemm_case_operands(shape, res, kb.case_seed(kb.IGEMM_CASES, name))
    slices = kb.igemm_slices(o["K"] // 64, split_k)
    M = shape[0] * o["ref"][0].shape[2] * o["ref"][0].shape[3]
    need = ["chunk swap", "K tile missing"] + (["slice missing"] if split_k > 1 else ["batch shift", "tail tile"])
    if shape[4] == 100:
        need.append("pad columns")
    assert split_k > 1 or M % kb.GEMM_TILES[tile][0]
    _gemm_bar_and_controls(o, kb.gemm_controls(o, *kb.GEMM_TILES[tile], slices), out_f32, need)


def test_igemm_slices():
    """conv2d_igemm's slice ranges: which split_k reaches which loop of the reduce."""
    assert [len(kb.igemm_slices(72, s)) for s in (2, 5, 13, 15, 32)] == [2, 5, 12, 15, 24]
    assert kb.igemm_slices(72, 5)[-1] == (60, 72) and kb.igemm_slices(72, 15)[-1] == (70, 72)
    assert kb.bigtile_slices(18, 5) == [(0, 3), (3, 7), (7, 10), (10, 14), (14, 18)]
    for n in (64, 100, 192, 256, 1000):
        assert kb.npad(n) == {64: 64, 100: 128, 192: 192, 256: 256, 1000: 1024}[n]


@pytest.mark.parametrize("k,s,p", kb.STEM_CASES)
def test_stem_bar_and_controls(k, s, p):
    o = kb.gemm_operands(2, *kb.STEM_HW, 3, 64, k, s, p, seed=490 + k)
    _gemm_bar_and_controls(o, kb.gemm_controls(o, 256, 64), need=["chunk swap", "batch shift", "tail tile"])


@pytest.mark.parametrize("case", kb.E4M3_CASES, ids=[c[0] for c in kb.E4M3_CASES])
def test_igemm_e4m3_bar_and_controls(case):
    name, shape, in8, out8, res, tile = case[:6]
    o = kb.gemm_case_operands(shape, res, kb.case_seed(kb.E4M3_CASES, name), in8=in8, out8=out8)
    bm, bn = (256, 64) if tile == 1 else (128, 128)
    if out8:
        top = float((torch.relu(o["ref"][0]) * kb.f32(1.0 / o["out_scale"])).max())
        assert abs(top - 400.0) < 1e-3 and o["out_scale"] != 2.0 ** round(math.log2(o["out_scale"]))
    _gemm_bar_and_controls(o, kb.gemm_controls(o, bm, bn),
                           need=["chunk swap", "batch shift", "tail tile", "K tile missing"])


@pytest.mark.parametrize("case", kb.BIGTILE_CASES, ids=[c[0] for c in kb.BIGTILE_CASES])
def test_bigtile_bar_and_controls(case):
    name, shape, res, tile, n = case
    o = kb.gemm_case_operands(shape, res, kb.case_seed(kb.BIGTILE_CASES, name))
    slices = kb.bigtile_slices(o["K"] // 64, n) if tile != 13 else None
    need = ["chunk swap", "batch shift", "K tile missing"]
    need += ["slice missing"] if tile != 13 and n > 1 else []
    need += ["tail tile"] if "stride 2" not in name else []
    _gemm_bar_and_controls(o, kb.gemm_controls(o, *kb.GEMM_TILES[tile], slices), need=need)


_EXACT = [(c[1], c[2], False, False, kb.case_seed(kb.IGEMM_CASES, c[0])) for c in kb.IGEMM_EXACT] + \
         [(c[1], c[4], c[2], c[3], kb.case_seed(kb.E4M3_CASES, c[0])) for c in kb.E4M3_CASES] + \
         [(c[1], c[2], False, False, kb.case_seed(kb.BIGTILE_CASES, c[0])) for c in kb.BIGTILE_EXACT] + \
         [((2,) + kb.STEM_HW + (3, 64, 7, 2, 3), False, False, False, 497)]
_EXACT = _distinct(_EXACT, lambda c: c)


@pytest.mark.parametrize("case", _EXACT, ids=[str(c) for c in _EXACT])
def test_gemm_exact_operands(case):
    """The exactness conditions of the integer operands: integer values small
    enough that any fp32 partial sum is exact (sum |x| |w| alpha < 2^24),
    outputs exact in bf16 (|v| <= 256) or in the e4m3 units' fp32, and a
    chunk swap, a batch shift and a missing K tile each change the expectation."""
    shape, res, in8, out8, seed = case
    o = kb.gemm_operands(*shape, res=res, seed=seed, exact=True, in8=in8, out8=out8)
    v, mag = o["ref"]
    for t in (o["x"], o["w"], o["bias"]) + (() if o["r"] is None else (o["r"],)):
        assert torch.equal(t, t.round())
    assert float(mag.max()) < 2 ** 24 and float(o["x"].abs().max()) <= 3 and float(o["w"].abs().max()) <= 2
    if out8:
        want = kb.e4m3_bytes(v * kb.f32(1.0 / o["out_scale"]))
        assert int((want == 0x7E).sum()) > 0
        exp = lambda t: kb.e4m3_bytes(t * kb.f32(1.0 / o["out_scale"]))  # noqa: E731
    else:
        assert float(torch.relu(v).max()) <= 256
        exp = torch.relu
    want = exp(v)
    bm, bn = 128, 128
    for name, wrong in kb.gemm_controls(o, bm, bn):
        assert not torch.equal(exp(wrong), want), name


@pytest.mark.parametrize("M,N,K,splits", [(M, N, kb.FC_K, s) for M in kb.FC_MS for N in kb.FC_NS for s in (1, 2, 4)] +
                         [(200, 1000, 512, 2)])
def test_fc_gemm_bar_and_controls(M, N, K, splits):
    o = kb.fc_operands(M, K, N, seed=(600 + M + N) if K == kb.FC_K else 650)
    v, mag = o["ref"]
    controls = kb.fc_controls(o, splits)
    assert len(controls) == 1 + (splits > 1) + (M > 16)
    for out_f32 in (False, True):
        f = (lambda t: t) if out_f32 else torch.relu
        bnd = kb.bound(f(v), mag, K, out_bf16=not out_f32)
        got = f(v).float().double() if out_f32 else kb.bf16r(f(v))
        kb.assert_close(got, f(v), bnd, "rounded reference")
        for name, wrong in controls:
            kb.assert_rejects(got, f(wrong), bnd, name)


def test_fc_exact_operands():
    o = kb.fc_operands(17, kb.FC_K, 1000, seed=660, exact=True)
    v, mag = o["ref"]
    assert torch.equal(v, v.round()) and float(v.abs().max()) <= 256 and float(v.min()) < 0 < float(v.max())
    for name, wrong in kb.fc_controls(o, 4):
        assert not torch.equal(wrong, v), name

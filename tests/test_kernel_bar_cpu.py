"""The op tests' bar (tests/_kernel_bar.py) on the CPU: the float64 reference
rounded to bf16 (what a correct kernel may return at worst, to first order)
passes against itself, and each modelled kernel fault is rejected."""
import pytest
import torch

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

"""conv3x3_stream8's basic-block forms (conv3x3_stream8_block.hip: ResNet18 /
34 layers 3-4 in e4m3) against the float64 result on the same e4m3 operands,
under _kernel_bar's e4m3 bar:

 * RES: 3x3/s1 + residual at 14x14x256 and 7x7x512;
 * WIDE: 3x3/s2 14x14x256 -> 7x7x512, alone and with the block's 1x1/s2
   downsample from the same launch (DS).

B = 1 and B = 3: 7x7x512 and the WIDE forms hold IMG = 2 images per
workgroup, so B = 3 fills one workgroup and leaves the last an image short;
RES at 14x14x256 (IMG = 1) runs three workgroups per channel half.

The kernel's arithmetic (kernels.h): q = fma(acc, alpha inv, bias inv), then
q = fma(res, res_scale inv, q), each factor rounded to fp32 once: two more
roundings of 2^-24 on terms inside mag, well inside the K 2^-23 mag of the bar
(K = 9 CI, or CI for the downsample).

Measured on an MI355X: worst |err| / bar 0.91 (RES), 0.90 (WIDE), 0.94 (the
downsample, K = 256); the controls miss the bar by 14x or more.
"""
import pytest
import torch

import dmlc
from dmlc import ops

from _kernel_bar import (assert_close, assert_rejects, conv_ref, e4m3_bound, e4m3_bytes, e4m3_weights,
                         fault_border_taps_s2, fault_ds_missing)

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
FORMS = {  # (H, CI, CO, stride, res, ds)
    "res14": (14, 256, 256, 1, True, False),
    "res7": (7, 512, 512, 1, True, False),
    "wide_ds": (14, 256, 512, 2, False, True),
    "wide": (14, 256, 512, 2, False, False),
}


@pytest.mark.parametrize("B,exact", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("form", list(FORMS))
def test_stream8_block(gpu, form, B, exact):
    """Random e4m3 codes with scales that are no powers of two (the output
    scales put the largest |reference| at 400 of e4m3's 448) under the e4m3
    bar, with one negative control per form: the residual left out of one
    pixel fragment (RES), the downsample's products left out of one (DS), the
    kh = 1 taps of output row 0 (WIDE).
    exact: sparse power-of-two weights, small integer codes, power-of-two
    scales: every fp32 value inside the kernel is exact, so the output bytes
    are the float64 value rounded to e4m3 (the downsample's operands are
    non-negative: e4m3_bytes applies a ReLU)."""
    H, CI, CO, S, res, ds = FORMS[form]
    Ho = H // S
    g = torch.Generator().manual_seed(1000 * H + 10 * B + exact)
    if exact:
        x = torch.randint(0, 3, (B, CI, H, H), generator=g).double()
        w = torch.randint(-2, 3, (CO, CI, 3, 3), generator=g).double() * (torch.rand(CO, CI, 3, 3, generator=g) < 0.005)
        wd = torch.randint(1, 3, (CO, CI, 1, 1), generator=g).double() * (torch.rand(CO, CI, 1, 1, generator=g) < 0.03)
        alpha, alpha_d = (2.0 ** torch.randint(-1, 2, (2, CO), generator=g)).double()
        bias, bias_d = torch.randint(-8, 9, (CO,), generator=g).double(), torch.randint(0, 9, (CO,), generator=g).double()
        r, res_scale = torch.randint(0, 4, (B, CO, Ho, Ho), generator=g).double(), 4.0
    else:
        xv = torch.rand(B, CI, H, H, generator=g) * 4
        sx = (xv.max() / 448).float()
        x = (xv / sx).clamp(0, 448).to(FP8).double()
        w, sw = e4m3_weights(torch.randn(CO, CI, 3, 3, generator=g) / (9 * CI) ** 0.5)
        wd, sd = e4m3_weights(torch.randn(CO, CI, 1, 1, generator=g) / CI ** 0.5)
        alpha, alpha_d = (sx * sw).float().double(), (sx * sd).float().double()
        bias, bias_d = (torch.randn(2, CO, generator=g) * 0.1).float().double()
        r = (torch.rand(B, CO, Ho, Ho, generator=g) * 300).to(FP8).double()
        res_scale = float(torch.tensor(0.0137, dtype=torch.float32))
    weff, wdeff = w * alpha.view(-1, 1, 1, 1), wd * alpha_d.view(-1, 1, 1, 1)
    rv = r * res_scale if res else None
    ref, mag = conv_ref(x, weff, bias, S, 1, res=rv)
    refd, magd = conv_ref(x, wdeff, bias_d, 2, 0)
    out_scale = 2.0 if exact else float(torch.relu(ref).max()) / 400
    out_scale_d = 2.0 if exact else float(refd.abs().max()) / 400

    extra = {}
    if res:
        extra.update(res=r.permute(0, 2, 3, 1).contiguous().float().to(FP8).to(gpu), res_scale=res_scale)
    if ds:
        extra.update(wd=wd.reshape(CO, CI).float().to(FP8).to(gpu), alpha_d=alpha_d.float().to(gpu),
                     bias_d=bias_d.float().to(gpu), out_scale_d=out_scale_d)
    out = ops.conv3x3_stream8(x.permute(0, 2, 3, 1).contiguous().float().to(FP8).to(gpu),
                              w.permute(0, 2, 3, 1).reshape(CO, 9 * CI).float().to(FP8).to(gpu), alpha.float().to(gpu),
                              bias.float().to(gpu), relu=True, out_scale=out_scale, stride=S, **extra)
    torch.cuda.synchronize()
    y, yd = out if ds else (out, None)
    y = y.cpu().permute(0, 3, 1, 2).contiguous()
    yd = yd.cpu().permute(0, 3, 1, 2).contiguous() if ds else None

    if exact:
        want = e4m3_bytes(ref / out_scale)
        assert torch.equal(y.view(torch.uint8), want), f"{int((y.view(torch.uint8) != want).sum())} bytes differ"
        if ds:
            wantd = e4m3_bytes(refd / out_scale_d)
            assert torch.equal(yd.view(torch.uint8), wantd), f"{int((yd.view(torch.uint8) != wantd).sum())} differ"
        return
    inv = float(torch.tensor(1.0 / out_scale, dtype=torch.float32))
    bnd = e4m3_bound(torch.relu(ref), mag, 9 * CI, inv)
    assert_close(y.double(), torch.relu(ref) * inv, bnd, f"stream8 {form} B={B}", l2=4e-2)
    if res:
        wrong = ref.clone()
        wrong.view(B, CO, -1)[B - 1, :, 16:32] -= rv.view(B, CO, -1)[B - 1, :, 16:32]
    else:
        wrong = fault_border_taps_s2(ref, x, weff)
    assert_rejects(y.double(), torch.relu(wrong) * inv, bnd, f"stream8 {form} B={B} [control]")
    if ds:
        invd = float(torch.tensor(1.0 / out_scale_d, dtype=torch.float32))
        bndd = e4m3_bound(refd, magd, CI, invd)
        assert_close(yd.double(), refd * invd, bndd, f"stream8 {form} B={B} downsample", l2=4e-2)
        wrongd = fault_ds_missing(refd, x, wdeff, b=B - 1, frag=1)
        assert_rejects(yd.double(), wrongd * invd, bndd, f"stream8 {form} B={B} downsample [control]")


def test_stream8_block_rejects(gpu):
    """Unsupported combinations and a residual that overlaps the output raise
    before any launch."""
    C = dmlc.native()
    z = lambda *s: torch.zeros(*s, device=gpu).to(FP8)
    v = lambda n: torch.ones(n, device=gpu)
    with pytest.raises(ValueError):  # a residual at stride 2
        ops.conv3x3_stream8(z(1, 14, 14, 256), z(512, 2304), v(512), v(512), stride=2, res=z(1, 7, 7, 512))
    with pytest.raises(ValueError):  # a downsample at stride 1
        ops.conv3x3_stream8(z(1, 14, 14, 256), z(256, 2304), v(256), v(256), wd=z(256, 256), alpha_d=v(256),
                            bias_d=v(256), out_scale_d=1.0)
    with pytest.raises(ValueError):  # a residual on ResNet50's 28x28x128 form
        ops.conv3x3_stream8(z(1, 28, 28, 128), z(128, 1152), v(128), v(128), res=z(1, 28, 28, 128))
    with pytest.raises(ValueError):  # channel doubling from 14x14x512
        ops.conv3x3_stream8(z(1, 14, 14, 512), z(1024, 4608), v(1024), v(1024), stride=2)
    assert not C.conv3x3_stream8_block_supported(14, 14, 256, 512, 2, True, False)
    x, y, r, wf, a, zero = z(1, 14, 14, 256), z(1, 14, 14, 256), z(1, 14, 14, 256), z(256, 2304), v(256), z(256)
    args = (x.data_ptr(), wf.data_ptr(), a.data_ptr(), a.data_ptr(), y.data_ptr(), zero.data_ptr(), 1, 14, 14, 256,
            256, 1, True, 1.0, 0)
    for bad in (y.data_ptr() + 8, x.data_ptr() + 8, r.data_ptr() + 4):  # res over y, over x, misaligned
        with pytest.raises(ValueError):
            C.conv3x3_stream8(*args, res=bad)

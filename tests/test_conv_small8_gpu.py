"""conv_small8 (conv_small8.hip: the query-batch e4m3 3x3 conv of the fp8
ResNets) against the float64 result on the same e4m3 operands under
_kernel_bar's e4m3 bar (K = 9 CI, CI for the downsample), at the ten forms the
models have. The real shapes are the smallest at which the kernel can go wrong:
a last pixel fragment with one live pixel (P = 49) and with four (P = 196),
tiles that cross output rows and touch both borders, KT = 9 and 18 (no
multiples of the 4 waves), and with B = 3 an image index > 0. Each case runs
the picked mf and mf = 1 against one reference.

Measured on an MI355X: worst |err| / bar 0.94 (the downsample, K = 256; 0.89
for the 3x3s); the controls miss the bar by 14x or more (profiles/small8.txt).
"""
import pytest
import torch

import dmlc
from dmlc import ops

from _kernel_bar import (assert_close, assert_rejects, conv_ref, e4m3_bound, e4m3_bytes, e4m3_weights,
                         fault_border_taps, fault_border_taps_s2, fault_ds_missing)

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
FORMS = {  # (H, CI, CO, stride, res, ds)
    "p28": (28, 128, 128, 1, False, False), "p14": (14, 256, 256, 1, False, False),
    "res14": (14, 256, 256, 1, True, False), "p7": (7, 512, 512, 1, False, False),
    "res7": (7, 512, 512, 1, True, False), "s56": (56, 128, 128, 2, False, False),
    "s28": (28, 256, 256, 2, False, False), "s14": (14, 512, 512, 2, False, False),
    "wide": (14, 256, 512, 2, False, False), "wide_ds": (14, 256, 512, 2, False, True)}


@pytest.mark.parametrize("B,exact", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("form", list(FORMS))
def test_conv_small8(gpu, form, B, exact):
    """test_stream8_block's operands and controls (the residual left out of one
    pixel fragment, the downsample's products left out of one, the kh = 1 taps
    of output row 0 at stride 2), and for plain stride 1 the kh = 0 taps of
    output row 1. exact: every fp32 value is exact whatever the wave order, so
    the output bytes are the float64 value rounded to e4m3."""
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
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    picked = dmlc.native().conv_small8_pick_mf(B, H, H, CI, CO, S, ds, cus)
    xg = x.permute(0, 2, 3, 1).contiguous().float().to(FP8).to(gpu)
    wg = w.permute(0, 2, 3, 1).reshape(CO, 9 * CI).float().to(FP8).to(gpu)
    for mf in sorted({picked, 1}):
        out = ops.conv_small8(xg, wg, alpha.float().to(gpu), bias.float().to(gpu), relu=True, out_scale=out_scale,
                              stride=S, mf=mf, **extra)
        torch.cuda.synchronize()
        y, yd = out if ds else (out, None)
        y = y.cpu().permute(0, 3, 1, 2).contiguous()
        yd = yd.cpu().permute(0, 3, 1, 2).contiguous() if ds else None
        what = f"conv_small8 {form} B={B} mf={mf}"

        if exact:
            want = e4m3_bytes(ref / out_scale)
            assert torch.equal(y.view(torch.uint8), want), f"{what}: {int((y.view(torch.uint8) != want).sum())} bytes differ"
            if ds:
                wantd = e4m3_bytes(refd / out_scale_d)
                assert torch.equal(yd.view(torch.uint8), wantd), f"{what}: {int((yd.view(torch.uint8) != wantd).sum())} differ"
            continue
        inv = float(torch.tensor(1.0 / out_scale, dtype=torch.float32))
        bnd = e4m3_bound(torch.relu(ref), mag, 9 * CI, inv)
        assert_close(y.double(), torch.relu(ref) * inv, bnd, what, l2=4e-2)
        if res:
            wrong = ref.clone()
            wrong.view(B, CO, -1)[B - 1, :, 16:32] -= rv.view(B, CO, -1)[B - 1, :, 16:32]
        elif S == 2:
            wrong = fault_border_taps_s2(ref, x, weff)
        else:
            wrong = fault_border_taps(ref, x, weff, 1)
        assert_rejects(y.double(), torch.relu(wrong) * inv, bnd, what + " [control]")
        if ds:
            invd = float(torch.tensor(1.0 / out_scale_d, dtype=torch.float32))
            bndd = e4m3_bound(refd, magd, CI, invd)
            assert_close(yd.double(), refd * invd, bndd, what + " downsample", l2=4e-2)
            wrongd = fault_ds_missing(refd, x, wdeff, b=B - 1, frag=1)
            assert_rejects(yd.double(), wrongd * invd, bndd, what + " downsample [control]")


def test_conv_small8_rejects(gpu):
    """Unsupported combinations, a residual that overlaps the output and a
    misaligned downsample output raise before any launch."""
    C = dmlc.native()
    z = lambda *s: torch.zeros(*s, device=gpu).to(FP8)
    v = lambda n: torch.ones(n, device=gpu)
    with pytest.raises(ValueError):  # a residual at stride 2
        ops.conv_small8(z(1, 14, 14, 256), z(512, 2304), v(512), v(512), stride=2, res=z(1, 7, 7, 512))
    with pytest.raises(ValueError):  # a downsample at stride 1
        ops.conv_small8(z(1, 14, 14, 256), z(256, 2304), v(256), v(256), wd=z(256, 256), alpha_d=v(256), bias_d=v(256))
    with pytest.raises(ValueError):  # CO = 2 CI at stride 1
        ops.conv_small8(z(1, 14, 14, 256), z(512, 2304), v(512), v(512))
    x, y, yd, wf, wdf, a, zero = z(1, 14, 14, 256), z(1, 14, 14, 256), z(1, 7, 7, 512 + 16), z(512, 2304), z(512, 256), \
        v(512), z(256)
    ptr = lambda *ts: [t.data_ptr() for t in ts]
    with pytest.raises(ValueError):  # res over y (4-B aligned: the overlap is what is wrong)
        C.conv_small8(*ptr(x, wf, a, a, y, zero), 1, 14, 14, 256, 256, 1, True, 1.0, 1, res=y.data_ptr() + 8)
    y2 = z(1, 7, 7, 512)
    ds = dict(wd=wdf.data_ptr(), alpha_d=a.data_ptr(), bias_d=a.data_ptr(), out_inv_scale_d=1.0)
    with pytest.raises(ValueError):  # a misaligned yd
        C.conv_small8(*ptr(x, wf, a, a, y2, zero), 1, 14, 14, 256, 512, 2, True, 1.0, 1, yd=yd.data_ptr() + 2, **ds)
    C.conv_small8(*ptr(x, wf, a, a, y2, zero), 1, 14, 14, 256, 512, 2, True, 1.0, 1, yd=yd.data_ptr(), **ds)
    torch.cuda.synchronize()  # (the same call, aligned, is accepted)

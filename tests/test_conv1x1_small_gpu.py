"""conv1x1_small (conv1x1_small.hip: the query-batch 1x1 conv of ResNet50)
against the float64 result on the same rounded operands under _kernel_bar's
derived bars (`bound` for bf16 out, `e4m3_bound` for e4m3 out, K = Cin), at the
models' own forms. They are the smallest shapes at which the kernel can go
wrong: every WK x KSW wave arrangement, P = 49 (one live pixel in the last
fragment; with B = 3 fragments straddle images), stride 2 with an image index
> 0, both mixed-type forms. Each case runs the picked (mf, nf) and (1, 1)
against one reference.

Measured on an MI355X: worst |err| / bar 0.990 (wk1, K = 64, B = 3; 0.94 for the e4m3 outputs); the controls
miss the bar by 132x or more (profiles/small1x1.txt).
"""
import pytest
import torch

import dmlc
from dmlc import ops

from _kernel_bar import (assert_close, assert_rejects, e4m3_bytes, fault_k_tile_missing, gemm_bar, gemm_k_range,
                         gemm_operands, gemm_ref, nchw, nhwc)

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
FORMS = {  # (H, Cin, N, in8, out8, res, stride)
    "k2048": (7, 2048, 512, False, False, False, 1), "k2048_8": (7, 2048, 512, True, True, False, 1),
    "n2048": (7, 512, 2048, False, False, True, 1), "n2048_8": (7, 512, 2048, True, True, True, 1),
    "s14_8": (14, 1024, 2048, True, True, False, 2), "s56": (56, 256, 512, False, False, False, 2),
    "wk2_8": (56, 256, 128, True, True, False, 1), "mix_8_16": (56, 256, 64, True, False, False, 1),
    "wk1": (56, 64, 64, False, False, False, 1), "mix_16_8": (56, 64, 256, False, True, True, 1)}
CASES = [(f, B, False) for f in FORMS for B in (1, 3)] + [(f, 3, True) for f, v in FORMS.items() if v[4]]


@pytest.mark.parametrize("form,B,exact", CASES)
def test_conv1x1_small(gpu, form, B, exact):
    """Controls: a quarter of K (a wave's share at WK = 4) missing from one
    pixel fragment, the residual left out of one, the unstrided pixel read at
    stride 2. exact: every fp32 value is exact in any order, so the output
    bytes are the float64 value rounded to e4m3."""
    H, Cin, N, in8, out8, res, S = FORMS[form]
    o = gemm_operands(B, H, H, Cin, N, 1, S, 0, res=res, seed=7 * H + B, exact=exact, in8=in8, out8=out8)
    v, mag = o["ref"]
    it, ot = (FP8 if in8 else torch.bfloat16), (FP8 if out8 else torch.bfloat16)
    kw = dict(stride=S, relu=True, out_scale=o["out_scale"])
    if in8:
        kw["alpha"] = o["alpha"].float().to(gpu)
    if res:
        kw.update(res=nhwc(o["r"]).float().to(ot).to(gpu), res_scale=o["res_scale"])
    xg, wg = nhwc(o["x"]).float().to(it).to(gpu), o["w"].reshape(N, Cin).float().to(it).to(gpu)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    picked = tuple(dmlc.native().conv1x1_small_pick(B, H, H, Cin, N, S, in8, out8, cus))
    for mf, nf in sorted({picked, (1, 1)}):
        y = ops.conv1x1_small(xg, wg, o["bias"].float().to(gpu), mf=mf, nf=nf, **kw)
        torch.cuda.synchronize()
        y = nchw(y.cpu())
        what = f"conv1x1_small {form} B={B} mf={mf} nf={nf}"
        if exact:
            want = e4m3_bytes(v / o["out_scale"])
            assert torch.equal(y.view(torch.uint8), want), f"{what}: {int((y.view(torch.uint8) != want).sum())} bytes differ"
            continue
        want, bnd, l2 = gemm_bar(o, v, mag)
        assert_close(y.double(), want, bnd, what, l2=l2)
        rows = lambda t: nhwc(t).reshape(-1, N)
        back = lambda t: nchw(t.reshape(B, v.shape[2], v.shape[3], N))
        m0 = 16 * ((rows(v).shape[0] - 1) // 16)  # the last pixel fragment
        lost = gemm_k_range(o, 0, max(1, Cin // o["bk"] // 4))
        wrongs = [("K range", back(fault_k_tile_missing(rows(v), rows(lost), m0, 16)))]
        if res:
            wrongs.append(("residual", back(fault_k_tile_missing(rows(v), rows(o["r"] * o["res_scale"]), 16, 16))))
        if S == 2:
            wrongs.append(("unstrided", gemm_ref(dict(o, x=o["x"][:, :, :v.shape[2], :v.shape[3]], stride=1))[0]))
        for name, wrong in wrongs:
            assert_rejects(y.double(), gemm_bar(o, wrong, mag)[0], bnd, f"{what} [control: {name}]")


def test_conv1x1_small_rejects(gpu):
    """Unsupported geometry, a missing alpha, a misaligned output, a residual
    over the output and an unknown tile raise before any launch."""
    C = dmlc.native()
    z = lambda *s: torch.zeros(*s, device=gpu, dtype=torch.bfloat16)
    x, w, b, y = z(1, 7, 7, 512), z(64, 512), torch.zeros(64, device=gpu), z(1, 7, 7, 64 + 16)
    call = lambda **k: C.conv1x1_small(**{**dict(x=x.data_ptr(), w=w.data_ptr(), bias=b.data_ptr(), y=y.data_ptr(), B=1,
                                                 H=7, W=7, Cin=512, N=64, stride=1, relu=True, in_fp8=False,
                                                 out_fp8=False, mf=1, nf=1), **k})
    for bad in (dict(stride=3), dict(Cin=96), dict(N=24), dict(in_fp8=True), dict(y=y.data_ptr() + 4),
                dict(res=y.data_ptr() + 8), dict(x=0), dict(mf=3), dict(mf=8, nf=8), dict(Kpad=256)):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):  # a 3-channel-deep weight matrix is no 1x1 conv of x
        ops.conv1x1_small(x, z(64, 3 * 512), b)
    with pytest.raises(ValueError):  # a residual of the other type
        ops.conv1x1_small(x, w, b, res=z(1, 7, 7, 64), out_scale=1.0)
    call()
    torch.cuda.synchronize()  # (the same call, valid, is accepted)
    assert not y.float().any()

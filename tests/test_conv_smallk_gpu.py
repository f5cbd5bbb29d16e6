"""ops.conv_smallk (conv_smallk.hip) against float64 under the op tests' element-wise bar (_kernel_bar.py;
K = 1600 for the 5x5, 9 CI for the 3x3s). The exact cases use small integers: every partial sum is exact in
fp32 in any order (|sum| <= 3456 * 6), so the output is the float64 reference rounded to bf16 bit for bit."""
import pytest
import torch

from dmlc import ops

import _kernel_bar as kb

pytestmark = pytest.mark.gpu

# (H, CI, CO, ks, pad, pooled form)
SHAPES = {"features.3": (27, 64, 192, 5, 2, True), "features.6": (13, 192, 384, 3, 1, False),
          "features.8": (13, 384, 256, 3, 1, False), "features.10": (13, 256, 256, 3, 1, True)}


def _dev(x_nchw, gpu):
    return kb.nhwc(x_nchw).bfloat16().to(gpu)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_conv_smallk(gpu, name, B):
    H, CI, CO, ks, pad, pooled = SHAPES[name]
    g = torch.Generator().manual_seed(70 + 10 * list(SHAPES).index(name) + B)
    x = torch.randn(B, CI, H, H, generator=g).bfloat16().double()
    w = (torch.randn(CO, CI, ks, ks, generator=g) / (CI * ks * ks) ** 0.5).bfloat16().double()
    bias = (torch.randn(CO, generator=g) * 0.1).float().double()
    ref, mag = kb.conv_ref(x, w, bias, 1, pad)
    wp, xd, bd = ops.pack_conv_weight(w.float(), device=gpu), _dev(x, gpu), bias.float().to(gpu)
    controls = [("border taps", kb.fault_border_taps(ref, x, w, pad)),
                ("seam taps", kb.fault_border_taps(ref, x, w, pad, at=2 - pad))]  # conv row 2: pooled rows 0 and 1
    if B > 1:
        controls.append(("batch shift", kb.fault_batch_shift(ref)))
    for relu in (False, True):
        r = torch.relu(ref) if relu else ref
        bnd = kb.bound(r, mag, ks * ks * CI)
        for mf in (1, 2, 4, None):
            y = ops.conv_smallk(xd, wp, bd, ks=ks, pad=pad, relu=relu, mf=mf)
            assert y.shape == (B, H, H, CO)
            y = kb.nchw(y.cpu())
            kb.assert_close(y, r, bnd, f"conv_smallk {name} B={B} relu={relu} mf={mf}")
        for what, wrong in controls:
            kb.assert_rejects(y, torch.relu(wrong) if relu else wrong, bnd, what)
    with pytest.raises(ValueError):  # no pool without ReLU; no pooled form of features.6 / .8
        ops.conv_smallk(xd, wp, bd, ks=ks, pad=pad, relu=not pooled, pool=True)
    if pooled:
        yp = ops.conv_smallk(xd, wp, bd, ks=ks, pad=pad, pool=True)
        assert yp.shape == (B, (H - 3) // 2 + 1, (H - 3) // 2 + 1, CO)
        yp = kb.nchw(yp.cpu())
        kb.assert_close_pooled(yp, r, bnd, f"conv_smallk {name} + pool B={B}")
        for what, wrong in controls:
            kb.assert_rejects(yp, kb.maxpool(torch.relu(wrong)), kb.maxpool(bnd), what)


@pytest.mark.parametrize("name,pool", [("features.3", True), ("features.6", False), ("features.10", True)])
def test_conv_smallk_exact(gpu, name, pool):
    H, CI, CO, ks, pad, _ = SHAPES[name]
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-3, 4, (2, CI, H, H), generator=g).double()
    w = torch.randint(-2, 3, (CO, CI, ks, ks), generator=g).double()
    bias = torch.randint(-8, 9, (CO,), generator=g).double()
    ref = kb.bf16r(kb.conv_ref(x, w, bias, 1, pad)[0])
    wp, xd, bd = ops.pack_conv_weight(w.float(), device=gpu), _dev(x, gpu), bias.float().to(gpu)
    if pool:
        y = ops.conv_smallk(xd, wp, bd, ks=ks, pad=pad, pool=True)
        assert torch.equal(kb.nchw(y.cpu()).double(), kb.maxpool(torch.relu(ref)))
        return
    for mf in (1, 2, 4):
        y = ops.conv_smallk(xd, wp, bd, ks=ks, pad=pad, relu=False, mf=mf)
        assert torch.equal(kb.nchw(y.cpu()).double(), ref), mf


def test_conv_smallk_bad_operands(gpu):
    x = torch.zeros(1, 13, 13, 256, dtype=torch.bfloat16, device=gpu)
    wp = torch.zeros(256, 9 * 256, dtype=torch.bfloat16, device=gpu)
    bias = torch.zeros(264, device=gpu)
    ops.conv_smallk(x, wp, bias[:256], ks=3, pad=1)
    for bad in (dict(x=torch.zeros(1, 14, 14, 256, dtype=torch.bfloat16, device=gpu)),  # a 14x14 input
                dict(x=x[..., :128].contiguous(), w_packed=wp[:, :9 * 128].contiguous()),  # CI = 128
                dict(bias=bias[1:257]),  # a misaligned bias
                dict(out=x),  # y aliasing x
                dict(mf=3)):
        with pytest.raises(ValueError):
            ops.conv_smallk(**{**dict(x=x, w_packed=wp, bias=bias[:256], ks=3, pad=1), **bad})
    torch.cuda.synchronize()

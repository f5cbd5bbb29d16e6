"""conv3x3_stream8's ResNet50 forms (conv3x3_stream8.hip on the template of
conv3x3_stream8_kernel.h: the bottleneck's e4m3 3x3 conv) against the float64
result on the same e4m3 operands, under _kernel_bar's e4m3 bar:

 * stride 1 on 28x28x128 (two 14-row strips with a halo row), 14x14x256 (an
   image per workgroup) and 7x7x512 (two images per workgroup);
 * stride 2 on 56x56x128 (4-row strips, and the launcher's variant 4 with
   7-row strips), 28x28x256 (two 7-row strips) and 14x14x512 (an image).

These are the only spatial shapes the kernel takes. B = 1 and B = 3: 7x7x512
then leaves its last workgroup an image short, and every strip form runs
several workgroups per image and several images.

The kernel's arithmetic (conv3x3_stream8_kernel.h): q = fma(acc, alpha inv,
bias inv) with alpha inv and bias inv rounded to fp32 once, a med3 with (0 or
-448, 448), e4m3: two more roundings of 2^-24 on terms inside mag, well inside
the K 2^-23 mag of the bar (K = 9 C).

Per (form, B):
 * random e4m3 codes with scales that are no powers of two, the output scale
   putting the largest relu(ref) at 400 of 448, under the e4m3 bar and the
   relative-L2 bar 4e-2;
 * the same output against three faulty references, which the bar must
   reject: the kh = 0 taps of the row where the second workgroup's strip
   starts (the strip's halo row; the image's top border row where a workgroup
   holds whole images), a 16-byte chunk swapped between two pixels of the last
   image, and at B = 3 a batch shift;
 * exact operands (small integer codes, sparse weights in -2..2, power-of-two
   scales: every fp32 value inside the kernel is exact in any order): the
   output bytes are the float64 value rounded to e4m3 at out_scale = 2, and at
   a scale of 2^-6, where 13..25 % of the values exceed 448 and must come out
   as 0x7E; with relu=False (the lower clamp at -448) the bytes are the signed
   value's at both scales, 16..25 % of them 0xFE at the second.
tests/test_kernel_bar_cpu.py checks without a GPU that these operands keep a
correctly rounded result inside the bar and that the bar rejects each control.

Measured on an MI355X: worst |err| / bar 0.93 over the 14 cases (28x28x128
0.92, 14x14x256 0.89, 7x7x512 0.84, 56x56x128/s2 0.93 with either strip
height, 28x28x256/s2 0.89, 14x14x512/s2 0.85), which is what the float64
reference rounded to e4m3 gives against itself: the products are exact and the
fp32 sums nearly so, the error is the output rounding. The controls miss the
bar by 33x or more (seam / border taps 60x, chunk swap 33x, batch shift 117x
at the least). Every exact, saturation and relu=False case is byte-equal.
"""
import pytest
import torch

import dmlc
from dmlc import ops

from _kernel_bar import (L2_E4M3, STREAM8_FORMS, STREAM8_SAT_SCALE, assert_close, assert_rejects, e4m3_bytes,
                         e4m3_bytes_signed, nchw, nhwc, stream8_bar, stream8_controls, stream8_operands)

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
CASES = [(f, B) for f in STREAM8_FORMS for B in (1, 3)]
IDS = [f"{f}-b{B}" for f, B in CASES]
_RANDOM = {}


def _run(gpu, form, o, relu=True, out_scale=None):
    """The form's kernel on the operands o: the output, NCHW on the CPU."""
    C, variant = STREAM8_FORMS[form][1], STREAM8_FORMS[form][3]
    args = (nhwc(o["x"]).float().to(FP8).to(gpu), o["w"].permute(0, 2, 3, 1).reshape(C, 9 * C).float().to(FP8).to(gpu),
            o["alpha"].float().to(gpu), o["bias"].float().to(gpu))
    kw = dict(relu=relu, out_scale=o["out_scale"] if out_scale is None else out_scale, stride=o["S"])
    if variant:
        Cn = dmlc.native()
        Cn.conv3x3_stream8_set_variant(variant)
        try:
            y = ops.conv3x3_stream8(*args, **kw)
        finally:
            Cn.conv3x3_stream8_set_variant(0)
    else:
        y = ops.conv3x3_stream8(*args, **kw)
    torch.cuda.synchronize()
    return nchw(y.cpu())


def _random(gpu, form, B):
    """(operands, output) of the random case, run once for the two tests that read it."""
    if (form, B) not in _RANDOM:
        o = stream8_operands(form, B)
        _RANDOM[form, B] = (o, _run(gpu, form, o).double())
    return _RANDOM[form, B]


@pytest.mark.parametrize("form,B", CASES, ids=IDS)
def test_stream8_random(gpu, form, B):
    o, y = _random(gpu, form, B)
    want, bnd = stream8_bar(o)
    assert_close(y, want, bnd, f"stream8 {form} B={B}", l2=L2_E4M3)


@pytest.mark.parametrize("form,B", CASES, ids=IDS)
def test_stream8_controls(gpu, form, B):
    o, y = _random(gpu, form, B)
    want, bnd = stream8_bar(o)
    controls = stream8_controls(form, o)
    assert len(controls) == (3 if B > 1 else 2)
    for name, wrong in controls:
        assert_rejects(y, stream8_bar(o, wrong)[0], bnd, f"stream8 {form} B={B} [{name}]")


def _assert_bytes(y, want, what):
    got = y.view(torch.uint8)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} bytes differ"


@pytest.mark.parametrize("form,B", CASES, ids=IDS)
def test_stream8_exact(gpu, form, B):
    o = stream8_operands(form, B, exact=True)
    ref = o["ref"][0]
    for scale in (o["out_scale"], STREAM8_SAT_SCALE):
        v = ref / scale
        over, under = v > 448, v < -448
        assert (scale == STREAM8_SAT_SCALE) == bool(over.any()) == bool(under.any())
        y = _run(gpu, form, o, out_scale=scale)
        _assert_bytes(y, e4m3_bytes(v), f"stream8 {form} B={B} exact, out_scale {scale}")
        wrong = int((y.view(torch.uint8)[over] != 0x7E).sum())
        assert wrong == 0, f"stream8 {form} B={B}: {wrong} of {int(over.sum())} saturated bytes are not 0x7E"
        y = _run(gpu, form, o, relu=False, out_scale=scale)
        _assert_bytes(y, e4m3_bytes_signed(v), f"stream8 {form} B={B} exact, relu=False, out_scale {scale}")
        wrong = int((y.view(torch.uint8)[under] != 0xFE).sum())
        assert wrong == 0, f"stream8 {form} B={B}: {wrong} of {int(under.sum())} bytes below -448 are not 0xFE"

"""Op-level times of conv3x3_stream8's basic-block forms at B = 256 on
cuda:0 (device events around 50 back-to-back launches of the native launcher,
the forms interleaved in 5 rounds, minimum per form): the numbers of
profiles/stream8_block_forms.txt.  python tools/stream8_block_times.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dmlc
from dmlc import ops

FP8 = torch.float8_e4m3fn
gpu = torch.device("cuda:0")
B = 256
g = torch.Generator().manual_seed(0)


def q(*s):
    return (torch.rand(*s, generator=g) * 8).to(FP8).to(gpu)


def v(n):
    return torch.ones(n, device=gpu) * 0.01


C = dmlc.native()
zero = torch.zeros(4096, dtype=torch.uint8, device=gpu)
keep, forms = [], {}


def native(x, wf, H, Ci, Co, S, **kw):
    a, b, y = v(Co), v(Co), torch.empty(B, H // S, H // S, Co, dtype=torch.uint8, device=gpu)
    keep.extend([x, wf, a, b, y])
    kw = {k: (t.data_ptr() if torch.is_tensor(t) else t) for k, t in kw.items()}
    return lambda: C.conv3x3_stream8(x.data_ptr(), wf.data_ptr(), a.data_ptr(), b.data_ptr(), y.data_ptr(),
                                     zero.data_ptr(), B, H, H, Ci, Co, S, True, 1.0, 0, **kw)


for H, Cc in ((14, 256), (7, 512)):
    x, r = q(B, H, H, Cc), q(B, H, H, Cc)
    wf = ops.stream8_weight_frag(q(Cc, 9 * Cc), Cc)
    keep.append(r)
    forms[f"plain {H}x{H}x{Cc}"] = native(x, wf, H, Cc, Cc, 1)
    forms[f"RES   {H}x{H}x{Cc}"] = native(x, wf, H, Cc, Cc, 1, res=r, res_scale=0.5)
x = q(B, 14, 14, 256)
wf, wdf = ops.stream8_weight_frag(q(512, 2304), 512), ops.stream8_weight_frag(q(512, 256), 512)
ad, bd, yd = v(512), v(512), torch.empty(B, 7, 7, 512, dtype=torch.uint8, device=gpu)
keep.extend([wdf, ad, bd, yd])
forms["WIDE    14x14x256->7x7x512"] = native(x, wf, 14, 256, 512, 2)
forms["WIDE+DS 14x14x256->7x7x512"] = native(x, wf, 14, 256, 512, 2, wd=wdf, alpha_d=ad, bias_d=bd, yd=yd,
                                             out_inv_scale_d=1.0)
best = {k: 1e9 for k in forms}
for k, f in forms.items():
    for _ in range(5):
        f()
torch.cuda.synchronize()
N = 50
for rnd in range(5):
    for k, f in forms.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            f()
        e1.record()
        torch.cuda.synchronize()
        best[k] = min(best[k], e0.elapsed_time(e1) * 1000 / N)
for k, t in best.items():
    print(f"{k}: {t:.1f} us per call (B = {B}, min of 5 rounds of {N})")

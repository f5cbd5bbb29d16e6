"""Every launch of an engine forward against the float64 reference of its plan
step (_engine_ref.py), under the op tests' element-wise bars.

After one eager forward every step of plan(B, 224, 224, keep_acts=True) whose
kernel is not None is recomputed in float64 from the activations the engine
itself stored (its reported scales, weights rebuilt from the state dict by the
packer's rule, semantics from the torch model) and every activation the step
stores must lie within the step's bar (kb.assert_close at 1.0). So what sits
between the kernels is judged launch by launch: which activation a launch
reads and adds, the batch-norm fold, alpha = s_in s_w, the residual's scale
and the output's 1 / scale, cscale along N and K, fc_hwc, the ReLU flags, the
fused downsamples, the pools and the heads. Images 0, 1 and B - 1 are
compared. The stems' input values are pinned to the float64 normalisation. Every Conv, pool, quantise and head op lies in exactly one audited
step, a kernel without a reference fails; at least two modelled plumbing
faults per case are rejected on the engine's own output; three graph replays
give the eager forward's idx bit for bit.

The input is mixed_images. An e4m3 element whose reference lies within its bar
of 448 is left out (_engine_ref.judge); at most 1 % of a tensor may be.

Measured on an MI355X (records of the run that added this file; the thresholds
are the bars, at 1.0). Worst |err| / bar per kernel kind over the ten cases:
StemPoolU8 0.98, AlexStem 0.93, Small 0.99, Rows 0.97, Block 0.84, S2Rows
0.91, S2Rows128 0.93, Rows28 0.93, Stream 0.99, Stream8 0.94, Igemm 0.94,
BigTile 0.68, Conv1x1 0.96, Conv1x1Cat 0.94, Conv1x1Chain 0.94,
Bottleneck56Head 0.89, Bottleneck56 0.90, Direct27 0.77, Direct13 0.74,
QuantE4m3 0.89, FcSmall 0.35, FcGemm8 0.53, AvgPoolGlobal 0.99, HeadFused
0.07, HeadPooled and FcGemm (fp32 logits) below 0.01. The weakest control per
case, on the elements the good reference holds to its bar (neither saturated
nor left out): resnet18_fp8 72 (B = 3) and 1041 (B = 64), resnet34_fp8 45,
resnet50_fp8 638 at both batches and 740 with fp8_3x3_in off, resnet18 5113
(B = 1) and 519 (B = 256), alexnet 39, alexnet_fp8 5.8. The largest left-out
share of any tensor: 0.11 % (resnet50_fp8 B = 4; 0.04 % at B = 256, 0.03 % with
fp8_3x3_in off, 0.01 % alexnet_fp8, none elsewhere), so mixed_images meets the
1 % cap. The float64 reference of the largest case (resnet50_fp8, three
images) took 8 s of CPU time summed over the threads; the whole file ran in
17 s.

The default options run resnet50_fp8's layer2.0.conv2 on Stream8 (fp8_3x3_in);
the case with that option off brings S2Rows128 in, and Rows28 / Stream with
e4m3 outputs and per-channel scales.
"""
import functools
import time

import pytest
import torch

import _engine_ref as er
import _kernel_bar as kb
from dmlc import ops
from dmlc.models import state_dict_f32
from dmlc.models.calibrated import MEAN, STD, calibrated, mixed_images
from dmlc.runtime import InferenceEngine

pytestmark = pytest.mark.gpu

# (arch, B, options, kernels the planner picks on a 256-CU device, (kernel, detail or first op) some step must have)
CASES = [
    ("resnet18_fp8", 3, {}, {"Igemm"}, [("Igemm", n) for n in ("layer3.0.conv2", "layer3.1.conv1", "layer4.0.conv1",
                                                                "layer4.0.downsample.0", "layer4.1.conv2")]),
    ("resnet18_fp8", 64, {}, {"Stream8"}, [("Stream8", "ds=layer4.0.downsample.0"), ("Stream8", "layer3.1.conv2")]),
    ("resnet34_fp8", 64, {}, {"Stream8"}, [("Stream8", "ds=layer4.0.downsample.0"), ("Stream8", "layer3.1.conv2")]),
    ("resnet50_fp8", 4, {}, set(), []),
    ("resnet50_fp8", 256, {}, {"Bottleneck56", "Bottleneck56Head", "Conv1x1Chain", "Conv1x1Cat", "Stream8", "Conv1x1",
                               "AvgPoolGlobal", "HeadPooled"}, []),
    # the default options run layer2.0.conv2 on Stream8; with bf16-reading 3x3 convs S2Rows128 runs it, and
    # Rows28 / Stream write e4m3 with per-channel scales
    ("resnet50_fp8", 256, {"fp8_3x3_in": False}, {"S2Rows128", "Rows28", "Stream", "BigTile"},
     [("S2Rows128", "layer2.0.conv2")]),
    ("resnet18", 1, {}, {"Small", "HeadFused"}, []),
    ("resnet18", 256, {}, {"Block", "S2Rows", "Rows28", "Stream", "HeadPooled"},
     [("Rows28", "dsk=layer2.0.downsample.0"), ("Stream", "pool=avgpool")]),
    ("alexnet", 3, {}, set(), []),
    ("alexnet_fp8", 32, {}, set(), []),
]


@functools.lru_cache(maxsize=None)
def _model(base):
    m = calibrated(base, seed=11)
    return m, state_dict_f32(m)


def _read(e, a, i, B, sel, gpu):
    """Images `sel` of stored activation i as codes, NCHW float64."""
    dtype = torch.float32 if a.f32 else torch.uint8 if a.fp8 else torch.bfloat16
    t = torch.empty(B, a.H * a.W * a.C, dtype=dtype, device=gpu)
    e.read_activation(i, B, t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t = t[sel].cpu()
    t = t.view(er.FP8) if a.fp8 else t
    return kb.nchw(t.double().view(len(sel), a.H, a.W, a.C))


@pytest.mark.parametrize("arch,B,opts,kernels,details", CASES,
                         ids=[f"{c[0]}-b{c[1]}" + "".join(f"-{k}={v}" for k, v in c[2].items()) for c in CASES])
def test_engine_steps(gpu, arch, B, opts, kernels, details):
    m, sd = _model(arch.replace("_fp8", ""))
    eng = InferenceEngine(arch, sd, max_batch=B, options=opts)
    e = eng._e
    view = er.View.of_engine(e, B)
    if e.num_cus == 256:
        have = {p[0] for p in view.plan}
        assert kernels <= have, kernels - have
        for k, d in details:
            assert any(p[0] == k and (d in p[3].split() or d == p[1]) for p in view.plan), (k, d)
    else:
        print(f"{arch} B={B}: {e.num_cus} CUs, the expected kernels are those of a 256-CU device: not asserted")
    img = mixed_images(B, seed=40 + B)
    x = img.to(gpu)
    idx, prob, logits = eng.predict(x, return_logits=True, use_graph=False)
    torch.cuda.synchronize()
    sel = sorted({0, min(1, B - 1), B - 1})
    logits_act = [o for o in view.ops if o[0] in ("fc", "classifier.6")][0][2]
    cache = {logits_act: logits[sel].cpu().double().view(len(sel), -1, 1, 1)}

    def acts(i):
        if i not in cache:
            cache[i] = _read(e, view.acts[i], i, B, sel, gpu)
        return cache[i]

    # the values the stems read (preprocess_u8, as in the stems' op tests), pinned to the float64 normalisation:
    # (x / 255 - mean) / std evaluated in fp32 in whatever form (a few roundings of its terms' magnitude), then
    # rounded to bf16
    x0 = kb.nchw(ops.preprocess_u8(x[sel], 224, 0).cpu()).double()
    u = img[sel].permute(0, 3, 1, 2).double() / 255
    want = (u - MEAN.double()) / STD.double()
    kb.assert_close(x0, want, kb.EPS_OUT * want.abs() + 4 * 2.0 ** -24 * (u + MEAN.double()) / STD.double(),
                    f"{arch} B={B} stem input")
    ref = er.StepRef(er.Sem(m), view, acts, x0)
    worst, shares, done, outs, cpu = {}, [0.0], [], {}, 0.0
    for i, p in enumerate(view.plan):
        if p[0] == "None":
            continue
        t0 = time.process_time()
        outs[i] = ref.step(i)
        cpu += time.process_time() - t0
        assert outs[i] or p[0] in ("SoftmaxTop1", "Preprocess"), f"step {p} stores nothing"
        if p[0] != "Preprocess":
            done += view.covered(i)
        for out in outs[i]:
            what = f"{arch} B={B} {p[0]} {p[1]} -> act {out.act}"
            got, r, bar, share = er.judge(acts(out.act), out, view.acts[out.act].fp8, what)
            shares.append(share)
            assert share <= 0.01, f"{what}: {share:.2%} of the tensor left out"
            ratio, _ = kb.assert_close(got, r, bar, what, l2=out.l2)
            worst[p[0]] = max(worst.get(p[0], 0.0), ratio)
    print(f"{arch} B={B}: worst |err|/bar per kernel {({k: round(v, 3) for k, v in worst.items()})}; "
          f"largest left-out share {max(shares):.4%}; float64 reference {cpu:.1f} s CPU for {len(sel)} images")
    # coverage: every op of the model in exactly one audited step
    want = [o[0] for o in view.ops if o[0] != "preprocess"]
    assert sorted(n for n in done if n != "preprocess") == sorted(want), "an op is in no audited step, or in two"
    # the tail's top-1 against the logits it wrote
    assert torch.equal(idx.cpu().long(), logits.cpu().argmax(-1))
    assert torch.allclose(prob.cpu(), torch.softmax(logits.cpu(), -1).max(-1).values, rtol=1e-4, atol=1e-6)
    # controls on the engine's own output
    rejected, weakest = 0, float("inf")
    for label, (i, fault) in er.controls(view, ref.sem).items():
        weakest = min(weakest, er.rejected(ref, i, outs[i], acts, fault, f"{arch} B={B} {view.plan[i][1]} [{label}]"))
        rejected += 1
    print(f"{arch} B={B}: weakest control {weakest:.1f}")
    if len(sel) > 1:
        i = max(j for j in outs if outs[j])
        good = outs[i][0]
        kb.assert_rejects(acts(good.act), kb.fault_batch_shift(good.ref), good.bar, f"{arch} B={B} [batch shift]")
        rejected += 1
    assert rejected >= 2, "fewer than two controls apply to this case"
    for _ in range(3):
        assert torch.equal(eng.predict(x, use_graph=True)[0], idx)

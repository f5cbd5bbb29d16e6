"""_engine_ref.py, the reference the engine's forward is audited against
(test_engine_steps_gpu.py), checked without a GPU.

1. The semantics table is right: the step references of the one-op-per-step
   view chained with no rounding anywhere, from normalize(img), give the
   float64 torch model's logits. The two differ only by float64 reassociation
   (the batch norm folded into the weights, the sums in another order), a few
   ulps of float64 an op: the bar is 4 x 2^-53 x the number of ops in the
   chain, relative to the largest logit (resnet50: 56 ops, 2.5e-14; a wrong
   stride, padding, ReLU, residual or batch norm is off by percents).
2. The bar passes a correct engine: a software engine that stores every
   step's reference rounded to its storage type (the bf16 rounding of the
   folded weights is part of the operands), with scales that are no powers of
   two and put each tensor's largest value at 145 to 300 of e4m3's 448, passes
   every step of the plans the planner makes for a 256-CU device.
3. The bar rejects each modelled plumbing fault at the step where it occurs.
"""
import functools

import pytest
import torch

import _engine_ref as er
import _kernel_bar as kb
from dmlc import native
from dmlc.models import build, state_dict_f32
from dmlc.models.calibrated import noise_images, normalize

N_IMG = 2


@functools.lru_cache(maxsize=None)
def _model(arch):
    """A random-init model with non-trivial BN statistics, its residual branches damped as the calibrated models'
    are (undamped the net is chaotic, and the scales taken from the exact chain would not fit the rounded one)."""
    m = build(arch, seed=3, randomize_bn=True).double()
    with torch.no_grad():
        for mod in m.modules():
            if hasattr(mod, "bn2"):
                last = mod.bn3 if hasattr(mod, "bn3") else mod.bn2
                last.weight.mul_(0.15)
                last.bias.mul_(0.15)
    return m, {k: v.float() for k, v in state_dict_f32(m).items()}


@functools.lru_cache(maxsize=None)
def _x0():
    return normalize(noise_images(N_IMG, seed=5)).double()


def _exact_chain(arch):
    """Every activation of the unfused, unrounded chain: {act id: NCHW float64}."""
    m, sd = _model(arch)
    _, ops = native().plan_audit(arch, sd, {}, B=1)
    view = er.View(ops, [None] * (max(o[2] for o in ops) + 1), er.unfused_plan(ops))
    acts = {}
    ref = er.StepRef(er.Sem(m), view, acts.__getitem__, _x0(), rounded=False)
    for i in range(len(view.plan)):
        for out in ref.step(i):
            acts[out.act] = out.ref
    return ops, acts


@pytest.mark.parametrize("arch", ["resnet18", "resnet34", "resnet50", "alexnet"])
def test_unrounded_chain_is_the_torch_model(arch):
    m, _ = _model(arch)
    ops, acts = _exact_chain(arch)
    with torch.no_grad():
        want = m(_x0()[:1])
    got = acts[[o for o in ops if o[0] in ("fc", "classifier.6")][0][2]].flatten(1)[:1]
    tol = 4 * 2.0 ** -53 * len(ops)
    err = ((got - want).abs().max() / want.abs().max()).item()
    print(f"{arch}: unrounded chain vs float64 torch: {err:.2e} of the largest logit (bar {tol:.2e})")
    assert err <= tol


def _scaled(x, i=0):
    """A scale that is no power of two and puts the tensor's largest exact value x at 300 / 1.2^(i mod 5) of e4m3's
    448: a block's input and output (ids 2 or 3 apart) then have scales an e4m3 step apart even where the tensors
    have the same range, as a damped block's do."""
    return float(er._f32(float(x) * 1.2 ** (i % 5) / 300.0))


@functools.lru_cache(maxsize=None)
def _software_engine(arch, B, opts=()):
    """(view, StepRef on the stored codes, {step: [Out]}, stored) of an ideal engine on the plan for batch B
    (opts: engine options as items)."""
    m, sd = _model(arch)
    base = arch.replace("_fp8", "")
    C = native()
    plan, ops = C.plan_audit(arch, sd, dict(opts), B=B, keep_acts=True)
    _, exact = _exact_chain(base)
    ex_ops = {o[0]: o for o in C.plan_audit(base, sd, {}, B=1)[1]}
    acts = []
    for i, (H, W, Ch, f32, fp8, chan) in enumerate(C.shape_audit(arch, sd, dict(opts))):
        scale, cscale = 1.0, None
        if fp8:  # as the engine calibrates: from the exact values of the tensor this activation stores
            name = [o[0] for o in ops if o[2] == i][0]
            v = exact[ex_ops["features.12" if name == "classifier.quant" else name][2]].abs()
            if chan:
                cscale = torch.tensor([_scaled(max(c, float(v.max()) * 0.05), i) for c in v.amax((0, 2, 3)).tolist()])
            else:
                scale = _scaled(v.max(), i)
        acts.append(er.Act(H, W, Ch, f32, fp8, scale, cscale))
    view = er.View(ops, acts, plan)
    stored, outs = {}, {}
    ref = er.StepRef(er.Sem(m), view, stored.__getitem__, kb.bf16r(_x0()), ideal=True)
    for i in range(len(plan)):
        outs[i] = ref.step(i)
        for out in outs[i]:
            a = acts[out.act]
            stored[out.act] = er.store(out, a.fp8, a.f32)
    return view, ref, outs, stored


NO_FP8_IN = (("fp8_3x3_in", False),)  # resnet50_fp8's 3x3 convs read bf16: S2Rows128, Rows28 and Stream write e4m3
CASES = [("resnet18", 256, ()), ("resnet18", 1, ()), ("resnet18_fp8", 64, ()), ("resnet50_fp8", 256, ()),
         ("resnet50_fp8", 256, NO_FP8_IN), ("alexnet", 3, ()), ("alexnet_fp8", 32, ())]


@pytest.mark.parametrize("arch,B,opts", CASES)
def test_rounded_reference_passes_every_step(arch, B, opts):
    view, ref, outs, stored = _software_engine(arch, B, opts)
    if opts:
        assert "S2Rows128" in {p[0] for p in view.plan}
    done = []
    for i in range(len(view.plan)):
        if view.plan[i][0] != "None":
            assert outs[i] or view.plan[i][0] == "SoftmaxTop1", view.plan[i]
            done += view.covered(i)
        for out in outs[i]:
            what = f"{arch} B={B} {view.plan[i][0]} {view.plan[i][1]} -> act {out.act}"
            got, r, bar, share = er.judge(stored[out.act], out, view.acts[out.act].fp8, what)
            assert share <= 0.01, what
            kb.assert_close(got, r, bar, what, l2=out.l2)
    want = [o[0] for o in view.ops if o[0] != "preprocess"]
    assert sorted(done) == sorted(want) or sorted(done) == sorted(want + ["preprocess"]), "an op is in no step, or in two"


@pytest.mark.parametrize("arch,B,expected", [
    ("resnet18", 256, {"ReLU dropped", "downsample bias left out"}),
    ("resnet18_fp8", 64, {"residual with the output's scale", "alpha from another activation's scale", "ReLU dropped"}),
    ("resnet50_fp8", 256, {"residual with the output's scale", "alpha from another activation's scale",
                           "ReLU dropped", "downsample bias left out", "cscale along N"}),
    ("alexnet_fp8", 32, {"fc read in NCHW order", "ReLU dropped"}),
])
def test_every_modelled_fault_is_rejected(arch, B, expected):
    view, ref, outs, stored = _software_engine(arch, B)
    found = er.controls(view, ref.sem)
    assert expected <= set(found), (expected - set(found), "the test scales are not an e4m3 step apart")
    for label, (i, fault) in found.items():
        er.rejected(ref, i, outs[i], stored.__getitem__, fault, f"{arch} {view.plan[i][1]} [{label}]")
    i = max(j for j in outs if outs[j] and float(outs[j][0].bar.min()) > 0)  # (a bar of 0 makes the ratio infinite)
    good = outs[i][0]
    kb.assert_rejects(stored[good.act], kb.fault_batch_shift(good.ref), good.bar, f"{arch} {view.plan[i][1]} [batch shift]")

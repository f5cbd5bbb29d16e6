"""A float64 reference of one step of the engine's plan, independent of the
engine (test_engine_ref_cpu.py, test_engine_steps_gpu.py).

A step reads stored activations and stores activations. Its reference starts
from the stored inputs themselves (dequantised with the engine's reported
scales), so no error carries from step to step and every output is judged by
the op tests' element-wise bars (_kernel_bar.py), not by a whole-model
tolerance.

What the engine contributes (`View`): activation ids per op, shapes, storage
types, scales and the plan. Everything else is rebuilt here:

 * the semantics of an op come from the torch model (`Sem`): kernel size,
   stride and padding from the nn.Module with the op's name, the batch norm
   that follows it, ReLU / residual / pooling from the architecture's rule;
 * the weights come from the state dict by the packer's stated rule (`fold`,
   `quant_rows`): s = g / sqrt(v + 1e-5) in double then fp32, w = bf16(W s) as
   an fp32 product, bias = b + (conv_bias - mean) s in double then fp32; an
   output with per-channel scales divides s and bias by cscale[n] first; an
   e4m3 layer multiplies the bf16 rows along K by the input's cscale, then
   s_w = amax / 448 in fp32, codes = e4m3(w / s_w), alpha = s_in s_w.

Units. An activation is held as its stored numbers ("codes": the bf16 values,
or the e4m3 numbers before the scale), NCHW float64. A conv computes
conv(codes, w) alpha + bias + res_codes res_scale, and an e4m3 output is that
times fp32(1 / scale); with per-channel scales the engine reports scale = 1,
the scales live in the weights.

Saturation (`judge`): an e4m3 element whose reference minus bar is at or past
448 must be the saturated code, one whose reference plus bar is below 448 is
judged by the bar, the ones in between are left out and counted.

`fault=` builds the same reference with one modelled plumbing fault, for the
negative controls: "res_scale" (the residual dequantised with the output's
scale), "alpha" (alpha from the residual's / another activation's scale, given
as fault_scale), "relu" (the last ReLU dropped), "ds_bias" (the fused
downsample's bias left out), "nchw" (an fc after a spatial tensor read in the
storage order without the permutation), "cscale_n" (the input's per-channel
scales applied along N). The batch shift is kb.fault_batch_shift on the result.
"""
import re
from collections import namedtuple

import torch
import torch.nn as nn
import torch.nn.functional as F

import _kernel_bar as kb

FP8 = torch.float8_e4m3fn
Act = namedtuple("Act", "H W C f32 fp8 scale cscale")  # cscale: fp32 tensor [C] or None
Out = namedtuple("Out", "act ref bar l2")  # ref / bar in the output's own units, NCHW float64 ([n, N] for an fc)

SINGLE = {"Small", "Igemm", "Stream", "Stream8", "S2Rows", "S2Rows128", "Rows", "Rows28", "Conv1x1", "Conv1x1Cat",
          "BigTile", "FcSmall", "FcGemm", "FcSmall8", "FcGemm8", "Direct13", "Direct27"}
UNAUDITED = {"None", "Preprocess", "PackTensor"}  # nothing computed, or the input's layout (not an op of the model)


class View:
    """ops: [(name, in, out, res)]; acts: [Act]; plan: [(kernel, first op, n_ops, detail)]."""

    def __init__(self, ops, acts, plan):
        self.ops, self.acts, self.plan = list(ops), list(acts), list(plan)
        self.index = {o[0]: i for i, o in enumerate(self.ops)}

    @classmethod
    def of_engine(cls, e, B, S=224):
        acts = []
        for i in range(e.num_activations):
            H, W, C, f32 = e.activation_shape(i)
            fp8, scale = e.activation_quant(i)
            cs = e.activation_cscale(i)
            acts.append(Act(H, W, C, f32, fp8, scale, torch.tensor(cs, dtype=torch.float32) if len(cs) else None))
        return cls(e.op_list(), acts, e.plan(B, S, S, keep_acts=True))

    def step(self, i):
        kernel, first, n, detail = self.plan[i]
        f = self.index[first]
        d = dict(kv.split("=") for kv in detail.split() if "=" in kv)
        return dict(kernel=kernel, ops=self.ops[f:f + n], ds=d.get("ds"), dsk=d.get("dsk"), pool=d.get("pool"),
                    store_y="nostore" not in detail.split())

    def covered(self, i):
        """The op names step i computes."""
        st = self.step(i)
        return [o[0] for o in st["ops"]] + [n for n in (st["ds"], st["dsk"]) if n] + \
            ([st["pool"]] if st["pool"] and st["pool"] not in [o[0] for o in st["ops"]] else [])


def unfused_plan(ops):
    """One step per op, whatever kernel would run it."""
    def kernel(name):
        if name == "preprocess":
            return "None"
        if name == "conv1+maxpool":
            return "StemPool"
        if name in ("maxpool",) or re.fullmatch(r"features\.(2|5|12)", name):
            return "MaxPool"
        return {"avgpool": "AvgPoolGlobal", "softmax_top1": "SoftmaxTop1", "classifier.quant": "QuantE4m3"}.get(name, "Igemm")
    return [(kernel(o[0]), o[0], 1, "") for o in ops]


class Sem:
    """The architecture's rule, written down once."""

    def __init__(self, model):
        self.model = model
        self.resnet = hasattr(model, "layer1")

    def module(self, name):
        return self.model.get_submodule("conv1" if name == "conv1+maxpool" else name)

    def bn(self, name):
        if not self.resnet or name == "fc":
            return None
        if name in ("conv1", "conv1+maxpool"):
            return self.model.bn1
        if name.endswith("downsample.0"):
            return self.model.get_submodule(name[:-1] + "1")
        return self.model.get_submodule(name.replace(".conv", ".bn"))

    def relu(self, name):
        if self.resnet:  # every conv but the downsample is followed by a ReLU (the block's last one after the add)
            return name != "fc" and not name.endswith("downsample.0")
        seq, i = name.rsplit(".", 1)
        mods = list(self.model.get_submodule(seq))
        return int(i) + 1 < len(mods) and isinstance(mods[int(i) + 1], nn.ReLU)

    def has_res(self, name):
        """The block's last conv adds the block's input, or its downsample."""
        m = re.fullmatch(r"(layer\d\.\d+)\.conv(\d)", name)
        if not (self.resnet and m):
            return False
        return int(m.group(2)) == (3 if hasattr(self.model.get_submodule(m.group(1)), "conv3") else 2)

    def pool(self, name):
        m = self.model.maxpool if name in ("maxpool", "conv1+maxpool") else self.module(name)
        assert isinstance(m, nn.MaxPool2d), name
        return m.kernel_size, m.stride, m.padding

    def fold(self, name, rounded=True, out_cscale=None):
        """(w [N, C, kh, kw] or [N, K], bias [N]) float64: the packer's rule, or with rounded=False the exact fold."""
        m = self.module(name)
        W = m.weight.detach()
        cb = m.bias.detach().double() if m.bias is not None else torch.zeros(W.shape[0], dtype=torch.float64)
        bn = self.bn(name)
        shape = (-1,) + (1,) * (W.dim() - 1)
        if bn is not None:
            s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + 1e-5)
            bias = bn.bias.detach().double() + (cb - bn.running_mean.double()) * s
        else:
            s, bias = torch.ones(W.shape[0], dtype=torch.float64), cb
        if not rounded:
            return W.double() * s.view(shape), bias
        s32, b32 = s.float(), bias.float()
        if out_cscale is not None:
            s32, b32 = s32 / out_cscale, b32 / out_cscale
        return (W.float() * s32.view(shape)).bfloat16().double(), b32.double()


def quant_rows(w, in_cscale, s_in, along_n=False):
    """e4m3 rows of the bf16 weights w [N, C, kh, kw]: (codes float64, alpha = s_in s_w float64 [N])."""
    wv = w.float()
    if in_cscale is not None:
        if along_n:  # the modelled fault
            wv = wv * in_cscale[torch.arange(w.shape[0]) % in_cscale.numel()].view(-1, 1, 1, 1)
        else:
            wv = wv * in_cscale.view(1, -1, 1, 1)
    amax = wv.abs().amax((1, 2, 3))
    sw = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    codes = (wv / sw.view(-1, 1, 1, 1)).clamp(-448, 448).to(FP8).double()
    return codes, (torch.tensor(s_in, dtype=torch.float32) * sw).double()


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def inv_scale(a):
    """The epilogue's fp32 1 / scale of an e4m3 activation, as a float."""
    return float(_f32(1.0) / _f32(a.scale))


def e4m3_bar(ref, mag, K, inv):
    """kb.e4m3_bound without its range check: past 448 the rounding term stays at the top of the range (`judge`
    sorts those elements out)."""
    return K * kb.EPS_SUM * mag * inv + (kb.E4M3_EPS * ref.abs().clamp(max=kb.E4M3_MAX)).clamp_min(kb.E4M3_HALF_STEP)


class StepRef:
    def __init__(self, sem, view, acts, x0=None, rounded=True, ideal=False):
        """acts(id) -> the stored codes of an activation, NCHW float64 ([n, C, 1, 1] for a vector); x0: what the
        stem reads, [n, 3, S, S] float64. ideal: there is no engine, a launch's first output as its second conv
        reads it is the reference rounded to storage (a software engine: test_engine_ref_cpu.py)."""
        self.ideal = ideal
        self.sem, self.view, self.x0, self.rounded = sem, view, x0, rounded
        pre = [o[2] for o in view.ops if o[0] == "preprocess"]  # its activation is x0 in the stem's own layout
        self.acts = lambda i: x0 if i in pre else acts(i)

    # ------------------------------------------------------------ one conv / fc
    def weights(self, op, x, fault=None, fault_scale=None):
        """(w, alpha or None, bias, stride, pad, K) of op on an input of x's shape."""
        name, i, o, _ = op
        v = self.view
        a_in = v.acts[i] if i >= 0 else None
        w, bias = self.sem.fold(name, self.rounded, v.acts[o].cscale if self.rounded else None)
        m = self.sem.module(name)
        if isinstance(m, nn.Linear):  # torch flattens NCHW: a conv whose kernel is the whole [C, H, W] input
            C, H, W = x.shape[1:]
            w = w.view(-1, H, W, C).permute(0, 3, 1, 2) if fault == "nchw" else w.view(-1, C, H, W)
            stride, pad = 1, 0
        else:
            stride, pad = m.stride[0], m.padding[0]
        alpha = None
        if self.rounded and a_in is not None and a_in.fp8:
            w, alpha = quant_rows(w, a_in.cscale, fault_scale if fault == "alpha" else a_in.scale,
                                  along_n=fault == "cscale_n")
        return w, alpha, bias, stride, pad, w[0].numel()

    def conv(self, op, x, res=None, fault=None, fault_scale=None, ds=None):
        """(v before the ReLU in engine units, mag, K). ds: (op, its input codes) summed into the output."""
        w, alpha, bias, stride, pad, K = self.weights(op, x, fault, fault_scale)
        v, mag = F.conv2d(x, w, None, stride, pad), F.conv2d(x.abs(), w.abs(), None, stride, pad)
        if alpha is not None:
            v, mag = v * alpha.view(1, -1, 1, 1), mag * alpha.abs().view(1, -1, 1, 1)
        v, mag = v + bias.view(1, -1, 1, 1), mag + bias.abs().view(1, -1, 1, 1)
        if ds is not None:
            dv, dmag, dK = self.conv(ds[0], ds[1])
            if fault == "ds_bias":
                dv = dv - self.weights(ds[0], ds[1])[2].view(1, -1, 1, 1)
            v, mag, K = v + dv, mag + dmag, K + dK
        if res is not None:
            a_res = self.view.acts[op[3]]
            rs = float(_f32(self.view.acts[op[2]].scale if fault == "res_scale" else a_res.scale)) \
                if self.rounded and a_res.fp8 else 1.0
            v, mag = v + res * rs, mag + res.abs() * rs
        return v, mag, K

    def finish(self, op, v, mag, K, fault=None, extra=None):
        """The stored output of op: Out in its own units. extra: a slack in engine units added to the bar."""
        name, _, o, _ = op
        a = self.view.acts[o]
        r = torch.relu(v) if self.sem.relu(name) and fault != "relu" else v
        if not self.rounded:
            return Out(o, r, torch.zeros_like(r), kb.L2_BF16)
        if a.fp8:
            inv = inv_scale(a)
            bar = e4m3_bar(r * inv, mag, K, inv)
            return Out(o, r * inv, bar if extra is None else bar + extra * inv, kb.L2_E4M3)
        bar = kb.bound(r, mag, K, out_bf16=not a.f32)
        return Out(o, r, bar if extra is None else bar + extra, kb.L2_BF16)

    def check_res(self, op):
        assert (op[3] >= 0) == self.sem.has_res(op[0]), f"{op[0]}: the residual does not follow the block rule"

    def single(self, op, x=None, **fault):
        self.check_res(op)
        x = self.acts(op[1]) if x is None else x
        res = self.acts(op[3]) if op[3] >= 0 else None
        ds = fault.pop("ds", None)
        v, mag, K = self.conv(op, x, res, ds=ds, **fault)
        return self.finish(op, v, mag, K, fault.get("fault"))

    # ------------------------------------------------------------ a plan step
    def step(self, i, fault=None, fault_scale=None):
        """[Out] of every activation step i stores (logits included)."""
        st = self.view.step(i)
        k, ops = st["kernel"], st["ops"]
        by_name = lambda n: self.view.ops[self.view.index[n]]
        fk = dict(fault=fault, fault_scale=fault_scale)
        if k in UNAUDITED:
            return []
        if k in SINGLE:
            op = ops[0]
            x = self.acts(op[1])
            assert not (st["ds"] and st["dsk"])
            if st["pool"]:
                assert not st["ds"] and not st["dsk"]
                self.check_res(op)
                v, mag, K = self.conv(op, x, self.acts(op[3]) if op[3] >= 0 else None, **fk)
                y = self.finish(op, v, mag, K, fault)
                pop = by_name(st["pool"])
                assert pop[1] == op[2] and not self.view.acts[op[2]].fp8
                if len(ops) == 2:  # the max-pool that follows the conv is the step's last op: y is never stored
                    assert ops[1] == pop
                    return [self.maxpooled(pop, y)]
                outs = [y] if st["store_y"] else []
                assert len(ops) == 1 and self.sem.resnet and pop[0] == "avgpool"
                n, C, H, W = y.ref.shape
                flat = lambda t: kb.nhwc(t).reshape(n, H * W, C)
                ref = flat(y.ref).mean(1)
                return outs + [Out(pop[2], ref.view(n, C, 1, 1),
                                   kb.avgpool_bound(flat(y.ref), flat(y.bar), H * W).view(n, C, 1, 1), kb.L2_BF16)]
            assert len(ops) == 1, (k, ops)
            if st["dsk"]:  # the downsample as more K steps: the residual is never stored
                d = by_name(st["dsk"])
                assert op[3] == d[2], f"{op[0]}: its residual is not {d[0]}'s output"
                assert self.sem.has_res(op[0])
                v, mag, K = self.conv(op, x, None, ds=(d, self.acts(d[1])), **fk)
                return [self.finish(op, v, mag, K, fault)]
            outs = [self.single(op, x, **fk)]
            if st["ds"]:
                d = by_name(st["ds"])
                assert d[1] == op[1], f"{d[0]} does not read {op[0]}'s input"
                if fault == "ds_bias":
                    v, mag, K = self.conv(d, x)
                    outs.append(self.finish(d, v - self.weights(d, x)[2].view(1, -1, 1, 1), mag, K))
                else:
                    outs.append(self.single(d, x, **fk))
            return outs
        if k in ("StemPoolU8", "StemPool", "AlexStem"):
            cop = ops[-1] if k != "AlexStem" else ops[1]
            v, mag, K = self.conv(cop, self.x0, **fk)
            if k == "StemPoolU8":
                K = 154  # the dense-K order: 7 windows of 22 products, 7 of them on zero weights
            y = self.finish(cop, v, mag, K, fault)
            return [self.maxpooled(ops[-1], y)]
        if k == "Block":
            c1, c2 = ops
            assert c2[1] == c1[2] and c2[3] == c1[1] and self.sem.has_res(c2[0]) and self.sem.relu(c1[0])
            x = self.acts(c1[1])
            w1, _, b1, _, p1, K1 = self.weights(c1, x)
            w2, _, b2, _, p2, K2 = self.weights(c2, x)
            v, bar, _, _ = kb.chain(x, [(w1, b1, K1, p1), (w2, b2, K2, p2)], res=x)
            r = v if fault == "relu" else torch.relu(v)
            return [Out(c2[2], r, bar, kb.L2_BF16)]
        if k == "Bottleneck56Head":
            c1, c2 = ops
            assert c2[1] == c1[2] and c1[3] < 0 and c2[3] < 0 and self.sem.relu(c1[0])
            x = self.acts(c1[1])
            w1, _, b1, _, p1, K1 = self.weights(c1, x)
            w2, _, b2, _, p2, K2 = self.weights(c2, x)
            v, bar, _, _ = kb.chain(x, [(w1, b1, K1, p1), (w2, b2, K2, p2)])
            return [Out(c2[2], v if fault == "relu" else torch.relu(v), bar, kb.L2_BF16)]
        if k == "Bottleneck56":
            c1, c2, c3 = ops
            acts = self.view.acts
            assert c2[1] == c1[2] and c3[1] == c2[2] and c3[3] == c1[1] and self.sem.has_res(c3[0])
            assert acts[c1[1]].fp8 and acts[c3[2]].fp8 and not acts[c1[2]].fp8 and not acts[c2[2]].fp8
            x = self.acts(c1[1])
            w1, a1, b1, _, _, _ = self.weights(c1, x, **fk)
            w2, _, b2, _, _, _ = self.weights(c2, x)
            w3, _, b3, _, _, _ = self.weights(c3, x)
            o = dict(x=x, w1=w1, a1=a1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3,
                     res_scale=acts[c3[2]].scale if fault == "res_scale" else acts[c1[1]].scale,
                     out_scale=acts[c3[2]].scale)
            w3s, b3s, res = kb.bottleneck_last(o)
            # (kb.chain with e4m3_bar in place of kb.e4m3_bound's range check)
            v, _, deltas, ts = kb.chain(x, [(w1, b1, 256, 0), (w2, b2, 576, 1), (w3s, b3s, 64, 0)], alpha=a1, res=res)
            _, mag = kb.conv_ref(ts[1], w3s, b3s, 1, 0, res=res)
            r = v if fault == "relu" else torch.relu(v)
            bar = e4m3_bar(r, mag, 64, 1.0) + F.conv2d(deltas[1], w3s.abs())
            return [Out(c3[2], r, bar, kb.L2_E4M3)]
        if k == "Conv1x1Chain":  # the reduce conv reads the expand conv's stored output (its LDS copy)
            c3, c1 = ops
            assert c1[1] == c3[2]
            y = self.single(c3, **fk)
            a = self.view.acts[c3[2]]
            return [y, self.single(c1, store(self.single(c3), a.fp8, a.f32) if self.ideal else None)]
        if k == "MaxPool":
            op = ops[0]
            x = self.acts(op[1])
            return [self.maxpooled(op, Out(op[1], x, torch.zeros_like(x), kb.L2_BF16))]
        if k == "AvgPoolGlobal":
            op = ops[0]
            return [self.avgpool(op)]
        if k == "QuantE4m3":
            op = ops[0]
            x = self.acts(op[1])
            inv = inv_scale(self.view.acts[op[2]])
            return [Out(op[2], x * inv, e4m3_bar(x * inv, x.abs(), 1, inv), kb.L2_E4M3)]
        if k == "HeadPooled":  # fc on the stored pooled rows, then softmax / top-1
            assert [o[0] for o in ops[1:]] == ["softmax_top1"]
            return [self.single(ops[0], **fk)]
        if k == "HeadFused":  # avgpool, fc, softmax / top-1: the pooled row is rounded to bf16 on chip
            pop, fop = ops[0], ops[1]
            assert fop[1] == pop[2] and [o[0] for o in ops[2:]] == ["softmax_top1"]
            p = self.avgpool(pop)
            w, _, bias, _, _, K = self.weights(fop, p.ref)
            v, _ = kb.fc_ref(p.ref.flatten(1), w.flatten(1), bias)
            a_in = self.view.acts[pop[1]]
            xa = self.acts(pop[1]).abs().mean((2, 3)) * (float(_f32(a_in.scale)) if a_in.fp8 else 1.0)
            _, mag = kb.fc_ref(xa, w.flatten(1), bias)
            bar = kb.head_bound(mag, K) if self.rounded else torch.zeros_like(v)
            # (the logits carry the pooled row's bf16 rounding through an fc that cancels, mag >> |v|: no fixed
            # relative L2 follows from that. With the norm of the element-wise bar as the limit the relative-L2
            # check is vacuous for this kernel: whatever meets the element-wise bar meets it. The element-wise
            # bar is the check here.)
            l2 = max(kb.L2_BF16, (bar.norm() / v.norm()).item())
            return [Out(fop[2], v.view(*v.shape, 1, 1), bar.view(*v.shape, 1, 1), l2)]
        if k == "SoftmaxTop1":
            return []  # idx / prob: judged against the logits by the caller
        raise AssertionError(f"no reference for kernel {k}")

    def maxpooled(self, pop, y):
        """A max-pool of the (unrounded) conv output y: kb.assert_close_pooled's first comparison."""
        ks, s, pad = self.sem.pool(pop[0])
        return Out(pop[2], kb.maxpool(y.ref, ks, s, pad), kb.maxpool(y.bar, ks, s, pad), y.l2)

    def avgpool(self, op):
        """The global average of a stored activation as bf16: an HW-term fp32 sum (one more product for an e4m3
        input's scale) and the output rounding."""
        assert self.sem.resnet and op[0] == "avgpool"
        a = self.view.acts[op[1]]
        x = self.acts(op[1]) * (float(_f32(a.scale)) if self.rounded and a.fp8 else 1.0)
        ref = x.mean((2, 3), keepdim=True)
        if not self.rounded:
            return Out(op[2], ref, torch.zeros_like(ref), kb.L2_BF16)
        HW = x.shape[2] * x.shape[3]
        return Out(op[2], ref, kb.EPS_OUT * ref.abs() + (HW + 1) * kb.EPS_SUM * x.abs().mean((2, 3), keepdim=True),
                   kb.L2_BF16)


def judge(got, out, fp8, what):
    """(got, ref, bar, left-out share) restricted to the elements the bar judges: an e4m3 element surely past 448
    must be the saturated code, one that may or may not saturate is left out."""
    ref, bar = out.ref, out.bar
    if not fp8:
        return got, ref, bar, 0.0
    a = ref.abs()
    sat = a - bar >= kb.E4M3_MAX
    unsure = (a + bar >= kb.E4M3_MAX) & ~sat
    share = unsure.double().mean().item()
    print(f"{what}: {share:.4%} left out at the edge of e4m3's range, {sat.double().mean().item():.4%} saturated")
    keep = ~unsure
    ref = torch.where(sat, ref.sign() * kb.E4M3_MAX, ref)
    bar = torch.where(sat, torch.zeros_like(bar), bar)
    return got[keep], ref[keep], bar[keep], share


def store(out, fp8, f32=False):
    """The reference rounded to its storage type: what an ideal engine stores (codes, float64)."""
    if fp8:
        return out.ref.clamp(-kb.E4M3_MAX, kb.E4M3_MAX).float().to(FP8).double()
    return out.ref.float().double() if f32 else kb.bf16r(out.ref)


def rejected(ref, i, outs, acts, fault, what):
    """The largest |got - wrong| / bar over the activations step i stores, for the reference with `fault`: above
    1 the bar sees the fault. outs: the step's good [Out]; acts(id): what the engine stored. Only the elements
    `judge` holds to the bar of the good reference count: an e4m3 element that is surely saturated, or may be, is
    off its unclamped reference with no fault at all."""
    ratio = 0.0
    for g, w in zip(outs, ref.step(i, **fault)):
        keep = torch.ones_like(g.bar, dtype=torch.bool)
        if ref.view.acts[g.act].fp8:
            keep = g.ref.abs() + g.bar < kb.E4M3_MAX
        if bool(keep.any()):
            ratio = max(ratio, kb.worst(acts(g.act)[keep], w.ref[keep], g.bar[keep])[0])
    print(f"{what}: control |err|/bound {ratio:.1f}")
    assert ratio > 1.0, f"{what}: the bar does not see this fault ({ratio})"
    return ratio


def _apart(a, b):
    """Two scales at least one e4m3 step (2^-3 of the value) apart."""
    return max(a, b) / min(a, b) >= 1.0 + 2.0 ** -3


def controls(view, sem):
    """{label: (step index, fault keywords)}: for each modelled plumbing fault the first step of the plan where it
    applies. The two scales a fault confuses must be an e4m3 step apart (`_apart`): steps where they are not are
    passed over."""
    found = {}
    for i in range(len(view.plan)):
        st = view.step(i)
        k, ops, acts = st["kernel"], st["ops"], view.acts
        if k not in SINGLE and k not in ("Bottleneck56", "Conv1x1Chain", "Block"):
            continue
        first, last = ops[0], ops[2] if k == "Bottleneck56" else ops[0]
        if k in SINGLE and not st["dsk"] or k in ("Bottleneck56", "Conv1x1Chain"):
            if last[3] >= 0 and acts[last[3]].fp8 and _apart(acts[last[3]].scale, acts[last[2]].scale):
                found.setdefault("residual with the output's scale", (i, dict(fault="res_scale")))
        a_in = acts[first[1]]
        if a_in.fp8 and a_in.cscale is None:
            other = [acts[j].scale for j in (first[2], first[3]) if j >= 0 and acts[j].fp8 and acts[j].cscale is None
                     and _apart(acts[j].scale, a_in.scale)]
            if other:
                found.setdefault("alpha from another activation's scale", (i, dict(fault="alpha", fault_scale=other[0])))
        if a_in.fp8 and a_in.cscale is not None and k in SINGLE:
            found.setdefault("cscale along N", (i, dict(fault="cscale_n")))
        if sem.relu(last[0]) and (k in SINGLE or k == "Block"):
            found.setdefault("ReLU dropped", (i, dict(fault="relu")))
        if st["dsk"] or st["ds"]:
            found.setdefault("downsample bias left out", (i, dict(fault="ds_bias")))
        if isinstance(sem.module(first[0]), nn.Linear) and a_in.H * a_in.W > 1:
            found.setdefault("fc read in NCHW order", (i, dict(fault="nchw")))
    return found

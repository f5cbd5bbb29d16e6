#!/usr/bin/env python3
"""conv1x1_small against what the default plan runs for ResNet50's 1x1 convs
at query batches, and resnet50 / resnet50_fp8 with EngineOptions::small_1x1 on
and off -> profiles/small1x1.txt.

  python tools/small1x1_bench.py [--out profiles/small1x1.txt] [--max-b 32]

Per launch (B = 1 and 4): InferenceEngine.profile (one hipEvent pair per plan
step of an eager forward, so every kernel reads the operands, types and cache
state it has inside a forward; an Igemm step's time includes its splitk_reduce)
of an engine with the option on and one with it off, in turn ROUNDS times;
medians with [fastest .. slowest]. Layers of one geometry and type form are
one line (their times pooled). A step of several ops (Bottleneck56*,
Conv1x1Chain) is compared with the sum of the "on" steps of the same ops.

Per forward: REPS replays of the engine's own graph per round, host-launched,
"on" and two "off" engines in turn (the two give the run-to-run spread), over
B = 1 .. --max-b with the planner's bound raised through small_1x1_set_max_b.
resnet50_fp8 runs with small_conv8 on both sides.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import dmlc  # noqa: E402
from dmlc.models import state_dict_f32  # noqa: E402
from dmlc.models.calibrated import calibrated, mixed_images  # noqa: E402
from dmlc.runtime import InferenceEngine  # noqa: E402

ROUNDS, REPS = 15, 50
LINES = []
ARCHS = {"resnet50": {}, "resnet50_fp8": {"small_conv8": True}}


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def med(t):
    return f"{statistics.median(t):8.2f} us [{min(t):.2f} .. {max(t):.2f}]"


def timed(run, per):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / per


def per_launch(arch, sd, dev, B):
    on = InferenceEngine(arch, sd, max_batch=B, options={**ARCHS[arch], "small_1x1": True})
    off = InferenceEngine(arch, sd, max_batch=B, options=ARCHS[arch])
    img = mixed_images(B, seed=70 + B).to(dev)
    for e in (on, off):
        e.profile(img)
    t_on, t_off = {}, {}
    for _ in range(ROUNDS):
        for e, t in ((on, t_on), (off, t_off)):
            for name, ms in e.profile(img):
                t.setdefault(name, []).append(ms * 1e3)
    p_on, p_off = on._e.plan(B, 224, 224), off._e.plan(B, 224, 224)
    names = [k[1] for k in p_on if k[0] != "None"]
    shape = {}  # layer -> geometry of its weights and stride, as text
    for k, first, _, detail in p_on:
        if k == "Small1x1":
            w = sd[first + ".weight"]
            s2 = "downsample" in first
            shape[first] = f"{w.shape[1]:4d} -> {w.shape[0]:4d}{' s2' if s2 else '   '} {detail}"
    # the default plan's steps that hold a Small1x1 layer, with the "on" steps of the same ops
    order = [k[1] for k in p_on]
    rows = {}
    for k, first, n, _ in p_off:
        members = order[order.index(first):order.index(first) + n] if first in order else [first]
        if k == "None" or first not in t_off or not any(m in shape for m in members):
            continue
        key = (k, " + ".join(shape.get(m, "(3x3)") for m in members) if n > 1 else shape[first], _hw(first))
        r = rows.setdefault(key, ([], [], []))
        r[0].append(first)
        r[1].extend(t_off[first])
        on_sum = [sum(t_on[m][i] for m in members if m in t_on) for i in range(ROUNDS)]
        r[2].extend(on_sum)
    say(f"## {arch} B={B}: default plan's step against the small_1x1 plan's step(s) for the same ops")
    for (k, geom, hw), (layers, a, b) in rows.items():
        say(f"{hw:>5s} {geom:44s} x{len(layers):<2d} {k:16s} {med(a)}   Small1x1 {med(b)}   "
            f"ratio {statistics.median(b) / statistics.median(a):.3f}")
    tot = lambda t, p: statistics.median([sum(t[k[1]][i] for k in p if k[0] != "None" and k[1] in t)
                                          for i in range(ROUNDS)])
    l1 = lambda t, p: statistics.median([sum(t[k[1]][i] for k in p if k[1].startswith("layer1.") and k[1] in t)
                                         for i in range(ROUNDS)])
    say(f"      sum of all steps: off {tot(t_off, p_off):.1f} us, on {tot(t_on, p_on):.1f} us; layer1's steps: "
        f"off {l1(t_off, p_off):.1f} us, on {l1(t_on, p_on):.1f} us ({len(names)} launches on)")


def _hw(layer):
    if layer.startswith("layer1") or layer.startswith("layer2.0.conv1") or layer.startswith("layer2.0.down"):
        return "56x56"
    if layer.startswith("layer2") or layer.startswith("layer3.0.conv1") or layer.startswith("layer3.0.down"):
        return "28x28"
    if layer.startswith("layer3") or layer.startswith("layer4.0.conv1") or layer.startswith("layer4.0.down"):
        return "14x14"
    return "7x7"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "small1x1.txt"))
    ap.add_argument("--max-b", type=int, default=32, help="the Small1x1 path's batch bound for the forward sweep")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("small1x1_bench needs a GPU")
    C, dev = dmlc.native(), torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    say(f"# python tools/small1x1_bench.py   ({torch.cuda.get_device_name(0)}, {cus} CUs)")
    say(f"# per launch: medians of {ROUNDS} interleaved eager profile() forwards, one event pair per step; "
        f"[fastest .. slowest]; 1x1 input size, Cin -> N, stride, picked tile, layers pooled")
    sd = state_dict_f32(calibrated("resnet50", seed=11))
    C.small_1x1_set_max_b(a.max_b)
    for arch in ARCHS:
        for B in (1, 4):
            per_launch(arch, sd, dev, B)
    say()
    say(f"# forwards: medians of {ROUNDS} interleaved rounds of {REPS} graph replays (predict(), 224x224 u8 images); "
        f"small_1x1 on with the batch bound raised to {a.max_b} (kSmall1x1MaxB = {C.kSmall1x1MaxB}); two off engines")
    batches = [b for b in (1, 2, 4, 8, 16, 32) if b <= a.max_b]
    wins = {}
    for arch, base in ARCHS.items():
        engines = [("off", InferenceEngine(arch, sd, max_batch=batches[-1], options=base)),
                   ("off again", InferenceEngine(arch, sd, max_batch=batches[-1], options=base)),
                   ("small_1x1", InferenceEngine(arch, sd, max_batch=batches[-1], options={**base, "small_1x1": True}))]
        for B in batches:
            img = mixed_images(B, seed=70 + B).to(dev)
            ts = {}
            runs = []
            for name, e in engines:
                out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
                e.predict(img, out=out)
                torch.cuda.synchronize()
                runs.append((name, lambda e=e, out=out, img=img: [e.predict(img, out=out) for _ in range(REPS)]))
            for _ in range(ROUNDS):
                for name, run in runs:
                    ts.setdefault(name, []).append(timed(run, REPS))
            m = {n: statistics.median(t) for n, t in ts.items()}
            fast_off, spread = min(m["off"], m["off again"]), abs(m["off"] - m["off again"])
            wins[(arch, B)] = fast_off - m["small_1x1"] > spread
            say(f"{arch + ' forward B=' + str(B):28s} " + "   ".join(f"{n} {med(t)}" for n, t in ts.items()) +
                f"   on / faster off = {m['small_1x1'] / fast_off:.3f} (off spread {spread:.2f} us)"
                f"{'' if wins[(arch, B)] else '   NOT faster'}")
    C.small_1x1_set_max_b(0)
    for arch in ARCHS:
        upto = 0
        for B in batches:
            if not wins[(arch, B)]:
                break
            upto = B
        say(f"# {arch}: small_1x1 on beats the faster off run by more than the off spread at every swept B up to {upto} "
            f"(0: not even at B = 1)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

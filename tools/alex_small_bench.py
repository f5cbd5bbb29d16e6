#!/usr/bin/env python3
"""conv_smallk against conv5x5_27 / conv3x3_13 at query batches, and AlexNet
with EngineOptions::small_alex on and off -> profiles/alex_small.txt.

  python tools/alex_small_bench.py [--out profiles/alex_small.txt] [--max-b 64]

Per kernel, at B = 1 and 4: AlexNet's four stride-1 feature convs, with the
max-pool where the engine fuses it, on conv_smallk (one launch spread over the
CUs; the un-pooled forms at every mf, the picked one marked) against the
one-workgroup-per-image kernel of conv_direct.hip on the same operands.
And the fused u8 stem on alex_stem_rows (one workgroup per pooled row) against
alex_stem (one per image). Per forward: alexnet at B = 1 .. 64 with the option off, on (the planner's
batch bound raised to --max-b through small_alex_set_max_b for this sweep), and
a second engine with it off: the distance between the two "off" columns is the
spread a gain has to exceed.

Method: tools/small8_bench.py's (graphs of back-to-back launches over rotating
weight copies, > 512 MB together, the forms replayed in turn, device events,
median and fastest / slowest round).
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from small8_bench import LAUNCHES, LINES, REPS, ROUNDS, compare, graph_of, say  # noqa: E402

import dmlc  # noqa: E402
from dmlc import ops  # noqa: E402
from dmlc.models import state_dict_f32  # noqa: E402
from dmlc.models.calibrated import calibrated, mixed_images  # noqa: E402
from dmlc.runtime import InferenceEngine  # noqa: E402

LAYERS = [  # (name, H, CI, CO, ks, pad, pool)
    ("features.3+5", 27, 64, 192, 5, 2, True), ("features.6", 13, 192, 384, 3, 1, False),
    ("features.8", 13, 384, 256, 3, 1, False), ("features.10+12", 13, 256, 256, 3, 1, True)]


def kernel_pair(C, dev, cus, name, H, CI, CO, ks, pad, pool, B):
    g = torch.Generator().manual_seed(H + CI + B)
    x = torch.randn(B, H, H, CI, generator=g).bfloat16().to(dev)
    Ho = (H - 3) // 2 + 1 if pool else H
    y = torch.empty(B, Ho, Ho, CO, dtype=torch.bfloat16, device=dev)
    copies = -(-(512 << 20) // (CO * ks * ks * CI * 2))
    wf0 = ops.stream_weight_frag((torch.randn(CO, ks * ks * CI, generator=g) / (ks * ks * CI) ** 0.5).bfloat16().to(dev))
    wf = [wf0.clone() for _ in range(copies)]
    bias, zero = torch.zeros(CO, device=dev), torch.zeros(64, device=dev)
    cur = lambda: torch.cuda.current_stream().cuda_stream
    yp = y.data_ptr() if pool else 0

    def direct(i):
        if ks == 5:
            C.conv5x5_27(x.data_ptr(), wf[i].data_ptr(), bias.data_ptr(), y.data_ptr(), zero.data_ptr(), B, cur(), yp)
        else:
            C.conv3x3_13(x.data_ptr(), wf[i].data_ptr(), bias.data_ptr(), y.data_ptr(), zero.data_ptr(), B, CI, CO, True,
                         cur(), yp)

    def small(mf):
        return lambda i: C.conv_smallk(x.data_ptr(), wf[i].data_ptr(), bias.data_ptr(), y.data_ptr(), B, H, H, CI, CO,
                                       ks, pad, True, pool, mf, cur())

    pick = C.conv_smallk_pick_mf(B, H, H, CI, CO, ks, cus)
    forms = [("direct", graph_of(direct, copies).replay)]
    for mf in ([1] if pool else [1, 2, 4]):
        tag = "conv_smallk pool" if pool else f"conv_smallk mf={mf}" + ("*" if mf == pick else "")
        forms.append((tag, graph_of(small(mf), copies).replay))
    compare(f"{name} B={B}", forms, LAUNCHES)


def stem_pair(C, dev, B):
    g = torch.Generator().manual_seed(B)
    img = torch.randint(0, 256, (B, 224, 224, 3), generator=g, dtype=torch.uint8).to(dev)
    w = ops.pack_alex_stem_weight(torch.randn(64, 3, 11, 11, generator=g) / 363 ** 0.5, device=dev)
    bias, y = torch.zeros(64, device=dev), torch.empty(B, 27, 27, 64, dtype=torch.bfloat16, device=dev)
    cur = lambda: torch.cuda.current_stream().cuda_stream
    forms = [(n, graph_of(lambda i, f=f: f(img.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), B, cur()), 1)
              .replay) for n, f in (("alex_stem", C.alex_stem_u8), ("alex_stem_rows", C.alex_stem_rows_u8))]
    compare(f"features.0-2 B={B}", forms, LAUNCHES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "alex_small.txt"))
    ap.add_argument("--max-b", type=int, default=64, help="the SmallK path's batch bound for the forward sweep")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("alex_small_bench needs a GPU")
    C, dev = dmlc.native(), torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    say(f"# python tools/alex_small_bench.py   ({torch.cuda.get_device_name(0)}, {cus} CUs)")
    say(f"# kernels: medians of {ROUNDS} interleaved rounds of {LAUNCHES} graph-captured launches over weight copies "
        f"> 512 MB; [fastest .. slowest round]; * = conv_smallk_pick_mf's choice")
    for B in (1, 4):
        stem_pair(C, dev, B)
    for layer in LAYERS:
        for B in (1, 4):
            kernel_pair(C, dev, cus, *layer, B)

    say()
    say(f"# forwards: medians of {ROUNDS} interleaved rounds of {REPS} graph replays (predict(), 224x224 u8 images); "
        f"small_alex on with the batch bound raised to {a.max_b} (kSmallAlexMaxB = {C.kSmallAlexMaxB}); "
        f"'off again' = a second engine with default options")
    batches = [b for b in (1, 2, 4, 8, 16, 32, 64) if b <= a.max_b]
    C.small_alex_set_max_b(a.max_b)
    sd = state_dict_f32(calibrated("alexnet", seed=11))
    engines = [("off", InferenceEngine("alexnet", sd, max_batch=batches[-1])),
               ("small_alex", InferenceEngine("alexnet", sd, max_batch=batches[-1], options={"small_alex": True})),
               ("off again", InferenceEngine("alexnet", sd, max_batch=batches[-1]))]
    upto, open_ = 0, True
    for B in batches:
        img = mixed_images(B, seed=70 + B).to(dev)
        forms = []
        for name, e in engines:
            out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
            e.predict(img, out=out)
            torch.cuda.synchronize()
            forms.append((name, lambda e=e, out=out, img=img: [e.predict(img, out=out) for _ in range(REPS)]))
        med = compare(f"alexnet forward B={B}", forms, REPS)
        spread = abs(med[2] - med[0])
        gain = min(med[0], med[2]) - med[1]
        say(f"{'':28s} small_alex gains {gain:+.1f} us on the faster 'off' run; spread of the two 'off' runs "
            f"{spread:.1f} us")
        open_ = open_ and gain > spread
        if open_:
            upto = B
    C.small_alex_set_max_b(0)
    say(f"# small_alex on is faster than off by more than the spread at every swept B up to {upto}"
        if upto else "# small_alex on is not faster than off by more than the spread at B = 1")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

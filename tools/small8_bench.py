#!/usr/bin/env python3
"""conv_small8 against the e4m3 implicit GEMM at query batches, and the fp8
ResNets with EngineOptions::small_conv8 on and off -> profiles/small8.txt.

  python tools/small8_bench.py [--out profiles/small8.txt] [--max-b 32]

Per kernel: the ten e4m3 3x3 forms of resnet18_fp8 / resnet34_fp8 /
resnet50_fp8 at B = 1 and 4, conv_small8 (one launch, the picked mf) against
conv2d_igemm's e4m3 path on the same operands (the DS form: the 3x3 and the
1x1/s2 downsample, two launches). Per forward: the three fp8 models at B = 1 ..
32 with the option on (the planner's batch bound raised to --max-b through
small_conv8_set_max_b for this sweep) and off, and the bf16 model of the same
depth at B = 1.

Method (tools/fc8_bench.py's): a hipGraph of LAUNCHES back-to-back launches on
preallocated buffers that walk COPIES copies of the weights, together > 512 MB,
so every launch streams its weights from HBM as inside a forward; the two forms
replayed in turn ROUNDS times, timed by device events; reported: the median
per-launch time and the fastest / slowest round. Forwards: REPS replays of the
engine's own graph per round, host-launched (at B = 1 the host's launch rate
can be what is measured).
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import dmlc  # noqa: E402
from dmlc import ops  # noqa: E402
from dmlc.models import state_dict_f32  # noqa: E402
from dmlc.models.calibrated import calibrated, mixed_images  # noqa: E402
from dmlc.runtime import InferenceEngine  # noqa: E402

LAUNCHES, ROUNDS, REPS = 48, 15, 50
LINES = []
FORMS = [  # (name, H, CI, CO, stride, res, ds)
    ("28x128 s1", 28, 128, 128, 1, False, False), ("14x256 s1", 14, 256, 256, 1, False, False),
    ("14x256 s1 RES", 14, 256, 256, 1, True, False), ("7x512 s1", 7, 512, 512, 1, False, False),
    ("7x512 s1 RES", 7, 512, 512, 1, True, False), ("56x128 s2", 56, 128, 128, 2, False, False),
    ("28x256 s2", 28, 256, 256, 2, False, False), ("14x512 s2", 14, 512, 512, 2, False, False),
    ("14x256->512 s2", 14, 256, 512, 2, False, False), ("14x256->512 s2 DS", 14, 256, 512, 2, False, True)]


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def graph_of(launch, copies):
    """A captured graph of LAUNCHES calls launch(i % copies), warmed up first."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for i in range(copies):
            launch(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(LAUNCHES):
            launch(i % copies)
    g.replay()
    torch.cuda.synchronize()
    return g


def timed(run, per):
    """us per unit of one run() that does `per` units."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / per


def compare(what, forms, per):
    """forms: [(name, run)], replayed in turn; one line with each one's median [fastest .. slowest].
    Returns the medians."""
    ts = {n: [] for n, _ in forms}
    for _ in range(ROUNDS):
        for n, run in forms:
            ts[n].append(timed(run, per))
    med = [statistics.median(t) for t in ts.values()]
    parts = [f"{n} {statistics.median(t):8.2f} us [{min(t):.2f} .. {max(t):.2f}]" for n, t in ts.items()]
    ratio = f"   {list(ts)[1]} / {list(ts)[0]} = {med[1] / med[0]:.3f}" if len(med) == 2 else ""
    say(f"{what:28s} " + "   ".join(parts) + ratio)
    return med


def kernel_pair(C, dev, cus, name, H, CI, CO, S, res, ds, B):
    g = torch.Generator().manual_seed(H + CI + B)
    codes = lambda *s: torch.randint(0, 120, s, generator=g, dtype=torch.uint8).to(dev)  # finite e4m3 bytes
    Ho = H // S
    x, y, yd = codes(B, H, H, CI), codes(B, Ho, Ho, CO), codes(B, Ho, Ho, CO)
    r = codes(B, Ho, Ho, CO) if res else None
    copies = -(-(512 << 20) // (CO * 9 * CI))
    w0 = codes(CO, 9 * CI)
    wf0 = ops.stream8_weight_frag(w0, CO)
    w = [w0.clone() for _ in range(copies)]    # row-major for the implicit GEMM
    wf = [wf0.clone() for _ in range(copies)]  # the same weights in fragment order
    wd = codes(CO, CI)
    wdf = ops.stream8_weight_frag(wd, CO)
    alpha, bias = torch.full((CO,), 1e-4, device=dev), torch.zeros(CO, device=dev)
    zero = torch.zeros(64, device=dev)
    mf = C.conv_small8_pick_mf(B, H, H, CI, CO, S, ds, cus)
    extra = dict(res=r.data_ptr(), res_scale=0.01) if res else {}
    if ds:
        extra = dict(wd=wdf.data_ptr(), alpha_d=alpha.data_ptr(), bias_d=bias.data_ptr(), yd=yd.data_ptr(),
                     out_inv_scale_d=1.0)
    cur = lambda: torch.cuda.current_stream().cuda_stream

    def small(i):
        C.conv_small8(x.data_ptr(), wf[i].data_ptr(), alpha.data_ptr(), bias.data_ptr(), y.data_ptr(), zero.data_ptr(),
                      B, H, H, CI, CO, S, True, 1.0, mf, cur(), **extra)

    def gemm(wt, out, k, pad, K, relu, rp):
        C.conv2d(x=x.data_ptr(), w=wt.data_ptr(), bias=bias.data_ptr(), res=rp, y=out.data_ptr(), B=B, H=H, W=H, Cin=CI,
                 KH=k, KW=k, stride=S, pad=pad, N=CO, Npad=CO, Kpad=K, ldo=CO, relu=relu, out_f32=False, split_k=1,
                 ws=0, tile=-1, zero=zero.data_ptr(), stem=False, Ho=Ho, Wo=Ho, max_blocks=0, stream=cur(), in_fp8=True,
                 out_fp8=True, alpha=alpha.data_ptr(), res_scale=0.01, out_inv_scale=1.0, num_cus=cus, x2=0, cin2=0)

    def igemm(i):
        gemm(w[i], y, 3, 1, 9 * CI, True, r.data_ptr() if res else 0)
        if ds:
            gemm(wd, yd, 1, 0, CI, False, 0)

    small(0)
    ys = y.clone()
    igemm(0)
    torch.cuda.synchronize()
    same = (ys == y).float().mean().item()  # (summation order differs: a few bytes may)
    gs, gi = graph_of(small, copies), graph_of(igemm, copies)
    compare(f"{name} B={B} mf={mf}", [("igemm", gi.replay), ("conv_small8", gs.replay)], LAUNCHES)
    say(f"{'':28s} output bytes equal to the implicit GEMM's: {100 * same:.2f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "small8.txt"))
    ap.add_argument("--max-b", type=int, default=32, help="the Small8 path's batch bound for the forward sweep")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("small8_bench needs a GPU")
    C, dev = dmlc.native(), torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    say(f"# python tools/small8_bench.py   ({torch.cuda.get_device_name(0)}, {cus} CUs)")
    say(f"# kernels: medians of {ROUNDS} interleaved rounds of {LAUNCHES} graph-captured launches over weight copies "
        f"> 512 MB; [fastest .. slowest round]")
    for form in FORMS:
        for B in (1, 4):
            kernel_pair(C, dev, cus, *form, B)

    say()
    say(f"# forwards: medians of {ROUNDS} interleaved rounds of {REPS} graph replays (predict(), 224x224 u8 images); "
        f"small_conv8 on with the batch bound raised to {a.max_b} (kSmallConv8MaxB = {C.kSmallConv8MaxB})")
    batches = [b for b in (1, 2, 4, 8, 16, 32) if b <= a.max_b]
    C.small_conv8_set_max_b(a.max_b)
    wins = {}
    for arch in ("resnet18", "resnet34", "resnet50"):
        sd = state_dict_f32(calibrated(arch, seed=11))
        engines = [("off", InferenceEngine(arch + "_fp8", sd, max_batch=batches[-1])),
                   ("small_conv8", InferenceEngine(arch + "_fp8", sd, max_batch=batches[-1],
                                                   options={"small_conv8": True})),
                   (arch + " bf16", InferenceEngine(arch, sd, max_batch=1))]
        for B in batches:
            img = mixed_images(B, seed=70 + B).to(dev)
            forms = []
            for name, e in engines[:3 if B == 1 else 2]:
                out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
                e.predict(img, out=out)
                torch.cuda.synchronize()
                forms.append((name, lambda e=e, out=out, img=img: [e.predict(img, out=out) for _ in range(REPS)]))
            med = compare(f"{arch}_fp8 forward B={B}", forms, REPS)
            wins[(arch, B)] = med[1] < med[0]
            if B == 1:
                say(f"{'':28s} {arch}_fp8 with small_conv8 / {arch} bf16 at B = 1: {med[1] / med[2]:.3f} "
                    f"({med[1] - med[2]:+.1f} us)")
    C.small_conv8_set_max_b(0)
    upto = 0
    for B in batches:
        if not all(wins[(arch, B)] for arch in ("resnet18", "resnet34", "resnet50")):
            break
        upto = B
    say(f"# small_conv8 on is faster for all three models at every swept B up to {upto} (0: not even at B = 1)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

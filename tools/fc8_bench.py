#!/usr/bin/env python3
"""e4m3 against bf16 fully connected layers on one GPU -> profiles/fc8.txt.

  python tools/fc8_bench.py [--out profiles/fc8.txt]

Per-launch kernel times of fc_small / fc_small8 (B = 1, 16) and fc_gemm /
fc_gemm8 (B = 256) on AlexNet's classifier.1 (9216 -> 4096) and classifier.4
(4096 -> 4096), quant_e4m3 at B = 1 and 256, graph-replayed forwards of
`alexnet` and `alexnet_fp8` at B = 1 and 256, and both engines' logits against
the fp32 model.

How the kernel times are taken: a hipGraph of LAUNCHES back-to-back launches
(native calls on preallocated buffers, nothing else in the graph) that walk
COPIES copies of the weights, enough that the copies together exceed 512 MB, so
every launch streams its weights from HBM as it does inside a forward, not
from the 256 MB last-level cache. The two forms of a pair are replayed in turn,
ROUNDS times each, timed by device events; reported: the median per-launch
time and the fastest / slowest round. Forwards the same way (REPS replays of the
engine's own graph per round, host-launched: at B = 1 the host's launch rate
can be what is measured, and both archs then read alike).
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
from dmlc.models.calibrated import calibrated, mixed_images, normalize  # noqa: E402
from dmlc.runtime import InferenceEngine  # noqa: E402

LAUNCHES, ROUNDS, REPS = 48, 15, 50
LINES = []


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
    """forms: [(name, run)], replayed in turn; one line with each one's median [fastest .. slowest]."""
    ts = {n: [] for n, _ in forms}
    for _ in range(ROUNDS):
        for n, run in forms:
            ts[n].append(timed(run, per))
    parts = [f"{n} {statistics.median(t):8.2f} us [{min(t):.2f} .. {max(t):.2f}]" for n, t in ts.items()]
    med = [statistics.median(t) for t in ts.values()]
    ratio = f"   {list(ts)[1]} / {list(ts)[0]} = {med[1] / med[0]:.3f}" if len(med) == 2 else ""
    say(f"{what:34s} " + "   ".join(parts) + ratio)


def fc_pair(C, dev, B, K, N, cus):
    g = torch.Generator().manual_seed(K + B)
    x = torch.randn(B, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.zeros(N, device=dev)
    copies16 = -(-(512 << 20) // (N * K * 2))
    copies8 = -(-(512 << 20) // (N * K))
    w16 = [w.bfloat16().to(dev) for _ in range(copies16)]
    q, s = ops.pack_conv_weight_fp8(w[:, :, None, None])
    w8 = [q.to(dev) for _ in range(copies8)]
    sx = float(x.abs().max()) / 448
    alpha = (sx * s).float().to(dev)
    x16 = x.bfloat16().to(dev)
    x8 = ops.quantize_fp8(x, sx).to(dev)
    y16 = torch.empty(B, N, dtype=torch.bfloat16, device=dev)
    y8 = torch.empty(B, N, dtype=torch.uint8, device=dev)
    zero = torch.zeros(64, device=dev)
    if B <= 16:
        l16 = lambda i: C.fc_small(x16.data_ptr(), K, w16[i].data_ptr(), K, bias.data_ptr(), y16.data_ptr(), N, False, B,
                                   K, N, N, True, torch.cuda.current_stream().cuda_stream)
        l8 = lambda i: C.fc_small8(x8.data_ptr(), K, w8[i].data_ptr(), K, alpha.data_ptr(), bias.data_ptr(),
                                   y8.data_ptr(), N, False, True, 1.0, B, K, N, N, True,
                                   torch.cuda.current_stream().cuda_stream)
        names = ("fc_small", "fc_small8")
    else:
        s16, s8 = C.fc_gemm_splits(B, K, N, cus), C.fc_gemm8_splits(B, K, N, cus)
        ws = torch.empty(max(s16, s8) * B * N, device=dev)
        l16 = lambda i: C.conv2d(x=x16.data_ptr(), w=w16[i].data_ptr(), bias=bias.data_ptr(), res=0, y=y16.data_ptr(),
                                 B=B, H=1, W=1, Cin=K, KH=1, KW=1, stride=1, pad=0, N=N, Npad=N, Kpad=K, ldo=N,
                                 relu=True, out_f32=False, split_k=s16, ws=ws.data_ptr(), tile=C.CONV_FC,
                                 zero=zero.data_ptr(), stem=False, Ho=1, Wo=1, max_blocks=0,
                                 stream=torch.cuda.current_stream().cuda_stream)
        l8 = lambda i: C.fc_gemm8(x8.data_ptr(), w8[i].data_ptr(), alpha.data_ptr(), bias.data_ptr(), y8.data_ptr(),
                                  ws.data_ptr(), zero.data_ptr(), B, K, N, N, N, True, False, True, 1.0, s8,
                                  torch.cuda.current_stream().cuda_stream)
        names = (f"fc_gemm/{s16}+reduce", f"fc_gemm8/{s8}+reduce")
    g16, g8 = graph_of(l16, copies16), graph_of(l8, copies8)
    floor = lambda bytes_: bytes_ / 8e12 * 1e6
    compare(f"{K}->{N} B={B}", [(names[0], g16.replay), (names[1], g8.replay)], LAUNCHES)
    say(f"{'':34s} weight bytes at 8 TB/s: bf16 {floor(N * K * 2):.2f} us, e4m3 {floor(N * K):.2f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "fc8.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fc8_bench needs a GPU")
    C, dev = dmlc.native(), torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    say(f"# python tools/fc8_bench.py   ({torch.cuda.get_device_name(0)}, {cus} CUs)")
    say(f"# kernels: medians of {ROUNDS} interleaved rounds of {LAUNCHES} graph-captured launches over weight copies "
        f"> 512 MB; [fastest .. slowest round]")
    for K, N in ((9216, 4096), (4096, 4096)):
        for B in (1, 16, 256):
            fc_pair(C, dev, B, K, N, cus)
    for B in (1, 256):
        x = torch.randn(B, 9216).bfloat16().to(dev)
        y = torch.empty(B, 9216, dtype=torch.uint8, device=dev)
        g = graph_of(lambda i: C.quant_e4m3(x.data_ptr(), y.data_ptr(), B, 9216, 3.0,
                                            torch.cuda.current_stream().cuda_stream), 1)
        compare(f"quant_e4m3 9216 B={B}", [("quant_e4m3", g.replay)], LAUNCHES)

    say()
    say(f"# forwards: medians of {ROUNDS} interleaved rounds of {REPS} graph replays (predict(), 224x224 u8 images)")
    model = calibrated("alexnet", seed=11)
    sd = state_dict_f32(model)
    engines = {a_: InferenceEngine(a_, sd, max_batch=256) for a_ in ("alexnet", "alexnet_fp8")}
    for B in (1, 256):
        img = mixed_images(B, seed=70 + B).to(dev)
        forms = []
        for name, e in engines.items():
            out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
            e.predict(img, out=out)
            torch.cuda.synchronize()
            forms.append((name, lambda e=e, out=out: [e.predict(img, out=out) for _ in range(REPS)]))
        compare(f"forward B={B}", forms, REPS)

    say()
    say("# logits against the fp32 torch model, relative L2, 32 calibrated discriminating images (mixed_images seed 62)")
    img = mixed_images(32, seed=62)
    with torch.no_grad():
        ref = model(normalize(img))
    for name, e in engines.items():
        _, _, logits = e.predict(img.to(dev), return_logits=True, use_graph=False)
        torch.cuda.synchronize()
        rel = ((logits.cpu() - ref).norm() / ref.norm()).item()
        agree = (logits.cpu().argmax(-1) == ref.argmax(-1)).float().mean().item()
        say(f"{name:12s} rel L2 {rel:.4f}   top-1 agreement {agree:.3f}   ({ref.argmax(-1).unique().numel()} fp32 classes)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

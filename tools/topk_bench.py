#!/usr/bin/env python3
"""Measurements for softmax + top-k (csrc/kernels/softmax_topk.hip and
Engine.forward_topk), written as plain text. One GPU.

  kernel  ops.softmax_topk at B=256, N=1000 for k = 1, 5, 16 next to
          ops.softmax_top1 on the same logits: device events around blocks of
          back-to-back launches after a warm-up, the variants interleaved.
  engine  ResNet18 b256, graph-replayed predict(topk=5) against
          predict(topk=1) in one process: device events around blocks of
          forwards, the two interleaved, median over the blocks. The
          difference is what the extra launch costs a forward.

usage: python tools/topk_bench.py [kernel] [engine] [--iters 500] [--blocks 9] [--steps 50]
                                  [--out profiles/topk.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dmlc  # noqa: E402
from dmlc import ops  # noqa: E402

B, N = 256, 1000


def _block_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _interleaved(fns, iters, blocks, warmup):
    """{name: fn} -> {name: [us per call, one per block]}, the variants taking turns block by block."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            times[name].append(_block_us(fn, iters))
    return times


def bench_kernel(a, emit):
    dev = torch.device("cuda", 0)
    logits = (torch.randn(B, N, generator=torch.Generator().manual_seed(0)) * 3).to(dev)
    # the native launchers on preallocated outputs: as little host work per launch as Python allows
    C = dmlc.native()
    idx = torch.empty(B, 16, dtype=torch.int32, device=dev)
    prob = torch.empty(B, 16, dtype=torch.float32, device=dev)
    lp, ip, pp, stream = logits.data_ptr(), idx.data_ptr(), prob.data_ptr(), torch.cuda.current_stream().cuda_stream
    fns = {"softmax_top1": lambda: C.softmax_top1(lp, B, N, N, ip, pp, stream)}
    for k in (1, 5, 16):
        fns[f"softmax_topk k={k}"] = (lambda k: lambda: C.softmax_topk(lp, B, N, N, k, ip, pp, stream))(k)
        i, p = ops.softmax_topk(logits, k)
        i1, p1 = ops.softmax_top1(logits)
        if not (torch.equal(i[:, 0], i1) and torch.equal(p[:, 0], p1)):
            raise SystemExit(f"topk_bench kernel: k={k} rank 0 differs from softmax_top1")
    t = _interleaved(fns, a.iters, a.blocks, 50)
    emit(f"kernel ({torch.cuda.get_device_name(0)}), fp32 logits [{B}, {N}], time per launch (device events around "
         f"back-to-back launches on one stream, so never less than the launch rate of the host), median (min) of "
         f"{a.blocks} interleaved blocks of {a.iters} launches:")
    for name, ts in t.items():
        emit(f"  {name:<20} {statistics.median(ts):7.2f} us ({min(ts):.2f})")


def bench_engine(a, emit):
    from dmlc.models.calibrated import mixed_images
    from dmlc.runtime import InferenceEngine
    dev = torch.device("cuda", 0)
    eng = InferenceEngine("resnet18", None, max_batch=B)
    img = mixed_images(B, seed=1).to(dev)
    out = {1: (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)),
           5: (torch.empty(B, 5, dtype=torch.int32, device=dev), torch.empty(B, 5, dtype=torch.float32, device=dev))}
    fns = {k: (lambda k: lambda: eng.predict(img, out=out[k], topk=k))(k) for k in (1, 5)}
    t = _interleaved(fns, a.steps, a.blocks, 10)
    torch.cuda.synchronize()
    if not torch.equal(out[5][0][:, 0], out[1][0]):
        raise SystemExit("topk_bench engine: topk=5 and topk=1 disagree on the top class")
    m1, m5 = statistics.median(t[1]), statistics.median(t[5])
    emit(f"engine ({torch.cuda.get_device_name(0)}), resnet18 b{B} on native 224x224 images, graph replay into "
         f"preallocated outputs, device events, median (min) of {a.blocks} interleaved blocks of {a.steps} forwards:")
    emit(f"  predict(topk=1)      {m1:8.1f} us per forward ({min(t[1]):.1f})   {B / m1 * 1e6:9.0f} images/s")
    emit(f"  predict(topk=5)      {m5:8.1f} us per forward ({min(t[5]):.1f})   {B / m5 * 1e6:9.0f} images/s")
    diffs = [x5 - x1 for x1, x5 in zip(t[1], t[5])]
    emit(f"  added by top-5       {m5 - m1:8.1f} us per forward = {(m5 - m1) / m1 * 100:.2f} %   (block by block: "
         f"median {statistics.median(diffs):.1f}, min {min(diffs):.1f}, max {max(diffs):.1f} us; the spread of "
         f"topk=1 alone over its blocks is {max(t[1]) - min(t[1]):.1f} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "engine"], help="kernel, engine")
    ap.add_argument("--iters", type=int, default=500, help="kernel calls per block")
    ap.add_argument("--steps", type=int, default=50, help="forwards per block")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench: no GPU visible")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for w in a.what:
        if w == "kernel":
            bench_kernel(a, emit)
        elif w == "engine":
            bench_engine(a, emit)
        else:
            raise SystemExit(f"unknown measurement: {w}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

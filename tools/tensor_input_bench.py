#!/usr/bin/env python3
"""Measurements for float-tensor input (csrc/kernels/pack_tensor.hip and
Engine.forward_tensor), written as plain text. One GPU.

  kernel  pack_tensor alone at B=256, S=224 into the fused ResNet stem's paired
          image (pad 3) for fp32 NCHW, bf16 NCHW and fp32 channels_last, next
          to preprocess_u8 on a u8 batch of the same size: device events
          around blocks of back-to-back launches after a warm-up, the variants
          interleaved. Achieved bytes/s = (input bytes + packed bytes written)
          over the time per launch, both computed from the shapes.
  engine  ResNet18 and AlexNet b256, graph-replayed predict() on an fp32 NCHW
          tensor against predict() on the u8 images it was made from, in one
          process: device events around blocks of forwards, the two
          interleaved, median over the blocks. u8 input at 224x224 runs the
          fused u8 stems; tensor input runs the pack pass and the strip stem.

usage: python tools/tensor_input_bench.py [kernel] [engine] [--iters 200] [--blocks 9] [--steps 30]
                                          [--out profiles/tensor_input.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dmlc  # noqa: E402
from dmlc import ops  # noqa: E402

B, S, PAD = 256, 224, 3


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
    from dmlc.models.calibrated import mixed_images, normalize
    dev = torch.device("cuda", 0)
    C = dmlc.native()
    Wr = ops.stem_row_width(S, PAD, 7, 2)
    u8 = mixed_images(B, seed=1).to(dev)
    x = normalize(u8.cpu()).contiguous().to(dev)
    inputs = {"pack_tensor fp32 NCHW": x,
              "pack_tensor bf16 NCHW": x.bfloat16(),
              "pack_tensor fp32 channels_last": x.contiguous(memory_format=torch.channels_last)}
    y = torch.empty(B, S + 2 * PAD, Wr // 2, 8, dtype=torch.bfloat16, device=dev)
    out_bytes = y.numel() * 2
    stream = torch.cuda.current_stream().cuda_stream
    # the native launchers on a preallocated output: as little host work per launch as Python allows
    fns = {"preprocess_u8": lambda: C.preprocess_u8(u8.data_ptr(), y.data_ptr(), B, S, S, S, PAD, Wr, stream, True)}
    in_bytes = {"preprocess_u8": u8.numel()}
    for name, t in inputs.items():
        dt, cl = ops.tensor_input(t)
        fns[name] = (lambda t, dt, cl: lambda: C.pack_tensor(t.data_ptr(), dt, cl, y.data_ptr(), B, S, PAD, Wr, True,
                                                             stream))(t, dt, cl)
        in_bytes[name] = t.numel() * t.element_size()
        want = ops.paired_image(t.permute(0, 2, 3, 1).to(torch.bfloat16), PAD, Wr // 2)
        if not torch.equal(ops.pack_tensor(t, PAD, Wr, True).view(torch.int16), want.view(torch.int16)):
            raise SystemExit(f"tensor_input_bench kernel: {name} differs from ops.paired_image")
    t = _interleaved(fns, a.iters, a.blocks, 20)
    emit(f"kernel ({torch.cuda.get_device_name(0)}), B={B}, S={S}, pad {PAD}, row width {Wr}, paired output "
         f"({out_bytes / 1e6:.1f} MB written), time per launch (device events around back-to-back launches on one "
         f"stream), median (min) of {a.blocks} interleaved blocks of {a.iters} launches; bytes/s = (bytes read + bytes "
         f"written, from the shapes) / median:")
    for name, ts in t.items():
        med = statistics.median(ts)
        emit(f"  {name:<32} {med:8.1f} us ({min(ts):.1f})   reads {in_bytes[name] / 1e6:6.1f} MB   "
             f"{(in_bytes[name] + out_bytes) / med / 1e6:6.2f} TB/s")


def bench_engine(a, emit):
    from dmlc.models.calibrated import mixed_images, normalize
    from dmlc.runtime import InferenceEngine
    dev = torch.device("cuda", 0)
    u8 = mixed_images(B, seed=1).to(dev)
    x = normalize(u8.cpu()).contiguous().to(dev)
    emit(f"engine ({torch.cuda.get_device_name(0)}), b{B} at {S}x{S}, graph replay into preallocated outputs, device "
         f"events, median (min) of {a.blocks} interleaved blocks of {a.steps} forwards; u8: the fused u8 stem, fp32 "
         f"tensor: pack_tensor + the stem on the packed image:")
    for arch in ("resnet18", "alexnet"):
        eng = InferenceEngine(arch, None, max_batch=B)
        out = {k: (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
               for k in ("u8", "tensor")}
        fns = {"u8": lambda: eng.predict(u8, out=out["u8"]), "tensor": lambda: eng.predict(x, out=out["tensor"])}
        t = _interleaved(fns, a.steps, a.blocks, 10)
        torch.cuda.synchronize()
        mu, mt = statistics.median(t["u8"]), statistics.median(t["tensor"])
        kernels = [k for k, _, _, _ in eng._e.plan(B, S, S, tensor_in=True)][:3]
        emit(f"  {arch} (tensor plan starts {' -> '.join(kernels)})")
        emit(f"    predict(u8)            {mu:8.1f} us per forward ({min(t['u8']):.1f})   {B / mu * 1e6:9.0f} images/s")
        emit(f"    predict(fp32 tensor)   {mt:8.1f} us per forward ({min(t['tensor']):.1f})   {B / mt * 1e6:9.0f} images/s")
        diffs = [b - c for c, b in zip(t["u8"], t["tensor"])]
        emit(f"    added by tensor input  {mt - mu:8.1f} us per forward = {(mt - mu) / mu * 100:.2f} %   (block by "
             f"block: median {statistics.median(diffs):.1f}, min {min(diffs):.1f}, max {max(diffs):.1f} us; the "
             f"spread of u8 alone over its blocks is {max(t['u8']) - min(t['u8']):.1f} us)")
        del eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "engine"], help="kernel, engine")
    ap.add_argument("--iters", type=int, default=200, help="kernel calls per block")
    ap.add_argument("--steps", type=int, default=30, help="forwards per block")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tensor_input_bench: no GPU visible")
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

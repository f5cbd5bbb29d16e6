#!/usr/bin/env python3
"""Measurements for the embeddings path (csrc/kernels/embed.hip and the
features buffer of Engine.forward_topk), written as plain text. One GPU.

  kernel  embed_rows at B=256 for (HW, C) = (1, 512), (1, 2048), (1, 4096),
          (49, 512) bf16 and (49, 2048) e4m3, plain and normalised: device
          events around blocks of back-to-back launches after a warm-up, the
          variants interleaved. Next to each time the bytes the launch has to
          move (x read once, out written once) over that time.
  engine  ResNet18 and AlexNet b256, graph-replayed predict() with and without
          return_features in one process: device events around blocks of
          forwards, the two interleaved, median over the blocks. The
          difference is what the extra launch costs a forward.
  fp8     resnet50_fp8's features against the fp32 model's penultimate
          features (relative L2) on a discriminating batch, next to the bf16
          ResNet50's on the same images and model. No bar is set for it.

usage: python tools/embed_bench.py [kernel] [engine] [fp8] [--iters 500] [--blocks 9] [--steps 50]
                                   [--out profiles/embed.txt]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dmlc  # noqa: E402
from dmlc import ops  # noqa: E402

B = 256
KERNEL_SHAPES = [(1, 512, False), (1, 2048, False), (1, 4096, False), (49, 512, False), (49, 2048, True)]


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
    C = dmlc.native()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    fns, nbytes, keep = {}, {}, []
    for HW, Ch, fp8 in KERNEL_SHAPES:
        if fp8:
            x = torch.randint(0, 0x78, (B, HW, Ch), dtype=torch.uint8, generator=g).to(dev)
        else:
            x = torch.randn(B, HW, Ch, generator=g).bfloat16().to(dev)
        out = torch.empty(B, Ch, dtype=torch.float32, device=dev)
        keep += [x, out]
        # the op against the kernel's contract before it is timed
        v = ops.embed_rows(x[:, 0].contiguous() if HW == 1 else x, scale=0.5 if fp8 else None)
        want = x[:, 0].float() if HW == 1 else None if fp8 else ops.avgpool_global(x.view(B, HW, 1, Ch)).float()
        if want is not None and not torch.equal(v, want):
            raise SystemExit(f"embed_bench kernel: HW={HW} C={Ch} differs from its reference")
        for norm in (False, True):
            name = f"HW={HW:<2} C={Ch:<4} {'e4m3' if fp8 else 'bf16'} {'normalised' if norm else 'plain'}"
            fns[name] = (lambda xp, op, HW, Ch, fp8, norm: lambda: C.embed_rows(
                xp, op, B, HW, Ch, fp8, 0.5 if fp8 else 1.0, norm, stream))(x.data_ptr(), out.data_ptr(), HW, Ch, fp8, norm)
            nbytes[name] = x.numel() * x.element_size() + out.numel() * 4
    t = _interleaved(fns, a.iters, a.blocks, 50)
    emit(f"kernel ({torch.cuda.get_device_name(0)}), embed_rows at B={B}, time per launch (device events around "
         f"back-to-back launches on one stream, so never less than the launch rate of the host), median (min) of "
         f"{a.blocks} interleaved blocks of {a.iters} launches; bytes = x read once + out written once:")
    for name, ts in t.items():
        med = statistics.median(ts)
        emit(f"  {name:<34} {med:7.2f} us ({min(ts):.2f})   {nbytes[name] / 1e6:6.2f} MB   "
             f"{nbytes[name] / med * 1e-6:6.2f} TB/s")


def bench_engine(a, emit):
    from dmlc.models.calibrated import mixed_images
    from dmlc.runtime import InferenceEngine
    dev = torch.device("cuda", 0)
    img = mixed_images(B, seed=1).to(dev)
    for arch in ("resnet18", "alexnet"):
        eng = InferenceEngine(arch, None, max_batch=B)
        out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev))
        feats = torch.empty(B, eng.feature_dim, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        ip, pp, xp = out[0].data_ptr(), out[1].data_ptr(), img.data_ptr()
        # the native entry point on preallocated buffers, one graph per variant
        fns = {"plain": lambda: eng._e.forward_topk(xp, B, 224, 224, 1, ip, pp, 0, stream, True),
               "features": lambda: eng._e.forward_topk(xp, B, 224, 224, 1, ip, pp, 0, stream, True,
                                                       features=feats.data_ptr()),
               "normalised": lambda: eng._e.forward_topk(xp, B, 224, 224, 1, ip, pp, 0, stream, True,
                                                         features=feats.data_ptr(), l2norm=True)}
        t = _interleaved(fns, a.steps, a.blocks, 10)
        torch.cuda.synchronize()
        base = eng.predict(img)
        with_f = eng.predict(img, return_features=True)
        torch.cuda.synchronize()
        if not (torch.equal(base[0], with_f[0]) and torch.equal(base[1], with_f[1])):
            raise SystemExit(f"embed_bench engine: {arch} answers differ with features")
        m = {k: statistics.median(v) for k, v in t.items()}
        emit(f"engine ({torch.cuda.get_device_name(0)}), {arch} b{B} on native 224x224 images, feature_dim "
             f"{eng.feature_dim}, graph replay into preallocated buffers, device events, median (min) of {a.blocks} "
             f"interleaved blocks of {a.steps} forwards:")
        for k, label in (("plain", "no features"), ("features", "features"), ("normalised", "normalised features")):
            emit(f"  {label:<20} {m[k]:8.1f} us per forward ({min(t[k]):.1f})   {B / m[k] * 1e6:9.0f} images/s")
        for k in ("features", "normalised"):
            diffs = [x - p for p, x in zip(t["plain"], t[k])]
            emit(f"  added by {k:<11} {m[k] - m['plain']:8.1f} us per forward = {(m[k] - m['plain']) / m['plain'] * 100:.2f} %"
                 f"   (block by block: median {statistics.median(diffs):.1f}, min {min(diffs):.1f}, max {max(diffs):.1f} us)")
        emit(f"  spread of the forward without features over its blocks: {max(t['plain']) - min(t['plain']):.1f} us")
        del eng


def bench_fp8(a, emit):
    from dmlc.models import penultimate_features, state_dict_f32
    from dmlc.models.calibrated import calibrated, mixed_images, normalize
    from dmlc.runtime import InferenceEngine
    dev = torch.device("cuda", 0)
    model = calibrated("resnet50", seed=11)
    img = mixed_images(32, seed=102)
    x = normalize(img)
    with torch.no_grad():
        n_cls = len(set(model(x).argmax(-1).tolist()))
    ref = penultimate_features(model, x)
    emit(f"features against the fp32 model's penultimate features, calibrated(resnet50, seed=11), 32 mixed images "
         f"({n_cls} distinct fp32 top-1 classes), relative L2 (rolled by one image):")
    for arch in ("resnet50", "resnet50_fp8"):
        eng = InferenceEngine(arch, state_dict_f32(model), max_batch=32)
        for B_ in (4, 32):
            f = torch.cat([eng.embed(c.to(dev)).cpu() for c in img.split(B_)])
            rel = ((f - ref).norm() / ref.norm()).item()
            rolled = ((f.roll(1, 0) - ref).norm() / ref.norm()).item()
            tail = eng._e.plan(B_, 224, 224, features=True)[-1][3]
            emit(f"  {arch:<13} in batches of {B_:<3} {rel:.4f} ({rolled:.3f})   Embed {tail}")
        del eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "engine", "fp8"], help="kernel, engine, fp8")
    ap.add_argument("--iters", type=int, default=500, help="kernel calls per block")
    ap.add_argument("--steps", type=int, default=50, help="forwards per block")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("embed_bench: no GPU visible")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for w in a.what:
        if w == "kernel":
            bench_kernel(a, emit)
        elif w == "engine":
            bench_engine(a, emit)
        elif w == "fp8":
            bench_fp8(a, emit)
        else:
            raise SystemExit(f"unknown measurement: {w}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

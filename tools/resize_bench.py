#!/usr/bin/env python3
"""Measurements for the ragged resize kernels (csrc/kernels/resize.hip), plain
and antialiased, written as plain text.

  kernel  time per launch of `resize_u8_ragged` at B = 64 and S = 224 for
          500x375 sources, 2048x1536 sources and the 224x224 copy case, both
          kernels, device events around back-to-back launches on uploaded
          descriptors, the two kernels alternating round by round in one
          process; and the ResNet18 forward of the same batch for context.
  node    wall time of one mixed-size 16-image query (member predict RPC,
          images resident in the HBM cache: resize + forward + top-1 + RPC) on
          one dmlc-node, --resize-antialias off and on, interleaved, --runs
          nodes each; p50 over the last three quarters of each node's queries.

usage: python tools/resize_bench.py [kernel] [node] [--runs 3] [--queries 200] [--out profiles/resize_aa.txt]
(both measurements make up profiles/resize_aa.txt: python tools/resize_bench.py kernel node)
"""
import argparse
import os
import statistics
import struct
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import dmlc  # noqa: E402
from dmlc.utils.dataset import make_synthetic_dataset, synthetic_labels, write_labels  # noqa: E402

RAGGED = [(224, 224), (375, 500), (500, 333), (256, 300), (480, 640), (199, 211), (224, 300), (640, 427)]
B, S = 64, 224


def bench_kernel(emit, rounds=7, min_iters=20):
    import torch
    from dmlc import ops
    from dmlc.runtime import InferenceEngine
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench kernel: no GPU visible")
    nat = dmlc.native()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    g = torch.Generator(device="cpu").manual_seed(0)

    def timed(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3  # us

    emit(f"kernel ({torch.cuda.get_device_name(0)}), resize_u8_ragged, B = {B} -> {S}x{S}, uniform-noise sources, "
         f"descriptors already uploaded, device events around back-to-back launches, median (min) of {rounds} "
         f"rounds, plain and antialiased alternating:")
    for name, (h, w) in (("500x375", (375, 500)), ("2048x1536", (1536, 2048)), ("224x224 (copy)", (S, S))):
        imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(B)]
        descs = np.zeros(B, dtype=np.dtype([("ptr", "<u8"), ("h", "<i4"), ("w", "<i4")]))
        for i, t in enumerate(imgs):
            descs[i] = (t.data_ptr(), h, w)
        d, _ = ops._upload([descs], dev)
        fns = {aa: (lambda aa=aa: nat.resize_u8_ragged(d.data_ptr(), out.data_ptr(), B, S, stream, aa))
               for aa in (False, True)}
        iters = {}
        for aa, fn in fns.items():  # warm-up, and enough launches for ~0.2 s per round
            timed(fn, 3)
            iters[aa] = max(min_iters, int(2e5 / max(timed(fn, 20), 0.5)))
        ts = {False: [], True: []}
        for _ in range(rounds):
            for aa, fn in fns.items():
                ts[aa].append(timed(fn, iters[aa]))
        src_mb = B * h * w * 3 / 1e6
        for aa in (False, True):
            med = statistics.median(ts[aa])
            emit(f"  {name:15s} {'antialiased' if aa else 'plain      '} {med:9.1f} us ({min(ts[aa]):.1f})  "
                 f"{iters[aa]} launches per round; {src_mb:.0f} MB of source"
                 + (f" = {src_mb / med:.2f} TB/s if every source byte is read once" if aa else ""))
    eng = InferenceEngine("resnet18", None, device=0, max_batch=B)
    x = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, generator=g).to(dev)
    for _ in range(5):
        eng.predict(x)
    torch.cuda.synchronize()
    fw = [timed(lambda: eng.predict(x), 50) for _ in range(rounds)]
    emit(f"  ResNet18 bf16 forward of the same batch (engine.predict, graph replay): {statistics.median(fw):.1f} us "
         f"({min(fw):.1f})")


def _pct(xs, q):
    xs = sorted(xs)
    k = (len(xs) - 1) * q / 100
    lo, hi = int(k), min(int(k) + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (k - lo)


def bench_node(root, runs, queries, emit, port=23300):
    from dmlc.serve import rpc
    from dmlc.serve.cluster import LocalCluster
    from dmlc.utils.ot import write_random_checkpoint
    labels = synthetic_labels(1000)
    lab = write_labels(os.path.join(root, "synset_words.txt"), labels)
    ds = make_synthetic_dataset(os.path.join(root, "train"), labels[:16], size=RAGGED, seed=9)
    ck = write_random_checkpoint("resnet18", os.path.join(root, "resnet18.ot"), seed=4)
    ids = [w for w, _ in labels[:16]]
    payload = rpc.s("resnet18") + struct.pack("<I", len(ids)) + b"".join(rpc.s(i) for i in ids)
    emit(f"node, one dmlc-node on GPU 0, one query of 16 mixed-size JPEGs ({len(RAGGED)} sizes from 199x211 to "
         f"640x480, resident in the HBM cache after the first query), member predict RPC over a new connection, "
         f"{queries} queries per node, {runs} nodes each, interleaved off/on; wall time per query over the last "
         f"three quarters:")
    p50s = {False: [], True: []}
    for r in range(runs):
        for flag in (False, True):
            cl = LocalCluster(1, port, os.path.join(root, f"c{r}{int(flag)}"), lab, n_leaders=1, executor="gpu",
                              dataset=ds, models=f"resnet18={ck}",
                              extra=["--jobs", "resnet18", "--max-batch", "16"] + (["--resize-antialias"] if flag else []))
            port += 10
            with cl:
                ms = []
                for _ in range(queries):
                    t0 = time.perf_counter()
                    status, body = rpc.call("127.0.0.1", cl.ports[0] + 2, rpc.M_PREDICT, payload, timeout=120)
                    ms.append((time.perf_counter() - t0) * 1e3)
                    if status != 0 or body[0] != 1:
                        raise SystemExit("resize_bench node: the query failed")
            ms = ms[len(ms) // 4:]
            p50s[flag].append(_pct(ms, 50))
            emit(f"  run {r} --resize-antialias {'on ' if flag else 'off'}: p50 {_pct(ms, 50):.3f} ms, p90 "
                 f"{_pct(ms, 90):.3f} ms, min {min(ms):.3f} ms")
    for flag in (False, True):
        emit(f"  median of the runs' p50, --resize-antialias {'on ' if flag else 'off'}: "
             f"{statistics.median(p50s[flag]):.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "node"], help="kernel, node")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "resize_aa.txt"))
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory(prefix="dmlc_resize_") as root:
        for w in a.what:
            if w == "kernel":
                bench_kernel(emit)
            elif w == "node":
                bench_node(root, a.runs, a.queries, emit)
            else:
                raise SystemExit(f"unknown measurement: {w}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measurements for the split JPEG decode (Huffman on the CPU, inverse DCT and
colour on the GPU: csrc/kernels/jpeg_finish.hip), written as plain text.

  host  per-image time of decode_jpeg against decode_jpeg_coeffs on the
        synthetic 500x375 set, one thread: the share of the decode that is
        entropy decoding. Needs no GPU.
  gpu   time of the launch pair (jpeg_idct_planes + jpeg_planes_to_rgb, device
        events, buffers already uploaded) for 1 image and for 64 ragged
        images, after warm-up; the whole ops.jpeg_decode call for context; and
        the share of bytes that differ from the CPU decoder.
  node  `jobs` throughput and p50 of both jobs on one dmlc-node with
        --query-batch 16 --adaptive-window 4 over a cold cache smaller than
        the dataset, --jpeg-gpu off and on, interleaved, --runs each.

usage: python tools/jpeg_bench.py [host] [gpu] [node] [--images 64] [--node-images 1000] [--runs 3]
                                  [--out profiles/jpeg_gpu.txt]
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import dmlc  # noqa: E402
from dmlc.utils.dataset import make_synthetic_dataset, synthetic_labels, write_labels  # noqa: E402

RAGGED = [(224, 224), (375, 500), (500, 333), (256, 300), (480, 640), (199, 211), (224, 300), (640, 427)]


def _blobs(root, n, size):
    labels = synthetic_labels(n)
    ds = make_synthetic_dataset(os.path.join(root, f"set{len(os.listdir(root))}"), labels, size=size)
    out = []
    for wnid, _ in labels:
        d = os.path.join(ds, wnid)
        with open(os.path.join(d, sorted(os.listdir(d))[0]), "rb") as f:
            out.append(f.read())
    return out


def _per_image_ms(fn, blobs, min_s=1.5):
    for b in blobs:  # warm-up: tables, allocator
        fn(b)
    best, t_end = [], time.perf_counter() + min_s
    while time.perf_counter() < t_end or len(best) < 3:
        t = time.perf_counter()
        for b in blobs:
            fn(b)
        best.append((time.perf_counter() - t) / len(blobs) * 1e3)
    return statistics.median(best), min(best), len(best)


def bench_host(root, n, emit):
    nat = dmlc.native()
    blobs = _blobs(root, n, (375, 500))
    lay, _ = nat.decode_jpeg_coeffs(blobs[0])
    full = _per_image_ms(nat.decode_jpeg, blobs)
    coef = _per_image_ms(nat.decode_jpeg_coeffs, blobs)
    emit(f"host, one thread, {n} synthetic 500x375 JPEGs ({sum(map(len, blobs)) // n} B mean, "
         f"{lay['hmax']}x{lay['vmax']} luma sampling), per image, median (min) of {full[2]} / {coef[2]} passes:")
    emit(f"  decode_jpeg          {full[0]:.3f} ms ({full[1]:.3f})   entropy decode + IDCT + upsampling + colour")
    emit(f"  decode_jpeg_coeffs   {coef[0]:.3f} ms ({coef[1]:.3f})   entropy decode only")
    emit(f"  entropy-decode share {coef[0] / full[0] * 100:.1f} %  (both through the Python binding, which copies "
         f"the result once)")


def bench_gpu(root, n, emit):
    import torch
    from dmlc import ops
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench gpu: no GPU visible")
    nat = dmlc.native()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream

    def pair_us(blobs, iters=200):
        decoded = [nat.decode_jpeg_coeffs(b) for b in blobs]
        layouts = [d[0] for d in decoded]
        offs, total = [], 0
        for lay in layouts:
            offs.append(total)
            total += (lay["height"] * lay["width"] * 3 + 255) // 256 * 256
        rgb = torch.empty(total, dtype=torch.uint8, device=dev)
        descs, tables, ncoef, pbytes = nat.jpeg_gpu_plan(layouts, [rgb.data_ptr() + o for o in offs])
        d, (od, ot, oc) = ops._upload([descs, tables, np.concatenate([x[1] for x in decoded])], dev)
        planes = torch.empty(pbytes, dtype=torch.uint8, device=dev)

        def launch():
            nat.jpeg_idct_planes(descs, d.data_ptr() + od, d.data_ptr() + ot, tables.shape[0], d.data_ptr() + oc,
                                 ncoef, planes.data_ptr(), pbytes, stream)
            nat.jpeg_planes_to_rgb(descs, d.data_ptr() + od, planes.data_ptr(), pbytes, stream)

        for _ in range(20):
            launch()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                launch()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / iters * 1e3)
        return statistics.median(times), min(times), ncoef * 2, total

    one = _blobs(root, 1, (375, 500))
    ragged = _blobs(root, n, RAGGED)
    emit(f"gpu ({torch.cuda.get_device_name(0)}), launch pair on uploaded buffers, device events, "
         f"median (min) of 5 x 200 back-to-back pairs:")
    t = pair_us(one)
    emit(f"  1 image 500x375      {t[0]:.1f} us ({t[1]:.1f})   {t[2]} B of coefficients in, {t[3]} B of RGB out")
    t = pair_us(ragged)
    emit(f"  {n} ragged images     {t[0]:.1f} us ({t[1]:.1f}) = {t[0] / n:.2f} us per image   "
         f"{t[2]} B in, {t[3]} B out")
    for name, blobs in (("1 image", one), (f"{n} ragged", ragged)):
        for _ in range(3):
            ops.jpeg_decode(blobs, dev)
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            ops.jpeg_decode(blobs, dev)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        emit(f"  ops.jpeg_decode, {name}: {statistics.median(ts):.3f} ms wall per call (host entropy decode, one "
             f"upload, launch pair, synchronise)")
    got = ops.jpeg_decode(ragged + one, dev)
    torch.cuda.synchronize()
    differ = total = worst = 0
    for g, b in zip(got, ragged + one):
        c = np.asarray(nat.decode_jpeg(b))
        g = g.cpu().numpy()
        differ += int((g != c).sum())
        total += c.size
        worst = max(worst, int(np.abs(g.astype(np.int32) - c).max()))
    emit(f"  bytes that differ from the CPU decoder: {differ} of {total} = {differ / total * 100:.4f} % "
         f"(largest difference {worst})")


def _pct(xs, q):
    xs = sorted(xs)
    k = (len(xs) - 1) * q / 100
    lo, hi = int(k), min(int(k) + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (k - lo)


def bench_node(root, n, runs, emit, port=23100):
    from dmlc.serve.cluster import LocalCluster
    from dmlc.utils.ot import write_random_checkpoint
    labels = synthetic_labels(1000)
    lab = write_labels(os.path.join(root, "synset_words.txt"), labels)
    ds = make_synthetic_dataset(os.path.join(root, "train"), labels[:n], size=(375, 500))
    ck = {m: write_random_checkpoint(m, os.path.join(root, f"{m}.ot"), seed=i)
          for i, m in enumerate(["resnet18", "alexnet"])}
    cache_mb = max(8, n * 375 * 500 * 3 // 4 >> 20)  # a quarter of the decoded dataset: every query misses
    emit(f"node, one dmlc-node on GPU 0, both jobs over {n} synthetic 500x375 JPEGs, --query-batch 16 "
         f"--adaptive-window 4, --hbm-cache-mb {cache_mb} (cold, smaller than the {n * 375 * 500 * 3 >> 20} MB "
         f"dataset), {runs} runs each, interleaved off/on; rates and p50 over the last three quarters of "
         f"each job's queries:")
    rows = {False: [], True: []}
    for r in range(runs):
        for flag in (False, True):
            extra = ["--job-limit", str(n), "--query-batch", "16", "--adaptive-window", "4", "--quiet-predictions",
                     "--max-batch", "64", "--hbm-cache-mb", str(cache_mb)] + (["--jpeg-gpu"] if flag else [])
            cl = LocalCluster(1, port, os.path.join(root, f"c{r}{int(flag)}"), lab, n_leaders=1, executor="gpu",
                              dataset=ds, models=",".join(f"{m}={p}" for m, p in ck.items()), extra=extra)
            port += 10
            with cl:
                nd = cl.nodes[0]
                nd.cmd("predict")
                deadline = time.time() + 300
                while time.time() < deadline:
                    counts = [int(x) for x in re.findall(r"Accuracy: \d+/(\d+)", nd.cmd("jobs", 30))]
                    if len(counts) == 2 and min(counts) >= n:
                        break
                    time.sleep(0.5)
                else:
                    raise SystemExit("jpeg_bench node: the jobs did not finish")
                dump = os.path.join(root, f"jobs{r}{int(flag)}.json")
                nd.cmd(f"jobs-dump {dump}")
                info = nd.cmd("info")
            jobs = json.load(open(dump))
            row = {}
            for j in jobs:
                # steady state, as tools/bench_jobs.py: the queries completed after the first
                # quarter (first-use costs: code objects, graphs, pinned and scratch buffers)
                done = sorted(x for x in j["done_us"] if x > 0)
                k0 = len(done) // 4
                rate = j["finished"] * (len(done) - 1 - k0) / len(done) / ((done[-1] - done[k0]) / 1e6)
                d = [x / 1000 for x in j["durations_us"]]
                row[j["model"]] = (rate, _pct(d[len(d) // 4:], 50))
            row["both"] = (row["resnet18"][0] + row["alexnet"][0], 0.0)
            rows[flag].append(row)
            m = re.search(r"jpeg gpu (\d+) cpu (\d+)", info)
            emit(f"  run {r} --jpeg-gpu {'on ' if flag else 'off'}: both jobs {row['both'][0]:8.1f} images/s | " +
                 " | ".join(f"{k} {row[k][0]:7.1f} images/s, query p50 {row[k][1]:6.2f} ms"
                            for k in ("resnet18", "alexnet")) + f" | decoded gpu {m.group(1)} cpu {m.group(2)}")
    for flag in (False, True):
        med = {k: statistics.median(r[k][0] for r in rows[flag]) for k in ("both", "resnet18", "alexnet")}
        p50 = {k: statistics.median(r[k][1] for r in rows[flag]) for k in ("resnet18", "alexnet")}
        emit(f"  median --jpeg-gpu {'on ' if flag else 'off'}: both jobs {med['both']:.1f} images/s, resnet18 "
             f"{med['resnet18']:.1f} images/s p50 {p50['resnet18']:.2f} ms, alexnet {med['alexnet']:.1f} images/s "
             f"p50 {p50['alexnet']:.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["host"], help="host, gpu, node")
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--node-images", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory(prefix="dmlc_jpeg_") as root:
        for w in a.what:
            if w == "host":
                bench_host(root, a.images, emit)
            elif w == "gpu":
                bench_gpu(root, a.images, emit)
            elif w == "node":
                bench_node(root, a.node_images, a.runs, emit)
            else:
                raise SystemExit(f"unknown measurement: {w}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

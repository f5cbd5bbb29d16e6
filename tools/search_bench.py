#!/usr/bin/env python3
"""Measurements for the nearest-neighbour search (csrc/kernels/sim_topk.hip,
dmlc.Gallery, InferenceEngine.search), written as plain text. One GPU.

  kernel  ops-level sim_topk (the native launcher on preallocated outputs) at
          D = 512, N = 10 k / 100 k / 1 M, B = 1 / 256, k = 1 / 16, dot and
          cosine, and one row at D = 2048, on bf16 randn; next to it torch on
          the same GPU in the same run, (q.bfloat16() @ g.T).float().topk(k),
          the two interleaved block by block after a warm-up that also primes
          the clocks. Device events around blocks of back-to-back launches;
          median (min - max) over the blocks. Per row: us per launch, gallery
          bytes / time against the 8 TB/s HBM peak, issued 2 B N D flop / time
          against the 2.5 PF bf16 peak.
  engine  a graph-replayed ResNet18 b256 embed() alone and engine.search()
          against a 100 k gallery (the same forward, then the search on the
          same stream), interleaved.
  filtered  the row filter and the k-NN vote (profiles/search_filtered.txt):
          at D = 512, B = 1 / 256, N = 100 k / 1 M, k = 1 / 16, dot metric,
          interleaved: the unfiltered launch; the same launch of another
          build of the library (--base-lib: libdmlc_gpu.so or sim_topk.hip
          alone built from the commit to compare with, loaded beside this
          tree's), measured twice so that the run prints the box's own
          spread; the filter on with every row live, with half the rows
          removed, and with wanted labels over 1000 classes. Then one
          knn_vote launch at B = 256, and a graph-replayed ResNet18 b256
          classify_knn() next to search(), both at k = 5.

  e4m3    the e4m3 gallery (profiles/search_e4m3.txt) at D = 512: the bf16
          launch and the e4m3 launch (its quantising of the queries
          included) interleaved at (B, N, k) = (256, 1 M, 1), (256, 1 M, 16),
          (1, 1 M, 1), (256, 100 k, 1), both metrics, with the e4m3 filtered
          form on live rows and, with --base-lib, the bf16 launch of the
          build to compare with measured twice (its two medians' difference
          is the box's spread, the bar for "the bf16 launch did not move").
          Then a gallery_pack8 launch at M = 256, a graph-replayed ResNet18
          b256 search() against a 100 k gallery of each dtype, and the e4m3
          gallery's recall@1 / recall@16 of the bf16 gallery's answer on
          randn and on a calibrated ResNet18's embeddings of mixed_images.

usage: python tools/search_bench.py [kernel] [engine] [filtered] [e4m3] [--blocks 5] [--base-lib LIB]
                                    [--out profiles/search.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dmlc  # noqa: E402
from dmlc import ops  # noqa: E402

HBM_PEAK, BF16_PEAK = 8e12, 2.5e15


def _block_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _interleaved(fns, blocks, target_us=30e3):
    """{name: fn} -> {name: [us per call, one per block]}: warm-up, iterations sized for ~30 ms blocks, turns."""
    iters = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        iters[name] = int(min(500, max(3, target_us / max(_block_us(fn, 3), 1.0))))
        _block_us(fn, iters[name])
    times = {name: [] for name in fns}
    for _ in range(blocks):
        for name, fn in fns.items():
            times[name].append(_block_us(fn, iters[name]))
    return times


def _fmt(ts):
    return f"{statistics.median(ts):9.1f} us ({min(ts):.1f} - {max(ts):.1f})"


def bench_kernel(a, emit):
    dev = torch.device("cuda", 0)
    C = dmlc.native()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    stream = torch.cuda.current_stream().cuda_stream
    emit(f"kernel ({torch.cuda.get_device_name(0)}, {cus} CUs), bf16 randn, native launcher on preallocated outputs "
         f"vs torch (q.bfloat16() @ g.T).float().topk(k); device events around back-to-back launches, median "
         f"(min - max) of {a.blocks} interleaved blocks; TB/s = gallery bytes / time (peak 8), TF/s = 2 B N D / time "
         f"(peak 2500):")
    gen = torch.Generator(device=dev).manual_seed(0)
    for D, N in ((512, 10_000), (512, 100_000), (512, 1_000_000), (2048, 100_000)):
        g32 = torch.randn(N, D, device=dev, generator=gen)
        g, ginv = ops.gallery_pack(g32, with_norms=True)
        del g32
        for B in (1, 256):
            q = torch.randn(B, D, device=dev, generator=gen)
            qb, qinv = ops.gallery_pack(q, with_norms=True)
            for k in (1, 16):
                if D == 2048 and (B, k) != (256, 16):
                    continue
                slices = C.sim_topk_slices(B, N, cus)
                ws = torch.empty(C.sim_topk_ws_bytes(B, k, slices), dtype=torch.uint8, device=dev)
                idx = torch.empty(B, k, dtype=torch.int32, device=dev)
                score = torch.empty(B, k, dtype=torch.float32, device=dev)
                BF = C.TensorDType.BF16

                def run(qs, gs):
                    C.sim_topk(qb.data_ptr(), BF, qs, g.data_ptr(), gs, B, N, D, k, idx.data_ptr(), score.data_ptr(),
                               ws.data_ptr(), ws.numel(), cus, stream)
                fns = {"dot": lambda: run(0, 0), "cosine": lambda: run(qinv.data_ptr(), ginv.data_ptr()),
                       "torch": lambda: (qb @ g.t()).float().topk(k)}
                run(0, 0)
                ti = (qb @ g.t()).float().topk(k).indices
                agree = (idx.long() == ti).float().mean().item()
                t = _interleaved(fns, a.blocks)
                for name in ("dot", "cosine"):
                    m = statistics.median(t[name]) * 1e-6
                    emit(f"  D={D:<5} N={N:<8} B={B:<4} k={k:<3} {name:<7} {_fmt(t[name])}  "
                         f"{N * D * 2 / m / 1e12:6.3f} TB/s ({N * D * 2 / m / HBM_PEAK * 100:5.1f} %)  "
                         f"{2.0 * B * N * D / m / 1e12:7.1f} TF/s ({2.0 * B * N * D / m / BF16_PEAK * 100:5.2f} %)  "
                         f"slices {slices}")
                mt = statistics.median(t["torch"])
                emit(f"  {'':<38} torch   {_fmt(t['torch'])}  = {mt / statistics.median(t['dot']):.2f} x the dot "
                     f"kernel's time; {agree * 100:.1f} % of its (bf16-rounded scores') indices equal the kernel's")
        del g, ginv


def bench_engine(a, emit):
    from dmlc.models.calibrated import mixed_images
    from dmlc.runtime import InferenceEngine
    dev = torch.device("cuda", 0)
    B, N = 256, 100_000
    eng = InferenceEngine("resnet18", None, max_batch=B)
    img = mixed_images(B, seed=1).to(dev)
    gal = dmlc.Gallery(eng.feature_dim, N, max_batch=B)
    gen = torch.Generator(device=dev).manual_seed(1)
    for i in range(0, N, 10_000):
        gal.add(torch.randn(10_000, eng.feature_dim, device=dev, generator=gen).abs())
    feats = torch.empty(B, eng.feature_dim, device=dev)
    out = (torch.empty(B, 16, dtype=torch.int32, device=dev), torch.empty(B, 16, device=dev))
    fns = {"embed": lambda: eng.embed(img, out=feats), "search": lambda: eng.search(img, gal, k=16, out=out)}
    t = _interleaved(fns, a.blocks)
    me, ms = statistics.median(t["embed"]), statistics.median(t["search"])
    emit(f"engine ({torch.cuda.get_device_name(0)}), resnet18 b{B} graph replay, gallery of {N} x {eng.feature_dim} "
         f"(cosine, k = 16), median (min - max) of {a.blocks} interleaved blocks:")
    emit(f"  embed()                 {_fmt(t['embed'])} per batch  {B / me * 1e6:9.0f} images/s")
    emit(f"  search() = embed+search {_fmt(t['search'])} per batch  {B / ms * 1e6:9.0f} images/s")
    emit(f"  added by the search     {ms - me:9.1f} us = {(ms - me) / me * 100:.1f} % of the forward")


# dmlc::sim_topk as it was before the row filter's two trailing arguments, and with them
_BASE_SYMBOL = "_ZN4dmlc8sim_topkEPKvNS_11TensorDTypeEPKfS1_S4_iliiPiPfPvmiP12ihipStream_ti"
_BASE_SYMBOL_FILTER = _BASE_SYMBOL + "PKiSB_"


def _base_sim_topk(path):
    """The unfiltered launcher of another build of the library, or None."""
    if not path:
        return None
    lib = ctypes.CDLL(os.path.abspath(path), mode=ctypes.RTLD_LOCAL)
    vp = ctypes.c_void_p
    args = [vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int, vp, vp, vp,
            ctypes.c_size_t, ctypes.c_int, vp, ctypes.c_int]
    if hasattr(lib, _BASE_SYMBOL_FILTER):
        fn = getattr(lib, _BASE_SYMBOL_FILTER)
        fn.argtypes, fn.restype = args + [vp, vp], None
        return lambda *a: fn(*a, None, None)
    fn = getattr(lib, _BASE_SYMBOL)
    fn.argtypes, fn.restype = args, None
    return fn


def bench_filtered(a, emit):
    dev = torch.device("cuda", 0)
    C = dmlc.native()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    stream = torch.cuda.current_stream().cuda_stream
    base = _base_sim_topk(a.base_lib)
    D, BF = 512, C.TensorDType.BF16
    emit(f"filtered search ({torch.cuda.get_device_name(0)}, {cus} CUs), D = {D}, dot metric, bf16 randn, native "
         f"launcher on preallocated outputs; device events around back-to-back launches, median (min - max) of "
         f"{a.blocks} interleaved blocks. base / base again: the unfiltered launch of the build to compare with "
         f"({'given' if base else 'not given: --base-lib'}), measured twice in the same turns: their difference is "
         f"the box's spread. live: filter on, every row live; half: 50 % of the rows removed; classes: wanted "
         f"labels over 1000 classes, nothing removed:")
    gen = torch.Generator(device=dev).manual_seed(0)
    for N in (100_000, 1_000_000):
        g = ops.gallery_pack(torch.randn(N, D, device=dev, generator=gen))
        live = torch.zeros(N, dtype=torch.int32, device=dev)
        half = torch.where(torch.rand(N, device=dev, generator=gen) < 0.5, -1, 0).to(torch.int32)
        classes = torch.randint(0, 1000, (N,), device=dev, generator=gen).to(torch.int32)
        for B in (1, 256):
            qb = ops.gallery_pack(torch.randn(B, D, device=dev, generator=gen))
            want = torch.randint(0, 1000, (B,), device=dev, generator=gen).to(torch.int32)
            for k in (1, 16):
                slices = C.sim_topk_slices(B, N, cus)
                ws = torch.empty(C.sim_topk_ws_bytes(B, k, slices), dtype=torch.uint8, device=dev)
                idx = torch.empty(B, k, dtype=torch.int32, device=dev)
                score = torch.empty(B, k, dtype=torch.float32, device=dev)

                def run(label=None, q_want=None):
                    C.sim_topk(qb.data_ptr(), BF, 0, g.data_ptr(), 0, B, N, D, k, idx.data_ptr(), score.data_ptr(),
                               ws.data_ptr(), ws.numel(), cus, stream, g_label=0 if label is None else label.data_ptr(),
                               q_want=0 if q_want is None else q_want.data_ptr())

                def run_base():
                    base(qb.data_ptr(), int(BF), None, g.data_ptr(), None, B, N, D, k, idx.data_ptr(),
                         score.data_ptr(), ws.data_ptr(), ws.numel(), cus, stream, 0)
                fns = {}
                if base:
                    run_base()
                    torch.cuda.synchronize()
                    theirs = (idx.clone(), score.clone())
                    run()
                    torch.cuda.synchronize()
                    if not (torch.equal(theirs[0], idx) and torch.equal(theirs[1], score)):
                        raise SystemExit("search_bench: the unfiltered launch and the base build's differ in bits")
                    fns["base"] = run_base
                fns["unfiltered"] = run
                if base:
                    fns["base again"] = run_base
                fns["live"] = lambda: run(live)
                fns["half"] = lambda: run(half)
                fns["classes"] = lambda: run(classes, want)
                t = _interleaved(fns, a.blocks)
                ref = statistics.median(t["unfiltered"])
                for name in fns:
                    m = statistics.median(t[name])
                    emit(f"  N={N:<8} B={B:<4} k={k:<3} {name:<11} {_fmt(t[name])}  {m / ref:6.3f} x unfiltered  "
                         f"{N * D * 2 / m / 1e6:6.3f} TB/s  slices {slices}")
                if base:
                    b1, b2 = statistics.median(t["base"]), statistics.median(t["base again"])
                    emit(f"  {'':<24} spread of the base build: {abs(b1 - b2) / min(b1, b2) * 100:.2f} % between its "
                         f"two medians; unfiltered is {(ref / ((b1 + b2) / 2) - 1) * 100:+.2f} % off their mean")
        del g, live, half, classes
    # the vote alone
    B, N = 256, 100_000
    labels = torch.randint(0, 1000, (N,), device=dev, generator=gen).to(torch.int32)
    for k in (5, 16):
        idx = torch.randint(0, N, (B, k), device=dev, generator=gen).to(torch.int32)
        score = torch.rand(B, k, device=dev, generator=gen)
        out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev))
        fns = {w: (lambda w=w: C.knn_vote(idx.data_ptr(), score.data_ptr(), labels.data_ptr(), N, B, k, w == "weighted",
                                          out[0].data_ptr(), out[1].data_ptr(), stream))
               for w in ("uniform", "weighted")}
        t = _interleaved(fns, a.blocks)
        for name in fns:
            emit(f"  knn_vote B={B} k={k:<3} {name:<9} {_fmt(t[name])} per launch (back to back)")
    # the engine
    from dmlc.models.calibrated import mixed_images
    from dmlc.runtime import InferenceEngine
    eng = InferenceEngine("resnet18", None, max_batch=B)
    img = mixed_images(B, seed=1).to(dev)
    gal = dmlc.Gallery(eng.feature_dim, N, max_batch=B)
    for i in range(0, N, 10_000):
        gal.add(torch.randn(10_000, eng.feature_dim, device=dev, generator=gen).abs(), labels=labels[i:i + 10_000])
    sout = (torch.empty(B, 5, dtype=torch.int32, device=dev), torch.empty(B, 5, device=dev))
    cout = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev))
    fns = {"search": lambda: eng.search(img, gal, k=5, out=sout),
           "classify_knn": lambda: eng.classify_knn(img, gal, k=5, out=cout)}
    t = _interleaved(fns, a.blocks)
    emit(f"engine, resnet18 b{B} graph replay, gallery of {N} x {eng.feature_dim} (cosine, 1000 labels, k = 5):")
    for name in fns:
        emit(f"  {name + '()':<15} {_fmt(t[name])} per batch  {B / statistics.median(t[name]) * 1e6:9.0f} images/s")
    gal.remove(range(0, N, 2))
    t = _interleaved(fns, a.blocks)
    emit("  the same with every second row removed (the filtered kernel):")
    for name in fns:
        emit(f"  {name + '()':<15} {_fmt(t[name])} per batch  {B / statistics.median(t[name]) * 1e6:9.0f} images/s")


def _recall(got, want):
    """(recall@1, recall@k) of idx `got` [B, k] against `want` [B, k]."""
    r1 = (got[:, 0] == want[:, 0]).float().mean().item()
    rk = (got[:, :, None] == want[:, None, :]).any(-1).float().mean().item()
    return r1, rk


def bench_e4m3(a, emit):
    dev = torch.device("cuda", 0)
    C = dmlc.native()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    stream = torch.cuda.current_stream().cuda_stream
    base = _base_sim_topk(a.base_lib)
    D, BF = 512, C.TensorDType.BF16
    emit(f"e4m3 gallery ({torch.cuda.get_device_name(0)}, {cus} CUs), D = {D}, randn, native launchers on preallocated "
         f"outputs, bf16 queries; the e4m3 launch includes quantising its queries (gallery_pack8, one more launch); "
         f"device events around back-to-back launches, median (min - max) of {a.blocks} interleaved blocks. base / "
         f"base again: the bf16 launch of the build to compare with "
         f"({'given' if base else 'not given: --base-lib'}), twice in the same turns: their difference is the box's "
         f"spread. e4m3 live: the filtered form, every row live. TB/s = the gallery's bytes / time:")
    gen = torch.Generator(device=dev).manual_seed(0)
    for N, shapes in ((1_000_000, ((256, 1), (256, 16), (1, 1))), (100_000, ((256, 1),))):
        g32 = torch.randn(N, D, device=dev, generator=gen)
        g, ginv = ops.gallery_pack(g32, with_norms=True)
        packed = {m: ops.gallery_pack8(g32, m) for m in ("dot", "cosine")}
        del g32
        live = torch.zeros(N, dtype=torch.int32, device=dev)
        for B, k in shapes:
            qb, qinv = ops.gallery_pack(torch.randn(B, D, device=dev, generator=gen), with_norms=True)
            slices = C.sim_topk_slices(B, N, cus)
            ws = torch.empty(max(C.sim_topk_ws_bytes(B, k, slices), C.sim_topk8_ws_bytes(B, k, slices)),
                             dtype=torch.uint8, device=dev)
            idx = torch.empty(B, k, dtype=torch.int32, device=dev)
            score = torch.empty(B, k, dtype=torch.float32, device=dev)
            for metric in ("dot", "cosine"):
                qs, gs = (qinv.data_ptr(), ginv.data_ptr()) if metric == "cosine" else (0, 0)
                codes, scale = packed[metric]

                def run16():
                    C.sim_topk(qb.data_ptr(), BF, qs, g.data_ptr(), gs, B, N, D, k, idx.data_ptr(), score.data_ptr(),
                               ws.data_ptr(), ws.numel(), cus, stream)

                def run_base():
                    base(qb.data_ptr(), int(BF), qs or None, g.data_ptr(), gs or None, B, N, D, k, idx.data_ptr(),
                         score.data_ptr(), ws.data_ptr(), ws.numel(), cus, stream, 0)

                def run8(label=None):
                    C.sim_topk8(qb.data_ptr(), BF, codes.data_ptr(), scale.data_ptr(), metric == "cosine", B, N, D, k,
                                idx.data_ptr(), score.data_ptr(), ws.data_ptr(), ws.numel(), cus, stream,
                                g_label=0 if label is None else label.data_ptr())
                fns = {}
                run16()
                torch.cuda.synchronize()
                want = idx.clone()
                if base:
                    mine = score.clone()
                    run_base()
                    torch.cuda.synchronize()
                    if not (torch.equal(want, idx) and torch.equal(mine, score)):
                        raise SystemExit("search_bench: the bf16 launch and the base build's differ in bits")
                    fns["base"] = run_base
                fns["bf16"] = run16
                fns["e4m3"] = run8
                if base:
                    fns["base again"] = run_base
                fns["e4m3 live"] = lambda: run8(live)
                run8()
                torch.cuda.synchronize()
                r1, rk = _recall(idx, want)
                t = _interleaved(fns, a.blocks)
                ref = statistics.median(t["bf16"])
                for name in fns:
                    m = statistics.median(t[name])
                    nbytes = N * D * (1 if name.startswith("e4m3") else 2)
                    emit(f"  N={N:<8} B={B:<4} k={k:<3} {metric:<6} {name:<10} {_fmt(t[name])}  {m / ref:6.3f} x bf16  "
                         f"{nbytes / m / 1e6:6.3f} TB/s  {2.0 * B * N * D / m / 1e6:7.1f} TF/s  slices {slices}")
                emit(f"  {'':<28} e4m3 against the bf16 answer: recall@1 {r1:.3f}" + (f", recall@{k} {rk:.3f}" if k > 1 else ""))
                if base:
                    b1, b2 = statistics.median(t["base"]), statistics.median(t["base again"])
                    emit(f"  {'':<28} spread of the base build: {abs(b1 - b2) / min(b1, b2) * 100:.2f} % between its two "
                         f"medians; bf16 is {(ref / ((b1 + b2) / 2) - 1) * 100:+.2f} % off their mean")
        del g, ginv, packed, live
    # the quantiser alone
    rows = torch.randn(256, D, device=dev, generator=gen)
    codes = torch.empty(256, D, dtype=torch.uint8, device=dev)
    scale = torch.empty(256, device=dev)
    t = _interleaved({"pack8": lambda: C.gallery_pack8(rows.data_ptr(), C.TensorDType.F32, codes.data_ptr(),
                                                       scale.data_ptr(), True, 256, D, stream)}, a.blocks)
    emit(f"  gallery_pack8 M=256 D={D} fp32 rows, cosine   {_fmt(t['pack8'])} per launch (back to back)")
    # recall at k = 16 on randn, cosine
    N, B = 100_000, 256
    g32 = torch.randn(N, D, device=dev, generator=gen)
    q32 = torch.randn(B, D, device=dev, generator=gen)
    gb, ginv = ops.gallery_pack(g32, with_norms=True)
    qb, qinv = ops.gallery_pack(q32, with_norms=True)
    want = ops.sim_topk(qb, gb, 16, qinv, ginv)[0]
    got = ops.sim_topk8(q32, *ops.gallery_pack8(g32, "cosine"), 16, "cosine")[0]
    r1, rk = _recall(got, want)
    emit(f"  recall of the e4m3 gallery against the bf16 gallery's answer, cosine, k = 16, randn N={N} B={B}: "
         f"recall@1 {r1:.3f}, recall@16 {rk:.3f}")
    del g32, gb, ginv
    # the engine
    from dmlc.models import state_dict_f32
    from dmlc.models.calibrated import calibrated, mixed_images
    from dmlc.runtime import InferenceEngine
    eng = InferenceEngine("resnet18", state_dict_f32(calibrated("resnet18", seed=11)), max_batch=B)
    F = eng.feature_dim
    gals = {dt: dmlc.Gallery(F, 2048, max_batch=B, dtype=dt) for dt in ("bf16", "e4m3")}
    for i in range(8):
        feats = eng.embed(mixed_images(B, seed=100 + i).to(dev))
        for gal in gals.values():
            gal.add(feats)
    img = mixed_images(B, seed=1).to(dev)
    want = eng.search(img, gals["bf16"], k=16)[0].clone()
    got = eng.search(img, gals["e4m3"], k=16)[0].clone()
    r1, rk = _recall(got, want)
    emit(f"  the same on a calibrated resnet18's embeddings of mixed_images, 2048 stored images, {B} other queries: "
         f"recall@1 {r1:.3f}, recall@16 {rk:.3f}")
    gals = {dt: dmlc.Gallery(F, N, max_batch=B, dtype=dt) for dt in ("bf16", "e4m3")}
    for i in range(0, N, 10_000):
        rows = torch.randn(10_000, F, device=dev, generator=gen).abs()
        for gal in gals.values():
            gal.add(rows)
    feats = torch.empty(B, F, device=dev)
    out = (torch.empty(B, 16, dtype=torch.int32, device=dev), torch.empty(B, 16, device=dev))
    fns = {"embed": lambda: eng.embed(img, out=feats),
           "search bf16": lambda: eng.search(img, gals["bf16"], k=16, out=out),
           "search e4m3": lambda: eng.search(img, gals["e4m3"], k=16, out=out)}
    t = _interleaved(fns, a.blocks)
    emit(f"engine, resnet18 b{B} graph replay, gallery of {N} x {F} (cosine, k = 16):")
    for name in fns:
        emit(f"  {name + '()':<15} {_fmt(t[name])} per batch  {B / statistics.median(t[name]) * 1e6:9.0f} images/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernel", "engine"], help="kernel, engine, filtered, e4m3")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--base-lib", default="", help="filtered: a library built from the commit to compare with")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("search_bench: no GPU visible")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for w in a.what:
        if w == "kernel":
            bench_kernel(a, emit)
        elif w == "engine":
            bench_engine(a, emit)
        elif w == "filtered":
            bench_filtered(a, emit)
        elif w == "e4m3":
            bench_e4m3(a, emit)
        else:
            raise SystemExit(f"unknown measurement: {w}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

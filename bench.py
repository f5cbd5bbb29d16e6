#!/usr/bin/env python3
"""Headline benchmark: ResNet18 ImageNet-shaped batch inference, images/s for
the whole node plus p50/p95 latency (BASELINE.json metric).

One process per GPU. ``--gpus N`` under torchrun uses the launcher's ranks;
without a launcher (no WORLD_SIZE in the environment) this script starts the
N rank processes itself (127.0.0.1 rendezvous) before any GPU call.

The data plane is the native layer in csrc/comm (RCCL over xGMI, driven from
C++; torch.distributed is used only as a CPU/gloo side channel to hand out
the RCCL unique ids, for barriers, and for the max over ranks of the timed
region). The serving path (scatter mode runs all of it every step):

  rank 0 holds the image pool (u8 [*,224,224,3], HBM-resident)
   -> grouped ncclSend/ncclRecv of one u8 shard (per_gpu_batch images) to
      every other rank, one step ahead on a high-priority comm stream
   -> on every GPU: preprocess + ResNet18 (hand-written MFMA kernels,
      hipGraph replay) + fused softmax/top-1
   -> grouped send/recv of (top-1 class, probability) back to rank 0 on a
      second communicator/stream, then a D2H of the answers.

Input modes (--input-mode):
  scatter (default) the per-step scatter above: every step moves each rank's
                    u8 shard (38.5 MB at 256 images) from rank 0's HBM over
                    RCCL, one step ahead of its forward. Rank 0 drives all the
                    send legs, and RCCL's copy kernels next to a forward slow
                    it ~1.2x (they hold CUs the one-workgroup-per-CU convs
                    need, profiles/r2_rccl_interference.txt), so rank 0
                    classifies --coord-weight x per_gpu_batch images and every
                    other rank per_gpu_batch (never more: 256 = the CU count,
                    and the one-workgroup-per-image kernels would run a second
                    round); global_batch = the sum, in the JSON.
  staged            rank 0's images are scattered to the ranks over RCCL once,
                    before timing (SDFS shard replicas placed in the HBM of the
                    GPU that serves them, as predict-shard does); every timed
                    step classifies the rank's HBM-resident shard and gathers
                    the answers to rank 0 over RCCL (8 B per image, one CTA).
  local             each rank generates its own shard (no transfer at all).
At N = 1 all three run the same forward.

A plain run sets up, primes, warms up, times the --steps pipelined steps and
prints the JSON line (the latency fields are null). ``--full`` adds the
measurements that take runs of their own: the unpipelined per-batch latency
(--latency-steps), the batch-1 GPU latency (--latency-queries), the query
latency through a dmlc-node cluster (--e2e-queries), and the sanity check of
the gathered answers. ``--dump-outputs DIR`` writes the answers of the last
timed step (what the coordinator receives: every image's top-1 class and its
probability) as DIR/top1_class.npy and DIR/top1_prob.npy, float32, in the
order of the global batch; models, images and the step -> batch mapping are
seeded, so two builds run with the same arguments can be compared.

Reference numbers (CS425MP4Report.pdf p.2): ResNet18 mean query latency
158.94 ms on CPU VMs, i.e. 6.29 images/s for one query stream; there is no
published images/s figure, so ``vs_baseline`` divides by that derived rate.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REF_MEAN_LATENCY_MS = 158.94  # ResNet18, CS425MP4Report.pdf p.2 §1a
REF_STREAM_IMG_S = 1000.0 / REF_MEAN_LATENCY_MS
# rank 0's share in scatter mode (it also runs the N-1 send legs, and RCCL's
# copy kernels next to its forward slow it: ~1.2x measured with one rank,
# profiles/r2_rccl_interference.txt). No multi-GPU measurement exists to seed
# it with, so at N > 1 bench.py starts from an even split and calibrates
# (--coord-weight auto, csrc/comm/runner.h Runner::calibrate): rounds of
# pipelined steps, every rank's forward time all-gathered, rank 0's count
# re-solved until its forward time matches the slowest other rank's.
COORD_WEIGHT = 1.0


def pct(xs, q):
    xs = sorted(xs)
    if not xs:
        return None
    k = (len(xs) - 1) * q / 100.0
    lo, hi = int(k), min(int(k) + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (k - lo)


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n: int) -> int:
    """Start n rank processes of this script (no GPU touched in the parent)."""
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env))
    rc = 0
    for p in procs:
        rc = max(rc, p.wait())
    return rc


def preflight(n_gpus: int, local_rank: int | None = None) -> None:
    """Enough GPUs for the ranks (torch.cuda.device_count() does not
    initialise the GPU, so the spawning parent may call it)."""
    import torch
    n = torch.cuda.device_count()
    if n < n_gpus or (local_rank is not None and local_rank >= n):
        raise SystemExit(f"bench.py: --gpus {n_gpus} (local rank {local_rank}) but {n} GPU(s) visible")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--batch", type=int, default=256, help="images per GPU per step")
    ap.add_argument("--input-mode", choices=["staged", "scatter", "local"], default="scatter")
    ap.add_argument("--coord-weight", default="auto",
                    help="rank 0's share of a step as a fraction of a fair share (scatter mode): a number, or "
                         f"'auto' (N > 1: calibrated during the prime steps starting from {COORD_WEIGHT}; N = 1: 1)")
    ap.add_argument("--calib-rounds", type=int, default=5, help="coordinator-share calibration rounds (auto)")
    ap.add_argument("--calib-steps", type=int, default=8, help="pipelined steps per calibration round")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--engine-opt", action="append", default=[], metavar="NAME=0|1",
                    help="engine kernel-path switch (EngineOptions field), for A/B runs; repeatable")
    ap.add_argument("--lanes", type=int, default=2, choices=[1, 2, 3, 4],
                    help="model instances per GPU on alternating streams (2: step i+1 starts under step i's tail)")
    ap.add_argument("--prime-steps", type=int, default=40,
                    help="untimed pipeline steps at setup, before the --warmup steps (brings the GPU clocks up: "
                         "measured 267k img/s after 5 warmup steps alone vs 290k after 30, profiles/r2_warmup_ramp.txt)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: batch latency, batch-1 GPU latency, "
                         "query latency through a dmlc-node cluster, and the check of the gathered answers")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's answers (top-1 class and probability of every image of the "
                         "global batch) to DIR/top1_class.npy and DIR/top1_prob.npy (float32)")
    ap.add_argument("--latency-steps", type=int, default=50, help="(--full) unpipelined steps for the batch latency")
    ap.add_argument("--latency-queries", type=int, default=200,
                    help="(--full) batch-1 GPU queries (GPU-only latency)")
    ap.add_argument("--profile-ops", action="store_true", help="print per-op times of one eager forward")
    ap.add_argument("--e2e-queries", type=int, default=200,
                    help="(--full) queries through a dmlc-node cluster for the reference-definition query latency (0: skip)")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU: every rank a process with a host worker (a forward of B images takes "
                         "B x --dry-us-per-image of modelled time, + --dry-coord-extra-us on rank 0 for its send "
                         "legs) on the cross-process socket communicator; the rest of the path (spawn, gloo, "
                         "unique ids, calibration all-gather, per-rank max, JSON) is the real one")
    ap.add_argument("--dry-us-per-image", type=int, default=4)
    ap.add_argument("--dry-coord-extra-us", type=int, default=200)
    ap.add_argument("--image-size", type=int, default=224, help="(--dry-run only; the models take 224)")
    args = ap.parse_args()
    dry = args.dry_run
    S = args.image_size if dry else 224

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        if not dry:
            preflight(args.gpus)
        sys.exit(spawn_ranks(args.gpus))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if dry:
        dev = torch.device("cpu")
    else:
        preflight(args.gpus, local_rank)
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    if world > 1:
        # CPU side channel only: unique ids, barriers, max of the timed region
        dist.init_process_group("gloo", rank=rank, world_size=world)

    import dmlc
    from dmlc.models import build, state_dict_f32
    from dmlc.runtime import InferenceEngine

    C = dmlc.native()
    B = args.batch
    scatter = args.input_mode == "scatter"  # per-step RCCL scatter (staged: once, before timing)
    opts = {k: bool(int(v)) for k, v in (o.split("=", 1) for o in args.engine_opt)}
    use_graph = not args.no_graph
    eng = sd = None
    if not dry:
        # one compute lane: the stream convs' workgroup start stagger (set
        # before any graph captures the launches; csrc/kernels/stagger.hip)
        C.kernel_stagger_for_lanes(args.lanes)
        # Random-init weights (the reference's .ot files are LFS stubs); every
        # rank builds the same seeded model.
        sd = state_dict_f32(build(args.model, seed=0))
        eng = InferenceEngine(args.model, sd, device=local_rank, max_batch=B, options=opts)

    ids = [b"", b""]
    if world > 1:
        new_id = C.socket_unique_id if dry else C.rccl_unique_id
        box = [[new_id(), new_id()] if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        ids = box[0]
    auto_weight = args.coord_weight == "auto" and world > 1 and scatter
    if args.coord_weight == "auto":
        coord_weight = COORD_WEIGHT if world > 1 else 1.0
    else:
        coord_weight = float(args.coord_weight)
    if not scatter:
        coord_weight = 1.0  # nothing to send per step: an even split
    if dry:
        runner = C.DpRunner.host(world, rank, ids[0], ids[1], B, scatter=scatter, image_size=S, lanes=args.lanes,
                                 coord_weight=coord_weight, us_per_image=args.dry_us_per_image,
                                 coord_extra_us=args.dry_coord_extra_us)
    else:
        runner = C.DpRunner(eng._e, world, rank, ids[0], ids[1], B, scatter=scatter, use_graph=use_graph,
                            lanes=args.lanes, coord_weight=coord_weight)
    counts = runner.counts  # images per rank per step (sum = B * world)
    M = runner.max_per_rank

    def sync():
        if not dry:
            torch.cuda.synchronize()

    # Input pool: two global batches of distinct synthetic images, in the
    # coordinator's HBM (scatter), staged from there into every rank's HBM
    # (staged), or generated by every rank (local).
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    pool = None
    n_pool = 0
    if args.input_mode == "staged":
        n_pool = 2 * M  # two per-rank batches at a stride of max_per_rank images
        pool = torch.empty((n_pool, S, S, 3), dtype=torch.uint8, device=dev)
        src = torch.randint(0, 256, (2, world * B, S, S, 3), dtype=torch.uint8, device=dev,
                            generator=g) if rank == 0 else None
        sync()
        for k in range(2):  # batch k: rank r's shard = its count's images of src[k]
            runner.stage(src[k].data_ptr() if rank == 0 else 0, pool[k * M].data_ptr())
        staged_src = src if dry else None  # (dry run: rank 0 checks the answers against it)
        del src
    elif rank == 0 or not scatter:
        n_pool = 2 * (B * world if scatter else M)
        pool = torch.randint(0, 256, (n_pool, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
    pool_ptr = pool.data_ptr() if pool is not None else 0
    sync()

    def barrier():
        sync()
        if world > 1:
            dist.barrier()
        sync()

    # Setup: prime the pipeline (hipGraph capture of every slot, RCCL
    # channels, and ~35 ms of load so the GPU leaves its idle clocks; a fixed
    # step count, the same on every rank), then the W warmup steps.
    calibration = None
    if args.prime_steps > 0:
        runner.run(pool_ptr, n_pool, 0, args.prime_steps)
        barrier()
    if auto_weight and args.calib_rounds > 0:
        def allgather(x):
            t = torch.tensor([x], dtype=torch.float64)
            out = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(out, t)
            return [float(v) for v in out]
        calibration = runner.calibrate(pool_ptr, n_pool, args.prime_steps, args.calib_steps, args.calib_rounds,
                                       0.05, allgather)
        coord_weight = calibration["weight"]
        counts = runner.counts
        barrier()
    runner.run(pool_ptr, n_pool, 0, args.warmup)
    barrier()
    t0 = time.perf_counter()
    runner.run(pool_ptr, n_pool, args.warmup, args.steps)
    barrier()
    elapsed = time.perf_counter() - t0
    per_rank_s = [elapsed]
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        gathered = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(gathered, t)
        per_rank_s = [float(x) for x in gathered]
        elapsed = max(per_rank_s)

    full = args.full
    if rank == 0 and args.dump_outputs:
        # the last timed step's gathered answers, in global-batch order
        import numpy as np
        idx, prob = runner.last_results()
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "top1_class.npy"), np.asarray(idx, dtype=np.float32))
        np.save(os.path.join(args.dump_outputs, "top1_prob.npy"), np.asarray(prob, dtype=np.float32))

    # Per-batch latency: unpipelined steps, scatter issue -> answers on the
    # coordinator's host.
    n_lat = args.latency_steps if full else 0
    batch_lat = []
    if n_lat > 0:
        lat = runner.run(pool_ptr, n_pool, args.warmup + args.steps, n_lat, pipelined=False)
        batch_lat = lat["step_ms"]
        barrier()

    # (a dry run exists to check the path, so it always checks its answers)
    answers_checked = False
    if rank == 0 and (full or dry):
        idx, prob = runner.last_results()
        assert len(idx) == sum(counts)
        assert min(idx) >= 0 and max(idx) < 1000, "bad class ids"
        assert min(prob) > 0 and max(prob) <= 1.0001, "bad probabilities"
        if dry and args.input_mode != "local":
            # the host worker's answer is a function of the image's bytes
            # (csrc/comm/dp.h make_host_worker): the last step's gathered
            # answers must be those of the images that step was given
            G = sum(counts)
            last = args.warmup + args.steps + n_lat - 1
            if scatter:
                imgs = pool[:(n_pool // G) * G].view(-1, G, S, S, 3)[last % (n_pool // G)]
            else:
                imgs = staged_src[last % 2][:G]
            want = (imgs.reshape(G, -1).sum(1, dtype=torch.int64) % 1000).tolist()
            assert list(idx) == want, "dry run: gathered answers do not match their images"
            answers_checked = True

    # Batch-1 GPU-only latency (hipGraph replay of preprocess+forward+top-1
    # for one HBM-resident image, host-timed including the D2H of the
    # answer). Not the reference's query definition (which includes the RPC
    # and the JPEG decode): that one is tools/bench_jobs.py's.
    qlat = []
    if rank == 0 and full and args.latency_queries > 0 and not dry:
        q_eng = InferenceEngine(args.model, sd, device=local_rank, max_batch=1, options=opts)
        qimg = pool[:1].contiguous()
        qout = (torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.float32, device=dev))
        for i in range(args.latency_queries + 20):
            torch.cuda.synchronize()
            t = time.perf_counter()
            q_eng.predict(qimg, out=qout)
            _ = qout[0].item()
            if i >= 20:
                qlat.append((time.perf_counter() - t) * 1e3)

    # Query latency with the reference's definition (connect + RPC + JPEG
    # decode + resize + forward + top-1, one query at a time) through a
    # one-node dmlc-node cluster on this GPU.
    e2e = None
    if rank == 0 and full and args.e2e_queries > 0 and not dry:
        try:
            from dmlc.serve.e2e import query_latency
            e2e = query_latency(args.e2e_queries, args.model if args.model in ("resnet18", "alexnet") else "resnet18",
                                device=local_rank)
        except Exception as ex:  # noqa: BLE001  (reported, never fails the throughput bench)
            print(f"# e2e query latency failed: {ex}", file=sys.stderr)

    ops_profile = None
    if rank == 0 and args.profile_ops and not dry:
        ops_profile = eng.profile(pool[:B].contiguous())

    if rank == 0:
        n_img = sum(counts) * args.steps
        value = n_img / elapsed
        res = {
            "metric": ("DRY RUN (host workers, no GPU): " if dry else "")
                      + "images/sec (whole node) + p50/p95 query latency, "
                      + ("ResNet18" if args.model == "resnet18" else args.model) + " ImageNet",
            "value": round(value, 1),
            "unit": "images/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(value / REF_STREAM_IMG_S, 1) if args.model == "resnet18" else None,
            "dtype": "fp8" if args.model.endswith("_fp8") else "bf16",
            "data": (f"DRY RUN: host workers ({args.dry_us_per_image} us/image modelled, +{args.dry_coord_extra_us} "
                     f"us per forward on rank 0), socket communicator; synthetic u8 {S}x{S}x3 images; " if dry
                     else "synthetic u8 224x224x3 images, random-init weights; ")
                    + {"staged": "generated on rank 0, shards scattered to the ranks' HBM over RCCL before timing",
                       "scatter": "HBM-resident on rank 0, scattered over RCCL every step",
                       "local": "generated in every rank's HBM"}[args.input_mode],
            "prime_steps": args.prime_steps,
            "config": {
                "model": args.model,
                "global_batch": sum(counts),
                "per_gpu_batch": B,
                "per_rank_counts": counts,
                "coord_weight": round(coord_weight, 4),
                "coord_weight_mode": "calibrated" if calibration else ("fixed" if world > 1 else "n/a"),
                "seq_len": None,
                "image_size": S,
                "parallelism": f"dp{world}",
                "input_mode": args.input_mode,
                "comm": ("socket (dry run) " if dry else "native RCCL ")
                        + "grouped send/recv (csrc/comm/runner.h), shards + answers on separate communicators"
                    + ("" if scatter else "; per step: answers only"),
                "rccl_ranks": world,
                "hipgraph": use_graph,
                "lanes": args.lanes,
                "prime_steps": args.prime_steps,
                "baseline": "6.29 img/s = one query stream at the reference's 158.94 ms mean ResNet18 latency "
                            "(CS425MP4Report.pdf p.2; no images/s is published)",
            },
            "per_rank_images_s": [round(c * args.steps / s, 1) for c, s in zip(counts, per_rank_s)],
            "batch_latency_p50_ms": round(pct(batch_lat, 50), 3) if batch_lat else None,
            "batch_latency_p95_ms": round(pct(batch_lat, 95), 3) if batch_lat else None,
            "query_latency_mean_ms": round(e2e["mean_ms"], 3) if e2e else None,
            "query_latency_p50_ms": round(e2e["p50_ms"], 3) if e2e else None,
            "query_latency_p95_ms": round(e2e["p95_ms"], 3) if e2e else None,
            "query_latency_def": "reference definition (src/services.rs:419-424): a new TCP connection per query "
                                 "(--new-conn-per-query) + RPC + JPEG decode + resize + forward + top-1 through a "
                                 "one-node dmlc-node cluster, one query in flight; "
                                 + (e2e["data"] if e2e else "not measured"),
            "vs_baseline_latency": round(REF_MEAN_LATENCY_MS / e2e["mean_ms"], 1) if e2e else None,
            "gpu_batch1_latency_p50_ms": round(pct(qlat, 50), 4) if qlat else None,
            "gpu_batch1_latency_p95_ms": round(pct(qlat, 95), 4) if qlat else None,
            "tflops_effective": round(value * eng.gflop_per_image / 1e3, 1) if eng else None,
            "dry_run": dry,
            "full": full,
        }
        if dry:
            res["answers_checked"] = answers_checked
        if calibration:
            res["calibration"] = [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
                                  for r in calibration["rounds"]]
        if ops_profile:
            print("# per-op (ms): " + ", ".join(f"{n}={t:.3f}" for n, t in ops_profile), file=sys.stderr)
        print(json.dumps(res), flush=True)

    del runner
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""bench.py's multi-process N > 1 path, end to end on the CPU (VERDICT r5
Missing 1): `bench.py --gpus N --dry-run` runs as N processes — spawned by
bench.py itself (spawn_ranks) or by torch.distributed.run exactly as the
driver launches it — through gloo init, the unique-id broadcast, the native
dp::Runner on host workers and the cross-process socket communicator
(csrc/comm/socket_comm.cpp: RCCL's one-rank-per-process shape with the host
fake's rendezvous / FIFO / group rules), the coordinator-share calibration's
all-gather, the per-rank max of the timed region, and the JSON line.

The host worker models a forward of B images as B x 4 us (+200 us on rank 0
for its send legs), so the calibration has a known answer: from an even split
rank 0's forward takes 1224 vs 1024 us, the solver moves its share to
1024/1224 = 0.8366 (214 of 256 images), where it is within the 5% tolerance.
Rank 0 also checks the gathered answers of the last step against its images
(the host worker's class is a function of the image bytes).
"""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = ["--full", "--steps", "4", "--warmup", "2", "--prime-steps", "4", "--calib-steps", "4", "--latency-steps", "2"]


def _json_line(out: str) -> dict:
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-3000:]
    return json.loads(lines[0])


def _run(cmd, timeout=240):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return _json_line(r.stdout)


def _check(d, n, mode):
    cfg = d["config"]
    counts = cfg["per_rank_counts"]
    assert d["dry_run"] is True and d["answers_checked"] is True
    assert d["n_gpus"] == n and cfg["rccl_ranks"] == n and cfg["parallelism"] == f"dp{n}"
    assert len(counts) == n and cfg["global_batch"] == sum(counts)
    assert d["value"] > 0 and d["steps"] == 4 and d["warmup"] == 2
    assert len(d["per_rank_images_s"]) == n
    if mode == "scatter":
        assert cfg["coord_weight_mode"] == "calibrated"
        assert counts == [214] + [256] * (n - 1), counts
        assert abs(cfg["coord_weight"] - 1024 / 1224) < 1e-3, cfg["coord_weight"]
        rounds = d["calibration"]
        assert rounds[0]["coord_count"] == 256 and rounds[-1]["coord_count"] == 214
        assert abs(rounds[0]["busy_coord_ms"] - 1.224) < 1e-6 and abs(rounds[0]["busy_worker_ms"] - 1.024) < 1e-6
    else:
        assert counts == [256] * n and cfg["coord_weight"] == 1.0


@pytest.mark.slow
@pytest.mark.parametrize("n,mode,size", [(4, "scatter", 224), (4, "staged", 224), (8, "scatter", 112),
                                         (8, "staged", 112)])
def test_bench_dry_run_spawned(n, mode, size):
    d = _run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dry-run", "--input-mode", mode,
              "--image-size", str(size), *SHORT])
    _check(d, n, mode)


@pytest.mark.slow
def test_bench_dry_run_under_torchrun():
    """The driver's own launch: torch.distributed.run with a 127.0.0.1 rendezvous."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    d = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4",
              "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
              "--gpus", "4", "--dry-run", "--image-size", "112", *SHORT])
    _check(d, 4, "scatter")


def test_bench_preflight_refuses_missing_gpus():
    """The real (non-dry) path checks torch.cuda.device_count() before it
    spawns ranks: on this GPU-less host --gpus 2 stops with a message."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], cwd="/tmp",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "GPU(s) visible" in (r.stderr + r.stdout)

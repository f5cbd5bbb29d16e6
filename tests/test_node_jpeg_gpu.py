"""dmlc-node with --jpeg-gpu: a cache miss is entropy-decoded on the host and
finished on the GPU (csrc/kernels/jpeg_finish.hip) straight into the image's
HBM cache block. Classification agrees with the CPU executor, and a one-node
cluster serves a job from images that all took the GPU path."""
import os
import re
import subprocess
import time

import pytest

from dmlc.serve.cluster import NODE_BIN, LocalCluster
from dmlc.utils.dataset import make_synthetic_dataset, synthetic_labels, write_labels
from dmlc.utils.ot import write_random_checkpoint

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    root = tmp_path_factory.mktemp("jpeggpu")
    labels = synthetic_labels(1000)
    lab = write_labels(str(root / "synset_words.txt"), labels)
    sizes = [(224, 224), (375, 500), (500, 333), (256, 300), (480, 640), (199, 211), (224, 300), (640, 427)]
    ds = make_synthetic_dataset(str(root / "ragged"), labels[:16], size=sizes, seed=9)
    ckpt = write_random_checkpoint("resnet18", str(root / "resnet18.ot"), seed=4)
    return {"root": root, "labels": lab, "dataset": ds, "ckpt": ckpt, "entries": labels}


def _classify(env, images, *extra):
    r = subprocess.run([NODE_BIN, "classify", "--model", "resnet18", "--weights", env["ckpt"], "--labels",
                        env["labels"], "--image", ",".join(images), *extra],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [int(x) for x in re.findall(r"class=(\d+)", r.stdout)], r.stdout


def test_classify_with_gpu_jpeg_finish_agrees_with_cpu(gpu, env):
    imgs = []
    for wnid, _ in env["entries"][:16]:
        d = os.path.join(env["dataset"], wnid)
        imgs.append(os.path.join(d, sorted(os.listdir(d))[0]))
    g, out = _classify(env, imgs, "--executor", "gpu", "--jpeg-gpu")
    c, _ = _classify(env, imgs, "--executor", "cpu")
    assert "[gpu:0]" in out
    assert len(g) == len(c) == 16
    agree = sum(a == b for a, b in zip(g, c))
    assert agree >= 14, (g, c)  # the bar of test_node_gpu.py for the same comparison


def test_cluster_job_decodes_every_image_on_the_gpu(gpu, env, tmp_path):
    cl = LocalCluster(1, 19900, str(tmp_path / "c"), env["labels"], n_leaders=1, executor="gpu",
                      dataset=env["dataset"], models=f"resnet18={env['ckpt']}",
                      extra=["--jobs", "resnet18", "--job-limit", "16", "--query-interval-ms", "20",
                             "--query-batch", "4", "--quiet-predictions", "--prefetch", "--jpeg-gpu"])
    with cl:
        n = cl.nodes[0]
        deadline = time.time() + 60
        while time.time() < deadline:
            m = re.search(r"prefetched (\d+)", n.cmd("info"))
            if m and int(m.group(1)) >= 16:
                break
            time.sleep(0.2)
        n.cmd("predict")
        deadline = time.time() + 60
        done = 0
        while time.time() < deadline:
            m = re.search(r"Accuracy: \d+/(\d+)", n.cmd("jobs"))
            done = int(m.group(1)) if m else 0
            if done >= 16:
                break
            time.sleep(0.5)
        assert done == 16
        info = n.cmd("info")
        assert re.search(r"jpeg gpu 16 cpu 0", info), info

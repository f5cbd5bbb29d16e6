"""Host-only audit of the features plan (Engine::plan(..., features=True)), no GPU needed.

A forward with a features buffer runs the plan without one, step for step,
plus one last Embed step (after SoftmaxTopK when there is one) that covers no
op. The step reads F, the input activation of the fc that writes the logits,
wherever a step of the plan stores F; where HeadFused pools inside the head, F
is never written, and the step pools the last conv's stored output itself
(detail ``in=<that conv> hw=49``).
"""
import pytest

from dmlc import native
from dmlc.models import build, state_dict_f32

CUS = 256
ARCHS = ("resnet18", "resnet50", "resnet50_fp8", "alexnet")
BATCHES = (1, 4, 64, 256)
CASES = [(a, B, nat, k) for a in ARCHS for B in BATCHES for nat in (True, False) for k in (1, 5)]


@pytest.fixture(scope="module")
def audit():
    C = native()
    weights = {}

    def get(arch, B, nat, topk, **kw):
        base = arch.replace("_fp8", "")
        if base not in weights:
            sd = state_dict_f32(build(base, seed=0))
            weights[base] = {k: v.detach().cpu().float().numpy() for k, v in sd.items()}
        return C.plan_audit(arch, weights[base], {}, B, nat, CUS, topk=topk, **kw)
    return get


def _producer(ops, act):
    (name,) = [n for n, _, out, _ in ops if out == act]
    return name


@pytest.mark.parametrize("arch,B,nat,topk", CASES, ids=[f"{a}-b{B}-{'native' if n else 'resized'}-k{k}"
                                                         for a, B, n, k in CASES])
def test_features_plan(audit, arch, B, nat, topk):
    plain, ops = audit(arch, B, nat, topk)
    off, ops_off = audit(arch, B, nat, topk, features=False)
    assert off == plain and ops_off == ops
    assert "Embed" not in [k for k, _, _, _ in plain]

    feat, ops_on = audit(arch, B, nat, topk, features=True)
    assert ops_on == ops
    assert feat[:-1] == plain and len(feat) == len(plain) + 1
    kernel, first, n_ops, detail = feat[-1]
    assert kernel == "Embed" and n_ops == 0 and first == ops[-1][0]
    assert [k for k, _, _, _ in feat].count("Embed") == 1
    tail = plain[-1]
    if topk == 5:
        assert tail[0] == "SoftmaxTopK" and feat[-2] == tail
        tail = plain[-2]
    else:
        assert "SoftmaxTopK" not in [k for k, _, _, _ in plain]

    # F = the input of the fc that writes the logits (the last op, softmax / top-1, reads them)
    (fc,) = [op for op in ops if op[2] == ops[-1][1]]
    d = dict(f.split("=") for f in detail.split())
    if tail[0] == "HeadFused":
        assert tail[1] == "avgpool" and tail[2] == 3
        (pool,) = [op for op in ops if op[0] == "avgpool"]
        assert pool[2] == fc[1]
        assert d == {"in": _producer(ops, pool[1]), "hw": "49"}
        assert ".conv" in d["in"] and d["in"].startswith("layer4.")
        # that conv's launch stores its output
        names, cover, pos = [o[0] for o in ops], {}, 0
        for s in plain:
            cover.update({names[pos + i]: s for i in range(s[2])})
            pos += s[2]
        st = cover[d["in"]]
        assert st[0] != "None" and names.index(st[1]) + st[2] - 1 == names.index(d["in"])
        assert "nostore" not in st[3].split()
    else:
        assert d == {"in": _producer(ops, fc[1])}
        assert d["in"] == ("classifier.4" if arch == "alexnet" else "avgpool")


def test_head_fused_only_at_query_batches(audit):
    """The pooling form is what the query batches take, the stored row what the throughput batches take."""
    for arch in ("resnet18", "resnet50", "resnet50_fp8"):
        for B, fused in ((1, True), (4, True), (64, False), (256, False)):
            feat, _ = audit(arch, B, True, 1, features=True)
            assert (feat[-2][0] == "HeadFused") == fused, (arch, B)
            assert ("hw=49" in feat[-1][3].split()) == fused, (arch, B)

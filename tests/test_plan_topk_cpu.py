"""Host-only audit of the top-k launch plan (Engine::plan with topk > 1), no
GPU needed: a top-k forward is the top-1 forward, step for step, plus one
final SoftmaxTopK launch on the logits the tail wrote.
"""
import pytest

from dmlc import native
from dmlc.models import build, state_dict_f32

CUS = 256
ARCHS = ("resnet18", "resnet50", "resnet50_fp8", "alexnet")
BATCHES = (1, 64, 256)


@pytest.fixture(scope="module")
def weights():
    cache = {}

    def get(arch):
        base = arch.replace("_fp8", "")
        if base not in cache:
            sd = state_dict_f32(build(base, seed=0))
            cache[base] = {k: v.detach().cpu().float().numpy() for k, v in sd.items()}
        return cache[base]
    return get


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("arch", ARCHS)
def test_topk_plan_is_top1_plan_plus_one_step(weights, arch, B):
    C = native()
    w = weights(arch)
    plain, plain_ops = C.plan_audit(arch, w, {}, B, True, CUS)
    one, one_ops = C.plan_audit(arch, w, {}, B, True, CUS, topk=1)
    five, five_ops = C.plan_audit(arch, w, {}, B, True, CUS, topk=5)
    assert one == plain and one_ops == plain_ops
    assert five_ops == plain_ops
    assert len(five) == len(plain) + 1
    assert five[:-1] == plain
    kernel, first_op, n_ops, detail = five[-1]
    assert kernel == "SoftmaxTopK"
    assert first_op == plain_ops[-1][0] and n_ops == 0  # belongs to the last op, covers none
    assert detail == "k=5"
    assert "SoftmaxTopK" not in [k for k, _, _, _ in plain]


def test_topk_plan_rejects_bad_k(weights):
    C = native()
    w = weights("resnet18")
    for k in (0, -1, C.MAX_TOPK + 1):
        with pytest.raises(ValueError):
            C.plan_audit("resnet18", w, {}, 4, True, CUS, topk=k)
    assert C.plan_audit("resnet18", w, {}, 4, True, CUS, topk=C.MAX_TOPK)[0][-1][3] == f"k={C.MAX_TOPK}"

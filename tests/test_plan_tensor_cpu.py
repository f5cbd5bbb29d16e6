"""Host-only audit of the tensor-input launch plan (Engine::plan with
tensor_in), no GPU needed: a forward on a float tensor is the forward on
resized u8 input (native = False), step for step, except that the step writing
the stem's packed image is PackTensor instead of Preprocess. None of the
kernels that read u8 images may appear.
"""
import pytest

from dmlc import native
from dmlc.models import build, state_dict_f32

CUS = 256
ARCHS = ("resnet18", "resnet50", "resnet50_fp8", "alexnet")
BATCHES = (1, 64, 256)
U8_KERNELS = {"StemPoolU8", "AlexStem", "Preprocess"}


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


@pytest.mark.parametrize("topk", (1, 5))
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("arch", ARCHS)
def test_tensor_plan_is_resized_plan_with_pack_tensor(weights, arch, B, topk):
    C = native()
    w = weights(arch)
    resized, resized_ops = C.plan_audit(arch, w, {}, B, False, CUS, topk=topk)
    tensor, tensor_ops = C.plan_audit(arch, w, {}, B, False, CUS, topk=topk, tensor_in=True)
    assert tensor_ops == resized_ops
    assert len(tensor) == len(resized)
    differing = [(t, r) for t, r in zip(tensor, resized) if t != r]
    assert len(differing) == 1
    (t, r), = differing
    assert t[0] == "PackTensor" and r[0] == "Preprocess" and t[1:] == r[1:]
    kernels = [k for k, _, _, _ in tensor]
    assert kernels.count("PackTensor") == 1
    assert not U8_KERNELS & set(kernels)
    # `native` is not looked at: there is one tensor plan
    assert C.plan_audit(arch, w, {}, B, True, CUS, topk=topk, tensor_in=True) == (tensor, tensor_ops)


@pytest.mark.parametrize("native_size", (True, False))
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("arch", ARCHS)
def test_tensor_in_false_is_the_existing_plan(weights, arch, B, native_size):
    C = native()
    w = weights(arch)
    for topk in (1, 5):
        plain = C.plan_audit(arch, w, {}, B, native_size, CUS, topk=topk)
        assert C.plan_audit(arch, w, {}, B, native_size, CUS, topk=topk, tensor_in=False) == plain
        assert "PackTensor" not in [k for k, _, _, _ in plain[0]]


def test_tensor_plan_without_the_fused_stem(weights):
    """fused_stem off: the unpaired image, then conv1 and maxpool as for resized u8 input."""
    C = native()
    w = weights("resnet18")
    opts = {"fused_stem": False}
    resized, _ = C.plan_audit("resnet18", w, opts, 64, False, CUS)
    tensor, _ = C.plan_audit("resnet18", w, opts, 64, False, CUS, tensor_in=True)
    assert tensor[0][0] == "PackTensor" and resized[0][0] == "Preprocess"
    assert tensor[1:] == resized[1:]

"""EngineOptions::small_1x1 on the host (plan_audit, no GPU): at query batches
every 1x1 conv that ResNet50's default plan runs on the implicit GEMM, conv1x1
(alone or chained) or a fused layer1 bottleneck kernel is a Small1x1 step
(conv1x1_small.hip), layer1.0's K-concatenated expand + downsample stays, and
outside the option's range the plan is the default one. The set of convs is
read off the default plan, the engine's op list and the weights' shapes.
"""
import pytest

from dmlc import native

from _golden_weights import golden_weights

CUS = 256
ARCHS = {"resnet50": {}, "resnet50_fp8": {"small_conv8": True}}
OLD = ("Igemm", "Conv1x1", "Conv1x1Chain", "Bottleneck56", "Bottleneck56Head")


def audit(arch, opts, B):
    lines, ops = native().plan_audit(arch, golden_weights(arch), opts, B, True, CUS)[:2]
    return lines, ops


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("arch", list(ARCHS))
def test_small1x1_plan(arch, B):
    base, ops = audit(arch, ARCHS[arch], B)
    on, _ = audit(arch, {**ARCHS[arch], "small_1x1": True}, B)
    names = [o[0] for o in ops]
    w = golden_weights(arch)
    one = {n for n in names if n + ".weight" in w and w[n + ".weight"].ndim == 4 and w[n + ".weight"].shape[-1] == 1}
    # the 1x1 conv ops inside the default plan's steps on the old kernels
    moved = set()
    for kernel, first, n, _ in base:
        if kernel in OLD:
            i = names.index(first)
            moved |= one & set(names[i:i + n])
    assert len(moved) >= 30
    by = {first: (kernel, n) for kernel, first, n, _ in on}
    for name in moved:
        assert by[name][0] == "Small1x1" and by[name][1] == 1, (name, by.get(name))
    assert not any(k.startswith("Bottleneck56") or k == "Conv1x1Chain" for k, _ in by.values())
    assert [l for l in on if l[0] == "Conv1x1Cat"] == [l for l in base if l[0] == "Conv1x1Cat"] != []
    # every op lies in exactly one step
    covered = [nm for _, first, n, _ in on for nm in names[names.index(first):names.index(first) + n]]
    assert sorted(covered) == sorted(names)


@pytest.mark.parametrize("arch", list(ARCHS))
def test_small1x1_plan_outside_the_option(arch):
    above = native().kSmall1x1MaxB + 1
    assert audit(arch, {**ARCHS[arch], "small_1x1": True}, above)[0] == audit(arch, ARCHS[arch], above)[0]
    assert audit(arch, {**ARCHS[arch], "small_1x1": False}, 1)[0] == audit(arch, ARCHS[arch], 1)[0]
    assert all(k != "Small1x1" for k, _, _, _ in audit(arch, ARCHS[arch], 1)[0])


@pytest.mark.parametrize("arch", ["resnet18", "alexnet"])
def test_small1x1_leaves_other_models(arch):
    for B in (1, 4):
        assert audit(arch, {"small_1x1": True}, B)[0] == audit(arch, {}, B)[0]

"""EngineOptions::small_conv8 on the host (plan_audit, no GPU): at query
batches every e4m3-in 3x3 conv of the fp8 ResNets is a Small8 step
(conv_small8.hip), layer4.0's downsample of the basic-block models rides in its
conv1's launch, and outside the option's range the plan is the default one.

The e4m3-in 3x3 convs are read off the default plan at a batch that fills a
256-CU device, where they are the Stream8 steps.
"""
import pytest

from dmlc import native

from _golden_weights import golden_weights

CUS = 256
FULL_B = {"resnet18_fp8": 64, "resnet34_fp8": 64, "resnet50_fp8": 256}
ON = {"small_conv8": True}


def plan(arch, opts, B):
    return native().plan_audit(arch, golden_weights(arch), opts, B, True, CUS)[0]


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("arch", list(FULL_B))
def test_small8_plan(arch, B):
    full = plan(arch, {}, FULL_B[arch])
    convs = {first: detail for kernel, first, _, detail in full if kernel == "Stream8"}
    assert len(convs) >= 7  # resnet18_fp8: layers 3-4 without layer3.0.conv1
    by = {first: (kernel, detail) for kernel, first, _, detail in plan(arch, ON, B)}
    for name, full_detail in convs.items():
        kernel, detail = by[name]
        assert kernel == "Small8", (name, kernel)
        # the downsample the Stream8 launch computes is computed by this one; then mf
        assert detail in [" ".join(filter(None, (full_detail, f"mf={mf}"))) for mf in (1, 2, 4)], (name, detail)
    if arch != "resnet50_fp8":
        assert by["layer4.0.downsample.0"] == ("None", "")
        assert by["layer4.0.conv1"][1].startswith("ds=layer4.0.downsample.0 mf=")
    assert sum(k == "Small8" for k, _ in by.values()) == len(convs)


@pytest.mark.parametrize("arch", list(FULL_B))
def test_small8_plan_outside_the_option(arch):
    """Above kSmallConv8MaxB with the option on, and at B = 1 with it off, the
    plan is the default options' plan line for line."""
    above = native().kSmallConv8MaxB + 1
    assert plan(arch, ON, above) == plan(arch, {}, above)
    assert plan(arch, {"small_conv8": False}, 1) == plan(arch, {}, 1)
    assert all(k != "Small8" for k, _, _, _ in plan(arch, {}, 1))

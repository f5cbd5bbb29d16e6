"""alexnet_fp8 on the host (plan_audit, pack_audit; no GPU): one op quantises
the classifier's input, classifier.1 / .4 read e4m3 on fc_small8 up to 16
images, fc_gemm8 up to 256, the e4m3 implicit GEMM above that and with fc8 off;
classifier.6 stays on `alexnet`'s bf16 paths.
"""
import pytest

from dmlc import native
from dmlc.models import build, state_dict_f32

CUS = 256


@pytest.fixture(scope="module")
def weights():
    return {k: v.detach().cpu().float().numpy() for k, v in state_dict_f32(build("alexnet", seed=0)).items()}


@pytest.mark.parametrize("fc8", [True, False])
@pytest.mark.parametrize("B", [1, 16, 17, 256, 512])
def test_plan(weights, B, fc8):
    steps, ops = native().plan_audit("alexnet_fp8", weights, {} if fc8 else {"fc8": False}, B, True, CUS)
    assert sum(n for _, _, n, _ in steps) == len(ops)
    names = [first for _, first, _, _ in steps]
    at = names.index("classifier.quant")
    assert names[at:] == ["classifier.quant", "classifier.1", "classifier.4", "classifier.6", "softmax_top1"]
    kernels = [k for k, _, _, _ in steps[at:]]
    fc_e4m3 = "Igemm" if not fc8 or B > 256 else "FcSmall8" if B <= 16 else "FcGemm8"
    fc_bf16 = "FcSmall" if B <= 16 else "FcGemm" if B <= 256 else "Igemm"
    assert kernels == ["QuantE4m3", fc_e4m3, fc_e4m3, fc_bf16, "SoftmaxTop1"]
    if fc_e4m3 == "FcGemm8":  # 72 / 32 K blocks of 128 over 32 column blocks: 8 slices each
        assert [d for _, _, _, d in steps[at + 1:at + 3]] == ["splits=8", "splits=8"]
    # everything before the classifier is `alexnet`'s plan
    base, base_ops = native().plan_audit("alexnet", weights, {}, B, True, CUS)
    assert steps[:at] == base[:at] and len(ops) == len(base_ops) + 1


def test_pack(weights):
    regions, total = native().pack_audit("alexnet_fp8", weights, {})
    spans = sorted((off, off + n, layer, kind) for layer, kind, off, n in regions)
    for (a0, a1, la, ka), (b0, b1, lb, kb) in zip(spans, spans[1:]):
        assert a1 <= b0, f"{la}.{ka} [{a0},{a1}) overlaps {lb}.{kb} [{b0},{b1})"
    assert spans[-1][1] <= total
    size = {(layer, kind): n for layer, kind, _, n in regions}
    assert {layer for layer, kind in size if kind == "alpha"} == {"classifier.1", "classifier.4"}
    assert size[("classifier.1", "w")] == 4096 * 9216 and size[("classifier.4", "w")] == 4096 * 4096  # 1 B a weight
    assert size[("classifier.1", "alpha")] == size[("classifier.4", "alpha")] == 4 * 4096
    assert size[("classifier.6", "w")] == 1024 * 4096 * 2  # bf16
    assert ("classifier.1", "wf") not in size and ("classifier.4", "wf") not in size  # no second copy


def test_unknown_fp8_arch_is_rejected(weights):
    """What InferenceEngine does with a name: the model zoo's check for random
    weights, the engine's own for given ones."""
    with pytest.raises(ValueError, match="unknown arch"):
        build("vgg16_fp8")
    with pytest.raises(Exception, match="unknown arch"):
        native().plan_audit("vgg16_fp8", weights, {}, 1, True, CUS)

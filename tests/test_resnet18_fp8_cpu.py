"""resnet18_fp8 / resnet34_fp8 on the host: the plan (plan_audit) and the
packed weight arena (pack_audit), no GPU.

Layers 3-4 are e4m3. From a batch that fills the CUs (4 B >= CUs) their 3x3
convs run on conv3x3_stream8: layer3.0.conv1 reads bf16 and writes e4m3 on
conv3x3_stream, its downsample is a launch of its own, every other conv1 is
the no-residual form, every conv2 the RES form, and layer4.0's conv1 and
downsample are one WIDE+DS launch. At B = 1 the same convs fall to the e4m3
implicit GEMM. The head is avgpool (from e4m3) + head_pooled at every batch.
"""
import pytest

from dmlc import native
from dmlc.models import build, state_dict_f32

CUS = 256
BLOCKS = {"resnet18_fp8": (2, 2), "resnet34_fp8": (6, 3)}  # layer3, layer4


@pytest.fixture(scope="module")
def weights():
    return {a: {k: v.detach().cpu().float().numpy() for k, v in state_dict_f32(build(a[:-4], seed=0)).items()}
            for a in BLOCKS}


@pytest.mark.parametrize("B", [256, 1])
@pytest.mark.parametrize("arch", list(BLOCKS))
def test_plan(weights, arch, B):
    steps, ops = native().plan_audit(arch, weights[arch], {}, B, True, CUS)
    assert sum(n for _, _, n, _ in steps) == len(ops)
    by = {first: (kernel, detail) for kernel, first, _, detail in steps}
    conv8 = "Stream8" if B == 256 else "Igemm"
    for li, nb in zip((3, 4), BLOCKS[arch]):
        for bi in range(nb):
            p = f"layer{li}.{bi}"
            assert by[p + ".conv2"] == (conv8, ""), (p, by[p + ".conv2"])
            if (li, bi) == (3, 0):  # the dtype boundary: bf16 in, e4m3 out
                assert by[p + ".conv1"][0] == ("Stream" if B == 256 else "Igemm")
                assert by[p + ".downsample.0"][0] in ("Conv1x1", "Igemm")
            elif bi == 0 and B == 256:  # layer4.0: one launch for conv1 and the downsample
                assert by[p + ".downsample.0"] == ("None", "")
                assert by[p + ".conv1"] == ("Stream8", f"ds={p}.downsample.0")
            elif bi == 0:
                assert by[p + ".downsample.0"][0] in ("Conv1x1", "Igemm") and by[p + ".conv1"] == ("Igemm", "")
            else:
                assert by[p + ".conv1"] == (conv8, "")
    assert by["avgpool"][0] == "AvgPoolGlobal" and by["fc"][0] == "HeadPooled"
    assert all(k not in ("Stream8", "HeadFused") for k, f, _, _ in steps if f.startswith(("layer1", "layer2")))


@pytest.mark.parametrize("arch", list(BLOCKS))
def test_pack(weights, arch):
    regions, total = native().pack_audit(arch, weights[arch], {})
    spans = sorted((off, off + n, layer, kind) for layer, kind, off, n in regions)
    for (a0, a1, la, ka), (b0, b1, lb, kb) in zip(spans, spans[1:]):
        assert a1 <= b0, f"{la}.{ka} [{a0},{a1}) overlaps {lb}.{kb} [{b0},{b1})"
    assert spans[-1][1] <= total
    size = {(layer, kind): n for layer, kind, _, n in regions}
    for li, nb in zip((3, 4), BLOCKS[arch]):
        c = 128 << (li - 2)
        for bi in range(nb):
            p = f"layer{li}.{bi}"
            cin1 = c // 2 if bi == 0 else c
            if (li, bi) != (3, 0):  # e4m3 weights, alpha, and the stream8 fragment copy (1 B a weight)
                assert size[(p + ".conv1", "wf")] == size[(p + ".conv1", "w")] == c * 9 * cin1
                assert size[(p + ".conv1", "alpha")] == 4 * c
            assert size[(p + ".conv2", "wf")] == size[(p + ".conv2", "w")] == c * 9 * c
            assert size[(p + ".conv2", "alpha")] == 4 * c
    assert size[("layer4.0.downsample.0", "wf")] == 512 * 256  # wd for the WIDE+DS launch
    assert size[("layer4.0.downsample.0", "alpha")] == 4 * 512
    assert ("layer3.0.downsample.0", "alpha") not in size  # bf16 in

"""Host-only audit of the engine's launch plan (csrc/runtime/engine_plan.cpp
Engine::plan), no GPU needed.

Which kernel runs which layer is decided by host integer logic alone, so a
predicate that silently stops matching shows up here as a changed kernel
sequence instead of as lost img/s. The sequences below were recorded from
plan_audit after the ordered kernel traces of eager forwards (same archs,
batches and option sets, on a 256-CU device) were identical before and after
run_ops became a planner and an executor.

A plan is a list of (kernel, first op, n_ops, detail); detail names what the
launch does beyond its ops: ds=OP (it also writes that downsample), dsk=OP
(it computes that downsample as extra K steps, nothing written), pool=OP (its
epilogue writes that pool), nostore (its own output is not written), wreg,
side, cfg=, strip= / mf= / splits=.
"""
import pytest

from dmlc import native
from dmlc.models import build, state_dict_f32
from test_pack_cpu import CASES as OPTION_CASES

CUS = 256
BATCHES = (1, 4, 5, 16, 64, 179, 180, 256, 257)  # 179/180, 256/257: the 70 %-of-a-round rule
R50_HEAD = ["None", "StemPoolU8", "None", "Bottleneck56Head", "Conv1x1Cat"]

# kernel names per (arch, batches), native 224x224 images, default options
NATIVE = {
    ("resnet18", (1, 4)): (
        ["None", "StemPoolU8"] + ["Small"] * 4 + ["None"] + ["Small"] * 4 + ["None"] + ["Small"] * 4 + ["None"] +
        ["Small"] * 4 + ["HeadFused"]),
    ("resnet18", (5,)): ["None", "StemPoolU8"] + ["Rows"] * 4 + ["Igemm"] * 15 + ["HeadFused"],
    ("resnet18", (16,)): (
        ["None", "StemPoolU8"] + ["Rows"] * 4 + ["Conv1x1"] + ["Igemm"] * 4 + ["Conv1x1"] + ["Igemm"] * 9 +
        ["HeadFused"]),
    ("resnet18", (64, 179, 257)): (
        ["None", "StemPoolU8"] + ["Rows"] * 4 + ["None"] + ["Stream"] * 4 + ["None"] + ["Stream"] * 4 + ["None"] +
        ["Stream"] * 4 + ["None", "HeadPooled"]),
    ("resnet18", (180, 256)): (
        ["None", "StemPoolU8"] + ["Block"] * 2 + ["None", "S2Rows"] + ["Rows28"] * 3 + ["None"] + ["Stream"] * 4 +
        ["None"] + ["Stream"] * 4 + ["None", "HeadPooled"]),
    ("resnet34", (1, 4)): (
        ["None", "StemPoolU8"] + ["Small"] * 6 + ["None"] + ["Small"] * 8 + ["None"] + ["Small"] * 12 + ["None"] +
        ["Small"] * 6 + ["HeadFused"]),
    ("resnet34", (5,)): ["None", "StemPoolU8"] + ["Rows"] * 6 + ["Igemm"] * 29 + ["HeadFused"],
    ("resnet34", (16,)): (
        ["None", "StemPoolU8"] + ["Rows"] * 6 + ["Conv1x1"] + ["Igemm"] * 8 + ["Conv1x1"] + ["Igemm"] * 19 +
        ["HeadFused"]),
    ("resnet34", (64, 179, 257)): (
        ["None", "StemPoolU8"] + ["Rows"] * 6 + ["None"] + ["Stream"] * 8 + ["None"] + ["Stream"] * 12 + ["None"] +
        ["Stream"] * 6 + ["None", "HeadPooled"]),
    ("resnet34", (180, 256)): (
        ["None", "StemPoolU8"] + ["Block"] * 3 + ["None", "S2Rows"] + ["Rows28"] * 7 + ["None"] + ["Stream"] * 12 +
        ["None"] + ["Stream"] * 6 + ["None", "HeadPooled"]),
    ("resnet50", (1,)): (
        R50_HEAD + ["Conv1x1", "Small", "Conv1x1"] * 2 +
        ["Igemm", "Conv1x1"] + ["Small", "Igemm", "Igemm"] * 4 + ["Igemm", "Small", "Igemm"] * 6 + ["Igemm"] * 5 +
        ["Small"] + ["Igemm"] * 2 + ["Small", "Igemm", "HeadFused"]),
    ("resnet50", (4,)): (
        R50_HEAD + ["Conv1x1", "Small", "Conv1x1"] * 2 +
        ["Conv1x1", "Conv1x1", "Small"] * 4 + ["Conv1x1", "Igemm", "Conv1x1"] + ["Small", "Igemm", "Igemm"] * 6 +
        ["Igemm"] * 4 + ["Small"] + ["Igemm"] * 2 + ["Small", "Igemm", "HeadFused"]),
    ("resnet50", (5,)): (
        R50_HEAD + ["Conv1x1", "Rows", "Conv1x1"] * 2 + ["Igemm", "Conv1x1"] + ["Igemm"] * 40 + ["HeadFused"]),
    ("resnet50", (16,)): (
        R50_HEAD + ["Conv1x1", "Rows", "Conv1x1"] * 2 +
        ["Conv1x1", "Conv1x1", "Igemm"] * 4 + ["Conv1x1", "Igemm"] * 3 + ["Igemm", "Conv1x1", "Igemm"] * 5 +
        ["Igemm"] * 9 + ["HeadFused"]),
    ("resnet50", (64,)): (
        R50_HEAD + ["Conv1x1", "Rows", "Conv1x1"] * 2 +
        ["Conv1x1", "Conv1x1", "Stream"] * 4 + ["Conv1x1", "Igemm"] * 3 + ["Stream", "Conv1x1", "Igemm"] * 5 +
        ["Igemm"] * 2 + ["Conv1x1", "Igemm", "Stream"] * 2 + ["Conv1x1", "AvgPoolGlobal", "HeadPooled"]),
    ("resnet50", (179,)): (
        R50_HEAD + ["Conv1x1", "Rows", "Conv1x1"] * 2 +
        ["Igemm", "Conv1x1"] + ["Stream", "Igemm", "Igemm"] * 4 + ["Igemm"] * 4 + ["Stream", "Igemm", "Igemm"] * 5 +
        ["Igemm"] * 4 + ["Stream"] + ["Igemm"] * 2 + ["Stream", "Igemm", "AvgPoolGlobal", "HeadPooled"]),
    ("resnet50", (180,)): (
        R50_HEAD + ["Conv1x1", "Rows", "Conv1x1"] * 2 +
        ["Conv1x1"] * 2 + ["S2Rows128"] + ["Conv1x1", "Conv1x1", "Rows28"] * 3 + ["Conv1x1", "Igemm"] * 2 +
        ["Igemm", "Igemm", "Stream"] * 5 + ["Igemm"] * 6 + ["Stream"] + ["Igemm"] * 2 +
        ["Stream", "Igemm", "AvgPoolGlobal", "HeadPooled"]),
    ("resnet50", (256,)): (
        R50_HEAD + ["Conv1x1", "Rows", "Conv1x1"] * 2 +
        ["Conv1x1"] * 2 + ["S2Rows128"] + ["Conv1x1", "Conv1x1", "Rows28"] * 3 + ["Conv1x1", "Igemm"] +
        ["Conv1x1", "BigTile"] * 2 + ["Stream", "Conv1x1", "BigTile"] * 4 + ["Stream", "Conv1x1"] + ["Igemm"] * 3 +
        ["Conv1x1", "Igemm", "Stream"] * 2 + ["Conv1x1", "AvgPoolGlobal", "HeadPooled"]),
    ("resnet50", (257,)): (
        R50_HEAD + ["Conv1x1", "Rows", "Conv1x1"] * 2 +
        ["Igemm", "Conv1x1"] + ["Stream", "Igemm", "Igemm"] * 4 + ["Igemm", "BigTile"] * 2 +
        ["Stream", "Igemm", "BigTile"] * 4 + ["Stream"] + ["Igemm"] * 6 + ["Stream"] + ["Igemm"] * 2 +
        ["Stream", "Igemm", "AvgPoolGlobal", "HeadPooled"]),
    ("resnet50_fp8", (1, 5)): (
        R50_HEAD + ["Bottleneck56"] * 2 + ["Igemm", "Conv1x1"] + ["Igemm"] * 40 + ["HeadFused"]),
    ("resnet50_fp8", (4,)): (
        R50_HEAD + ["Bottleneck56"] * 2 + ["Conv1x1"] * 2 +
        ["Igemm", "Conv1x1Chain"] * 3 + ["Igemm", "Conv1x1"] * 2 + ["Igemm"] * 27 + ["HeadFused"]),
    ("resnet50_fp8", (16,)): (
        R50_HEAD + ["Bottleneck56"] * 2 + ["Conv1x1"] * 2 +
        ["Igemm", "Conv1x1Chain"] * 3 + ["Igemm"] + ["Conv1x1"] * 3 + ["Igemm", "Conv1x1", "Conv1x1"] * 5 +
        ["Igemm", "Conv1x1"] * 2 + ["Igemm"] * 8 + ["HeadFused"]),
    ("resnet50_fp8", (64, 256)): (
        R50_HEAD + ["Bottleneck56"] * 2 + ["Conv1x1"] * 2 +
        ["Stream8", "Conv1x1Chain"] * 3 + ["Stream8"] + ["Conv1x1"] * 3 + ["Stream8", "Conv1x1", "Conv1x1"] * 5 +
        ["Stream8", "Conv1x1", "Igemm", "Conv1x1"] + ["Stream8", "Conv1x1", "Igemm"] * 2 +
        ["Stream8", "Conv1x1", "AvgPoolGlobal", "HeadPooled"]),
    ("resnet50_fp8", (179, 257)): (
        R50_HEAD + ["Bottleneck56"] * 2 +
        ["Igemm", "Conv1x1"] + ["Stream8", "Igemm", "Igemm"] * 4 + ["Igemm", "Stream8", "Igemm"] * 6 +
        ["Igemm", "Igemm", "Stream8"] * 3 + ["Igemm", "AvgPoolGlobal", "HeadPooled"]),
    ("resnet50_fp8", (180,)): (
        R50_HEAD + ["Bottleneck56"] * 2 + ["Conv1x1"] * 2 +
        ["Stream8", "Conv1x1Chain"] * 3 + ["Stream8", "Conv1x1", "Igemm", "Conv1x1"] +
        ["Stream8", "Igemm", "Igemm"] * 6 + ["Igemm", "Stream8", "Igemm"] * 3 + ["AvgPoolGlobal", "HeadPooled"]),
    ("alexnet", (1, 4, 5, 16)): ["AlexStem", "Direct27"] + ["Direct13"] * 3 + ["FcSmall"] * 3 + ["SoftmaxTop1"],
    ("alexnet", (64, 179, 180, 256)): ["AlexStem", "Direct27"] + ["Direct13"] * 3 + ["FcGemm"] * 3 + ["SoftmaxTop1"],
    ("alexnet", (257,)): ["AlexStem", "Direct27"] + ["Direct13"] * 3 + ["Igemm"] * 3 + ["SoftmaxTop1"],
}

# images of another size (preprocess runs), default options
RESIZED = {
    ("resnet18", 4): (
        ["Preprocess", "StemPool"] + ["Small"] * 4 + ["None"] + ["Small"] * 4 + ["None"] + ["Small"] * 4 + ["None"] +
        ["Small"] * 4 + ["HeadFused"]),
    ("resnet18", 256): (
        ["Preprocess", "StemPool"] + ["Block"] * 2 + ["None", "S2Rows"] + ["Rows28"] * 3 + ["None"] +
        ["Stream"] * 4 + ["None"] + ["Stream"] * 4 + ["None", "HeadPooled"]),
    ("alexnet", 4): ["Preprocess", "Igemm", "MaxPool", "Direct27"] + ["Direct13"] * 3 + ["FcSmall"] * 3 + ["SoftmaxTop1"],
    ("alexnet", 256): ["Preprocess", "Igemm", "MaxPool", "Direct27"] + ["Direct13"] * 3 + ["FcGemm"] * 3 + ["SoftmaxTop1"],
}

# the option sets of test_pack_cpu.py at B = 256, native; default options: NATIVE
R50_FP8_BF16_3X3 = (
    R50_HEAD + ["Bottleneck56"] * 2 + ["Conv1x1"] * 2 +
    ["S2Rows128"] + ["Conv1x1", "Conv1x1", "Rows28"] * 3 + ["Conv1x1"] * 3 + ["BigTile"] +
    ["Conv1x1", "Conv1x1", "Stream"] * 5 + ["Conv1x1", "Igemm"] * 3 +
    ["Stream", "Conv1x1", "Igemm", "Stream", "Conv1x1", "AvgPoolGlobal", "HeadPooled"])
OPTIONS = {
    ("resnet18", ("ds_into_conv2", "fused_block")): (
        ["None", "StemPoolU8"] + ["Rows"] * 4 + ["None", "S2Rows"] + ["Rows28"] * 3 + ["None"] + ["Stream"] * 4 +
        ["None"] + ["Stream"] * 4 + ["None", "HeadPooled"]),
    ("resnet50_fp8", ("fp8_3x3_in",)): R50_FP8_BF16_3X3,
    ("resnet50_fp8", ("fp8_3x3_out", "fp8_3x3_in")): R50_FP8_BF16_3X3,
    ("resnet50_fp8", ("ds_into_expand", "fused_bottleneck")): (
        ["None", "StemPoolU8"] + ["Conv1x1", "Conv1x1", "Rows"] * 3 + ["Conv1x1"] * 3 +
        ["Stream8", "Conv1x1Chain"] * 3 + ["Stream8"] + ["Conv1x1"] * 3 + ["Stream8", "Conv1x1", "Conv1x1"] * 5 +
        ["Stream8", "Conv1x1", "Igemm", "Conv1x1"] + ["Stream8", "Conv1x1", "Igemm"] * 2 +
        ["Stream8", "Conv1x1", "AvgPoolGlobal", "HeadPooled"]),
}

ALL = ([(a, {}, B, True, seq) for (a, bs), seq in NATIVE.items() for B in bs] +
       [(a, {}, B, False, seq) for (a, B), seq in RESIZED.items()] +
       [(a, o, 256, True, OPTIONS[(a, tuple(o))] if o else next(s for (x, bs), s in NATIVE.items() if x == a and 256 in bs))
        for a, o in OPTION_CASES])


def test_cases_cover_the_grid():
    assert sorted((a, B) for (a, bs) in NATIVE for B in bs) == sorted(
        (a, B) for a in ("resnet18", "resnet34", "resnet50", "resnet50_fp8", "alexnet") for B in BATCHES)
    assert {(a, tuple(o)) for a, o in OPTION_CASES if o} == set(OPTIONS)


@pytest.fixture(scope="module")
def plans():
    """plan_audit(arch, options, B, native) -> (steps, ops), each computed once."""
    C = native()
    weights, cache = {}, {}

    def get(arch, opts, B, nat):
        key = (arch, tuple(sorted(opts.items())), B, nat)
        if key not in cache:
            base = arch.replace("_fp8", "")
            if base not in weights:
                sd = state_dict_f32(build(base, seed=0))
                weights[base] = {k: v.detach().cpu().float().numpy() for k, v in sd.items()}
            cache[key] = C.plan_audit(arch, weights[base], opts, B, nat, CUS)
        return cache[key]
    return get


def _id(case):
    a, o, B, nat, _ = case
    return f"{a}-{'-'.join(o) or 'default'}-b{B}{'' if nat else '-resized'}"


def _detail(d):
    return dict(f.split("=") if "=" in f else (f, True) for f in d.split())


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_plan_kernels(plans, case):
    arch, opts, B, nat, expected = case
    steps, _ = plans(arch, opts, B, nat)
    assert [k for k, _, _, _ in steps] == expected


IMAGE = -1
READS_IMAGE = {"AlexStem", "StemPoolU8", "Preprocess"}
WRITES_EVERY_OP = {"Conv1x1Chain"}  # the expand output keeps its other reader


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_plan_structure(plans, case):
    arch, opts, B, nat, _ = case
    steps, ops = plans(arch, opts, B, nat)
    index = {name: i for i, (name, _, _, _) in enumerate(ops)}
    assert len(index) == len(ops)
    written = {IMAGE}
    unstored = set()  # activations of launches that did not store them
    nxt = 0
    for kernel, first, n, detail in steps:
        # the steps cover 0 .. len(ops) exactly once, in order
        assert index[first] == nxt and n >= 1, (kernel, first, n)
        nxt += n
        if kernel == "None":
            assert n == 1 and not detail
            continue
        covered = ops[index[first]:index[first] + n]
        d = _detail(detail)
        # what the launch reads from memory: its ops' inputs and residuals that no op of it produces
        inside, reads = set(), set()
        for _, src, out, res in covered:
            reads |= {a for a in (src, res) if a >= 0 and a not in inside}
            inside.add(out)
        if kernel in READS_IMAGE:
            reads = {IMAGE}
        if "dsk" in d:  # the downsample of the block input instead of the residual it would have written
            ds = ops[index[d["dsk"]]]
            reads = (reads - {ds[2]}) | {ds[1]}
        assert reads <= written, (kernel, first, sorted(reads - written), sorted(reads & unstored))
        # what it writes: its last op's output (every op's for a chain) and what detail names
        outs = [o[2] for o in covered] if kernel in WRITES_EVERY_OP else [covered[-1][2]]
        if "nostore" in d:
            unstored.update(outs)
            outs = []
        written.update(o for o in outs if o >= 0)
        for key in ("ds", "pool"):
            if key in d:
                written.add(ops[index[d[key]]][2])
    assert nxt == len(ops)
    assert not unstored & written


def _steps(plans, arch, B):
    steps, _ = plans(arch, {}, B, True)
    return {first: (kernel, n, _detail(detail)) for kernel, first, n, detail in steps}


def test_resnet18_b256(plans):
    s = _steps(plans, "resnet18", 256)
    assert s["layer1.0.conv1"][:2] == ("Block", 2) and s["layer1.1.conv1"][:2] == ("Block", 2)
    assert s["layer2.0.downsample.0"][0] == "None"
    assert s["layer2.0.conv1"][0] == "S2Rows" and "ds" not in s["layer2.0.conv1"][2]
    assert s["layer2.0.conv2"][0] == "Rows28" and s["layer2.0.conv2"][2]["dsk"] == "layer2.0.downsample.0"
    kernel, n, d = s["layer4.1.conv2"]
    assert kernel == "Stream" and d["pool"] == "avgpool" and "nostore" in d  # (a graph capture drops the activation)
    assert s["avgpool"][0] == "None" and s["fc"][:2] == ("HeadPooled", 2)
    assert not {"Igemm", "BigTile", "FcGemm", "AvgPoolGlobal"} & {k for k, _, _ in s.values()}


@pytest.mark.parametrize("B", [1, 4])
def test_resnet18_query_batches(plans, B):
    s = _steps(plans, "resnet18", B)
    _, ops = plans("resnet18", {}, B, True)
    convs3 = [name for name, _, _, _ in ops if ".conv" in name]
    assert len(convs3) == 16 and all(s[c][0] == "Small" for c in convs3)
    for layer in ("layer2", "layer3", "layer4"):
        assert s[f"{layer}.0.downsample.0"][0] == "None"
        assert s[f"{layer}.0.conv1"][2]["ds"] == f"{layer}.0.downsample.0"


def test_resnet50_fp8_b256(plans):
    s = _steps(plans, "resnet50_fp8", 256)
    assert s["layer1.1.conv1"][:2] == ("Bottleneck56", 3) and s["layer1.2.conv1"][:2] == ("Bottleneck56", 3)
    assert s["layer1.0.downsample.0"][0] == "None"
    assert s["layer1.0.conv1"][:2] == ("Bottleneck56Head", 2)
    assert s["layer1.0.conv3"][0] == "Conv1x1Cat" and s["layer1.0.conv3"][2]["dsk"] == "layer1.0.downsample.0"
    assert [f for f, (k, _, _) in s.items() if k == "Conv1x1Chain"] == [f"layer2.{i}.conv3" for i in range(3)]
    for layer, blocks in (("layer2", 4), ("layer3", 6), ("layer4", 3)):
        for b in range(blocks):
            assert s[f"{layer}.{b}.conv2"][0] == "Stream8", (layer, b)


def test_alexnet_b256(plans):
    steps, _ = plans("alexnet", {}, 256, True)
    assert steps[0][:3] == ("AlexStem", "preprocess", 3)
    s = _steps(plans, "alexnet", 256)
    assert s["features.3"][:2] == ("Direct27", 2) and s["features.3"][2]["pool"] == "features.5"
    assert s["features.10"][:2] == ("Direct13", 2) and s["features.10"][2]["pool"] == "features.12"

"""EngineOptions::small_alex on the host (plan_audit, no GPU): at B <= kSmallAlexMaxB AlexNet's u8 stem is
AlexStemRows and its four stride-1 convs are SmallK steps, features.3 / .10 swallowing their max-pool; elsewhere
the default plan. And conv_smallk.hip's LDS layout modelled from its formulas (test_layouts_cpu.py's method)."""
import pytest

from dmlc import native

from _golden_weights import golden_weights
from test_layouts_cpu import _b128_ways

ON = {"small_alex": True}


def plan(arch, opts, B, native_size=True, **kw):
    return native().plan_audit(arch, golden_weights(arch), opts, B, native_size, 256, **kw)


@pytest.mark.parametrize("arch", ["alexnet", "alexnet_fp8"])
@pytest.mark.parametrize("B", [1, native().kSmallAlexMaxB])
def test_small_alex_native_plan(arch, B):
    steps, ops = plan(arch, ON, B)
    by = {first: (kernel, n, detail) for kernel, first, n, detail in steps}
    assert by["features.3"] == ("SmallK", 2, "pool=features.5")
    assert by["features.10"] == ("SmallK", 2, "pool=features.12")
    for name in ("features.6", "features.8"):
        assert by[name][:2] == ("SmallK", 1) and by[name][2] in ("mf=1", "mf=2", "mf=4"), by[name]
    assert [k for k, _, _, _ in steps][:5] == ["AlexStemRows"] + ["SmallK"] * 4
    assert steps[0][1:3] == ("preprocess", 3)
    if (arch, B) == ("alexnet", 1):
        assert [k for k, _, _, _ in steps][5:] == ["FcSmall"] * 3 + ["SoftmaxTop1"]
    assert steps[5:] == plan(arch, {}, B)[0][5:]  # the classifier as without the option
    names = [o[0] for o in ops]  # every op in exactly one step
    covered = [i for _, f, n, _ in steps for i in range(names.index(f), names.index(f) + n)]
    assert sorted(covered) == list(range(len(names)))


@pytest.mark.parametrize("arch", ["alexnet", "alexnet_fp8", "resnet18"])
def test_small_alex_plan_outside_the_option(arch):
    above = native().kSmallAlexMaxB + 1
    assert plan(arch, ON, above) == plan(arch, {}, above)
    assert plan(arch, {"small_alex": False}, 1) == plan(arch, {}, 1)
    for steps in (plan(arch, {}, 1)[0], plan("resnet18", ON, 1)[0]):
        assert all(k not in ("SmallK", "AlexStemRows") for k, _, _, _ in steps)


@pytest.mark.parametrize("kw", [{}, {"tensor_in": True}], ids=["resized", "tensor"])
def test_small_alex_resized_plan(kw):
    kernels = [k for k, _, _, _ in plan("alexnet", ON, 4, False, **kw)[0]]
    assert kernels == ["PackTensor" if kw else "Preprocess", "Igemm", "MaxPool"] + ["SmallK"] * 4 + \
        ["FcSmall"] * 3 + ["SoftmaxTop1"]


def _xswz(K, cpx):
    return (K & 7) << 1 if cpx >= 16 else ((K >> 1) & 3) << 1


@pytest.mark.parametrize("KS,CI,HW,pool", [(5, 64, 27, False), (5, 64, 27, True), (3, 192, 13, False),
                                           (3, 384, 13, False), (3, 256, 13, False), (3, 256, 13, True)])
def test_conv_smallk_lds_layout(KS, CI, HW, pool):
    """The DMA's slots hold every staged chunk once; every (tile, K step, fragment) read takes, per lane, chunk
    4 kc + fq of pixel (ih, iw) from its staged place, or the zero region at the same bank slot for an outside
    tap or a dead lane; every such ds_read_b128 is bank-conflict free, border lanes included."""
    PAD, W, H, CPX, KPT = KS // 2, HW, HW, CI // 8, CI // 32
    PXC = (CPX + 15) // 16 * 16 if CPX > 8 else CPX
    PXB, FPR = PXC * 16, (W + 15) // 16
    for MF in ([3 * FPR] if pool else [1, 2, 4]):
        ZOFF = 4 * MF * 64 * 16
        ROFF = ZOFF + 256
        ntiles = (H - 3) // 2 + 1 if pool else (H * W + MF * 16 - 1) // (MF * 16)
        for tile in range(ntiles):
            p0 = tile * MF * 16
            p1 = min(p0 + MF * 16, H * W)
            r0, r1 = (2 * tile, 2 * tile + 2) if pool else (p0 // W, (p1 - 1) // W)
            ih_lo, ih_hi = max(0, r0 - PAD), min(H - 1, r1 + PAD)
            place = {}
            for s in range((ih_hi - ih_lo + 1) * W * PXC):
                K, pc = divmod(s, PXC)
                lc = pc ^ _xswz(K, CPX)
                assert 0 <= lc < PXC and (K, lc) not in place
                if lc < CPX:
                    place[(K, lc)] = ROFF + s * 16
            assert len(place) == (ih_hi - ih_lo + 1) * W * CPX
            for t in range(KS * KS * KPT):
                (kh, kw), kc = divmod(t // KPT, KS), t % KPT
                for f in range(MF):
                    addr = []
                    for lane in range(64):
                        fr, fq = lane & 15, lane >> 4
                        oh, ow = (r0 + f // FPR, 16 * (f % FPR) + fr) if pool else divmod(p0 + 16 * f + fr, W)
                        live = ow < W if pool else p0 + 16 * f + fr < p1
                        ih, iw = oh - PAD + kh, ow - PAD + kw
                        K = (oh - PAD - ih_lo) * W + ow - PAD + kh * W + kw
                        off = K * PXB + (((4 * kc + fq) ^ _xswz(K, CPX)) << 4)
                        if live and 0 <= ih < H and 0 <= iw < W:
                            a = ROFF + off
                            assert K == (ih - ih_lo) * W + iw and a == place[(K, 4 * kc + fq)], (MF, tile, t, f, lane)
                        else:
                            a = ZOFF + (off & 255)
                        addr.append(a)
                    assert _b128_ways(addr) == 1, (MF, tile, t, f)

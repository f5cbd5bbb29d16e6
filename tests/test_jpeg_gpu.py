"""The GPU half of the split JPEG decode (csrc/kernels/jpeg_finish.hip):
stage 1 (dequantise + inverse DCT) against the exact float64 transform, stage 2
(chroma upsampling + YCbCr -> RGB) bit-equal to the host decoder's colour
stage, and ops.jpeg_decode end to end against decode_jpeg and PIL."""
import io

import numpy as np
import pytest
import torch

import dmlc
from dmlc import ops
from dmlc.utils import jpeg_ref as ref

pytestmark = pytest.mark.gpu

# the standard luminance table (ITU T.81 Annex K.1), natural order: a non-trivial table
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
               14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.uint16)


def _sparse_blocks(n, rng, qt):
    """n blocks of a few low-frequency coefficients with magnitudes that fall
    with frequency, |coefficient * table| < 2^14."""
    co = np.zeros((n, 64), np.int16)
    co[:, 0] = rng.integers(-60, 60, n)
    for _ in range(6):
        pos = (rng.integers(0, 5, n) * 8 + rng.integers(0, 5, n)).astype(np.int64)
        co[np.arange(n), pos] = rng.integers(-30, 31, n)
    hi = rng.integers(0, n, n // 8)  # now and then a high-frequency term
    co[hi, rng.integers(40, 64, len(hi))] = rng.integers(-4, 5, len(hi))
    assert np.abs(co.astype(np.int64) * qt.astype(np.int64)).max() < 1 << 14
    return co


def _idct_cases():
    rng = np.random.default_rng(11)
    ones = np.ones(64, np.uint16)
    cases = {}
    dc = np.zeros((1, 64), np.int16)
    dc[0, 0] = 37
    cases["dc_only"] = (dc, K1, 1, 1)
    single = np.zeros((64, 64), np.int16)
    single[np.arange(64), np.arange(64)] = 50  # block k: only position k (row/column swaps show)
    cases["single_position"] = (single, K1, 8, 8)
    single_neg = -single
    cases["single_position_negative"] = (single_neg, (K1 * 2 + 1).astype(np.uint16), 64, 1)
    sat = np.zeros((4, 64), np.int16)
    sat[0, 0], sat[1, 0] = 1000, -1000  # +-2000 after the transform: clamps at 255 / 0
    sat[2, 0], sat[2, 1] = 900, 300
    sat[3, 0], sat[3, 8] = -900, -300
    cases["saturating"] = (sat, (ones * 16).astype(np.uint16), 2, 2)
    for bw, bh in ((3, 5), (1, 1), (63, 47)):  # partial waves, one block, many workgroups + a partial last one
        qt = (K1 * rng.integers(1, 4)).astype(np.uint16)
        cases[f"sparse_{bw}x{bh}"] = (_sparse_blocks(bw * bh, rng, qt), qt, bw, bh)
    return cases


IDCT_CASES = _idct_cases()


@pytest.mark.parametrize("name", list(IDCT_CASES))
def test_idct_against_exact_transform(gpu, name):
    co, qt, bw, bh = IDCT_CASES[name]
    got = ops.jpeg_idct(torch.from_numpy(co).to(gpu), qt, bw, bh)
    torch.cuda.synchronize()
    assert got.shape == (8 * bh, 8 * bw) and got.dtype == torch.uint8
    exact = np.clip(ref.exact_idct(co, qt, bw, bh) + 128, 0, 255)
    err = np.abs(got.cpu().numpy().astype(np.float64) - exact)
    print(f"{name}: max |u8 - exact| = {err.max():.4f}")
    # 0.5 of rounding + fp32 round-off (~30 operations at magnitudes up to 2^14, x 2^-24 < 0.03)
    assert err.max() <= 0.55


def _layout(factors, w, h):
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    return {"width": w, "height": h, "ncomp": len(factors), "hmax": hmax, "vmax": vmax,
            "comps": [{"h": fh, "v": fv, "bw": mcux * fh, "bh": mcuy * fv, "qt": np.ones(64, np.uint16)}
                      for fh, fv in factors]}


COLOUR_LAYOUTS = {"gray": [(1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)],
                  "420": [(2, 2), (1, 1), (1, 1)], "440": [(1, 2), (1, 1), (1, 1)]}
COLOUR_SIZES = [(2, 2), (7, 19), (17, 9), (33, 34), (500, 375)]


@pytest.mark.parametrize("name", list(COLOUR_LAYOUTS))
def test_colour_stage_bit_equal_to_host(gpu, name):
    nat = dmlc.native()
    rng = np.random.default_rng(5)
    for w, h in COLOUR_SIZES:
        lay = _layout(COLOUR_LAYOUTS[name], w, h)
        shapes = [(8 * c["bh"], 8 * c["bw"]) for c in lay["comps"]]
        for kind in ("random", "zeros", "full"):
            if kind == "random":
                planes = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
            else:
                planes = [np.full(s, 0 if kind == "zeros" else 255, np.uint8) for s in shapes]
            want = np.asarray(nat.ycc_planes_to_rgb(planes, lay))
            got = ops.jpeg_planes_to_rgb([torch.from_numpy(p).to(gpu) for p in planes], lay)
            torch.cuda.synchronize()
            assert tuple(got.shape) == (h, w, 3)
            assert (got.cpu().numpy() == want).all(), (name, w, h, kind)


@pytest.fixture(scope="module")
def e2e():
    """The ragged list, decoded once by each decoder."""
    from PIL import Image
    blobs = [ref.make_jpeg(w, h, s, seed=w * 7 + h) for (w, h) in COLOUR_SIZES for s in (0, 1, 2)]
    blobs.append(ref.make_jpeg(75, 41, None, seed=3))
    blobs.append(ref.make_jpeg(70, 50, 2, seed=5, restart_blocks=2))
    nat = dmlc.native()
    cpu = [np.asarray(nat.decode_jpeg(b)) for b in blobs]
    pil = [np.asarray(Image.open(io.BytesIO(b)).convert("RGB")) for b in blobs]
    got = ops.jpeg_decode(blobs, "cuda:0")
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got], cpu, pil


def test_decode_against_cpu_decoder(gpu, e2e):
    got, cpu, _ = e2e
    assert len(got) == len(cpu) == 17
    for g, c in zip(got, cpu):
        assert g.shape == c.shape and g.dtype == np.uint8
        assert np.abs(g.astype(np.int32) - c).max() <= 3, g.shape


def test_decode_against_pil(gpu, e2e):
    got, _, pil = e2e
    for g, p in zip(got, pil):
        diff = np.abs(g.astype(np.int32) - p)
        print(f"{g.shape}: mean {diff.mean():.3f} max {diff.max()}")
        assert diff.mean() < 0.6 and diff.max() <= 8, g.shape


# share of bytes that differ from the CPU decoder at all, as first measured on
# an MI355X (profiles/jpeg_gpu.txt): 0 of 1,719,933 bytes. The kernel runs the
# host's flowgraph in the host's order (columns, then rows) and both compilers
# contract the same multiply-adds, so the two fp32 transforms agree bit for bit.
MISMATCH_MEASURED = 0.0


def test_decode_mismatch_share(gpu, e2e):
    """Where an exact sample lies within fp32 error of x.5 the two fp32
    transforms (GPU; host with its own FMA contraction) may round apart."""
    got, cpu, _ = e2e
    differ = sum(int((g != c).sum()) for g, c in zip(got, cpu))
    total = sum(c.size for c in cpu)
    share = differ / total
    print(f"mismatch share: {differ} of {total} bytes = {share:.6f}")
    bound = min(3 * MISMATCH_MEASURED, 0.02)  # 3 x the measured share, never more than 2 %
    assert share <= bound


def test_unsupported_layout_falls_back_to_cpu_decoder(gpu):
    nat = dmlc.native()
    odd = ref.relabel_411(ref.make_jpeg(64, 32, 2, seed=4))
    assert not nat.jpeg_gpu_supported(nat.decode_jpeg_coeffs(odd)[0])
    plain = ref.make_jpeg(33, 34, 2, seed=8)
    got = ops.jpeg_decode([plain, odd, plain], gpu)
    torch.cuda.synchronize()
    assert (got[1].cpu().numpy() == np.asarray(nat.decode_jpeg(odd))).all()
    assert got[0].shape == (34, 33, 3) and (got[0] == got[2]).all()

"""numpy references for the split JPEG decode (tests and tools): the exact
inverse DCT of entropy-decoded coefficients, the decoder's fixed-point
YCbCr -> RGB, and small JPEG fixtures made with PIL."""
from __future__ import annotations

import io

import numpy as np

# 16.16 constants of csrc/runtime/jpeg.cpp (kCrR, kCbG, kCrG, kCbB)
CR_R, CB_G, CR_G, CB_B = 91881, -22554, -46802, 116130


def idct_matrix() -> np.ndarray:
    """C[x, u] = c(u) / 2 * cos((2x + 1) u pi / 16), c(0) = 1 / sqrt(2): the
    orthonormal 8-point inverse DCT as a matrix (float64)."""
    x = np.arange(8, dtype=np.float64)[:, None]
    u = np.arange(8, dtype=np.float64)[None, :]
    c = np.cos((2 * x + 1) * u * np.pi / 16) / 2
    c[:, 0] /= np.sqrt(2.0)
    return c


def exact_idct(coeffs: np.ndarray, qt: np.ndarray, bw: int, bh: int) -> np.ndarray:
    """Quantised coefficients [bh][bw][64] (natural order) and a table (64,
    natural order) -> the float64 samples [8 bh, 8 bw] BEFORE the level shift
    (exact separable transform)."""
    f = coeffs.astype(np.float64).reshape(bh, bw, 8, 8) * np.asarray(qt, dtype=np.float64).reshape(8, 8)
    c = idct_matrix()
    px = np.einsum("yv,abvu,xu->aybx", c, f, c)
    return px.reshape(8 * bh, 8 * bw)


def to_u8(samples: np.ndarray) -> np.ndarray:
    """+ 128, round half up, clamp."""
    return np.clip(np.floor(samples + 128.5), 0, 255).astype(np.uint8)


def exact_planes(layout: dict, coeffs: np.ndarray) -> list[np.ndarray]:
    """The u8 planes of a decode_jpeg_coeffs result through the exact IDCT."""
    out = []
    for c in layout["comps"]:
        n = c["bw"] * c["bh"] * 64
        out.append(to_u8(exact_idct(coeffs[c["offset"]:c["offset"] + n], c["qt"], c["bw"], c["bh"])))
    return out


def ycc_to_rgb(y: np.ndarray, cb: np.ndarray, cr: np.ndarray) -> np.ndarray:
    """ycc_pixel's integer formula on full-resolution u8 planes -> [H, W, 3]."""
    Y = y.astype(np.int64) << 16
    b = cb.astype(np.int64) - 128
    r = cr.astype(np.int64) - 128

    def fix(v):
        return np.clip((v + 32768) >> 16, 0, 255).astype(np.uint8)

    return np.stack([fix(Y + CR_R * r), fix(Y + CB_G * b + CR_G * r), fix(Y + CB_B * b)], -1)


def make_jpeg(w: int, h: int, subsampling: int | None, seed: int, quality: int = 90, restart_blocks: int = 0) -> bytes:
    """A w x h JPEG of smooth gradients + noise (tests/test_jpeg_cpu.py's
    image); subsampling 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0, None = grayscale;
    restart_blocks > 0 adds a restart interval of that many MCUs."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([128 + 100 * np.sin(xx / 17 + c) * np.cos(yy / 23 - c) for c in range(3)], -1)
    img = np.clip(img + rng.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    kw = {"restart_marker_blocks": restart_blocks} if restart_blocks else {}
    if subsampling is None:
        Image.fromarray(img[..., 0]).save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


def relabel_411(jpeg_420: bytes) -> bytes:
    """A 4:2:0 JPEG with its luma sampling factors rewritten from 2x2 to 4x1:
    the same four luma blocks per MCU, so the entropy-coded data still
    decodes (to a scrambled picture), but chroma is now subsampled by 4
    horizontally, a layout only the generic CPU path converts. The size must
    keep the MCU count: width a multiple of 32, height of 16."""
    i = jpeg_420.index(b"\xff\xc0")
    assert jpeg_420[i + 9] == 3 and jpeg_420[i + 11] == 0x22, "not a 4:2:0 baseline JPEG"
    return jpeg_420[:i + 11] + b"\x41" + jpeg_420[i + 12:]

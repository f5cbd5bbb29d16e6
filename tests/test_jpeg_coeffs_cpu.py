"""decode_jpeg_coeffs (csrc/runtime/jpeg.cpp): the host half of the split JPEG
decode stops after entropy decoding and returns a layout plus quantised int16
coefficients. Reconstructing pixels from them with an exact float64 inverse
DCT must land on decode_jpeg's output up to the float AAN transform's
rounding, which pins zig-zag order, block order, tables, DC prediction and
restart handling."""
import numpy as np
import pytest

import dmlc
from dmlc.utils import jpeg_ref as ref

pytest.importorskip("PIL.Image")

SIZES = [(500, 375), (17, 9), (33, 34), (224, 224), (7, 19), (2, 2)]


def _decode(data):
    nat = dmlc.native()
    lay, co = nat.decode_jpeg_coeffs(data)
    return lay, np.asarray(co), np.asarray(nat.decode_jpeg(data)).astype(np.int32)


def _check_gray(data, w, h):
    lay, co, rgb = _decode(data)
    assert co.dtype == np.int16 and co.shape == (lay["comps"][0]["bw"] * lay["comps"][0]["bh"] * 64,)
    assert (lay["width"], lay["height"], lay["ncomp"], lay["hmax"], lay["vmax"]) == (w, h, 1, 1, 1)
    assert rgb.shape == (h, w, 3)
    assert (rgb[..., 0] == rgb[..., 1]).all() and (rgb[..., 0] == rgb[..., 2]).all()
    plane = ref.exact_planes(lay, co)[0][:h, :w].astype(np.int32)
    # the float AAN transform may land on the other side of a rounding boundary, nothing more
    assert np.abs(plane - rgb[..., 0]).max() <= 1


@pytest.mark.parametrize("w,h", SIZES)
def test_grayscale_reconstruction(w, h):
    _check_gray(ref.make_jpeg(w, h, None, seed=w * 7 + h), w, h)


def test_grayscale_reconstruction_with_restart_markers():
    data = ref.make_jpeg(75, 41, None, seed=3, restart_blocks=3)
    assert b"\xff\xdd" in data and b"\xff\xd1" in data
    _check_gray(data, 75, 41)


def test_colour_restart_markers_interleaved():
    """Restart intervals in an interleaved 4:2:0 scan: the same image encoded
    with and without them quantises to the same coefficients, so predictor
    resets and block placement after a marker must reproduce them exactly."""
    nat = dmlc.native()
    a_lay, a = nat.decode_jpeg_coeffs(ref.make_jpeg(70, 50, 2, seed=5))
    b_lay, b = nat.decode_jpeg_coeffs(ref.make_jpeg(70, 50, 2, seed=5, restart_blocks=2))
    assert [(c["bw"], c["bh"], c["offset"]) for c in a_lay["comps"]] == \
        [(c["bw"], c["bh"], c["offset"]) for c in b_lay["comps"]]
    assert (np.asarray(a) == np.asarray(b)).all()  # same image, same tables: same coefficients


@pytest.mark.parametrize("w,h", SIZES)
def test_colour_444_reconstruction(w, h):
    lay, co, rgb = _decode(ref.make_jpeg(w, h, 0, seed=w * 7 + h))
    assert lay["ncomp"] == 3 and all(c["h"] == 1 and c["v"] == 1 for c in lay["comps"])
    y, cb, cr = (p[:h, :w] for p in ref.exact_planes(lay, co))
    got = ref.ycc_to_rgb(y, cb, cr).astype(np.int32)
    # each plane sample may differ by 1; the largest gain is 1 + 1.772 (blue) before one rounding
    assert np.abs(got - rgb).max() <= 3


@pytest.mark.parametrize("w,h", [(17, 9), (33, 34), (7, 19), (2, 2), (500, 375)])
@pytest.mark.parametrize("subsampling,hv", [(0, (1, 1)), (1, (2, 1)), (2, (2, 2))])
def test_block_counts_and_sampling_factors(w, h, subsampling, hv):
    lay, co = dmlc.native().decode_jpeg_coeffs(ref.make_jpeg(w, h, subsampling, seed=1))
    hmax, vmax = hv
    assert (lay["hmax"], lay["vmax"]) == hv
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    want = [hv, (1, 1), (1, 1)]
    off = 0
    for c, (ch, cv) in zip(lay["comps"], want):
        assert (c["h"], c["v"]) == (ch, cv)
        assert (c["bw"], c["bh"]) == (mcux * ch, mcuy * cv)
        assert c["offset"] == off
        assert np.asarray(c["qt"]).dtype == np.uint16 and np.asarray(c["qt"]).shape == (64,)
        off += c["bw"] * c["bh"] * 64
    assert len(co) == off


def _layout(factors, w=40, h=24):
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    return {"width": w, "height": h, "ncomp": len(factors), "hmax": hmax, "vmax": vmax,
            "comps": [{"h": fh, "v": fv, "bw": mcux * fh, "bh": mcuy * fv, "qt": np.ones(64, np.uint16)}
                      for fh, fv in factors]}


@pytest.mark.parametrize("factors,ok", [
    ([(1, 1)], True),                            # grayscale
    ([(1, 1), (1, 1), (1, 1)], True),            # 4:4:4
    ([(2, 1), (1, 1), (1, 1)], True),            # 4:2:2
    ([(2, 2), (1, 1), (1, 1)], True),            # 4:2:0
    ([(1, 2), (1, 1), (1, 1)], True),            # 4:4:0
    ([(4, 2), (2, 1), (2, 2)], True),            # factors of 2 and 1 against a 4x2 luma
    ([(3, 1), (1, 1), (1, 1)], False),           # chroma subsampled by 3
    ([(4, 1), (1, 1), (1, 1)], False),           # 4:1:1
    ([(1, 4), (1, 1), (1, 1)], False),
    ([(2, 2), (1, 1), (1, 3)], False),           # vmax 3: luma not at full resolution
    ([(1, 1), (2, 1), (2, 1)], False),           # subsampled luma
    ([(1, 1), (1, 2), (1, 1)], False),
])
def test_jpeg_gpu_supported(factors, ok):
    assert dmlc.native().jpeg_gpu_supported(_layout(factors)) is ok


def test_host_colour_stage_matches_decoder_on_444():
    """ycc_planes_to_rgb on exact planes = the numpy formula (4:4:4 needs no upsampling)."""
    nat = dmlc.native()
    lay, co = nat.decode_jpeg_coeffs(ref.make_jpeg(33, 34, 0, seed=2))
    planes = ref.exact_planes(lay, np.asarray(co))
    got = np.asarray(nat.ycc_planes_to_rgb(planes, lay))
    assert (got == ref.ycc_to_rgb(*(p[:34, :33] for p in planes))).all()
    with pytest.raises(Exception):
        nat.ycc_planes_to_rgb(planes[:2], lay)


def test_unsupported_layout_still_entropy_decodes():
    data = ref.relabel_411(ref.make_jpeg(64, 32, 2, seed=4))
    nat = dmlc.native()
    lay, co = nat.decode_jpeg_coeffs(data)
    assert (lay["hmax"], lay["vmax"]) == (4, 1) and not nat.jpeg_gpu_supported(lay)
    assert np.asarray(nat.decode_jpeg(data)).shape == (32, 64, 3)


def _error(fn, data):
    try:
        fn(data)
    except Exception as e:  # noqa: BLE001
        return type(e), str(e)
    return None


def test_errors_match_decode_jpeg():
    nat = dmlc.native()
    from PIL import Image
    import io
    good = ref.make_jpeg(64, 48, 2, seed=6)
    buf = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(buf, "JPEG", progressive=True)
    sos = good.index(b"\xff\xda")
    cases = [good[:3], good[:sos], good[:sos + 6], b"not a jpeg", buf.getvalue(),
             good[:good.index(b"\xff\xc4") + 10]]
    for data in cases:
        a, b = _error(nat.decode_jpeg, data), _error(nat.decode_jpeg_coeffs, data)
        assert a is not None and a == b, (a, b)
    assert "progressive" in _error(nat.decode_jpeg_coeffs, buf.getvalue())[1]


def test_launchers_reject_bad_descriptors():
    """The kernel launchers check every geometry on the host against the
    buffer sizes and throw before anything is launched."""
    nat = dmlc.native()
    lay = _layout([(2, 2), (1, 1), (1, 1)], 33, 34)
    descs, tables, ncoef, pbytes = nat.jpeg_gpu_plan([lay], [4096])
    assert tables.shape == (3, 64) and ncoef == pbytes == sum(c["bw"] * c["bh"] * 64 for c in lay["comps"])
    ok = dict(descs=descs, dev=4096, qf=4096, n_tables=3, coef=4096, coef_elems=ncoef, planes=4096,
              plane_bytes=pbytes, stream=0)
    for bad in (dict(coef_elems=ncoef - 1), dict(plane_bytes=pbytes - 1), dict(n_tables=2), dict(coef=4098),
                dict(planes=4097), dict(qf=0)):
        with pytest.raises(ValueError):
            nat.jpeg_idct_planes(**{**ok, **bad})
    with pytest.raises(ValueError):
        nat.jpeg_planes_to_rgb(descs, 4096, 4096, pbytes - 1, 0)
    misaligned = nat.jpeg_gpu_plan([lay], [4097])[0]
    with pytest.raises(ValueError):
        nat.jpeg_planes_to_rgb(misaligned, 4096, 4096, pbytes, 0)
    with pytest.raises(ValueError):  # a layout the kernels do not handle never gets a descriptor
        nat.jpeg_gpu_plan([_layout([(4, 1), (1, 1), (1, 1)], 33, 34)], [4096])

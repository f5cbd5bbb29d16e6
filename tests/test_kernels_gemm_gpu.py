"""Op-level tests of the general matrix family, which the other op tests use
as their yardstick and which test_kernels_gpu.py / test_fp8_gpu.py judge by a
relative-L2 norm alone: conv_igemm.hip (11 tiles, split-K with
splitk_reduce, persistent grids, the packed-RGB stem, six e4m3
instantiations), conv_bigtile.hip (256x256 / 256x128 tiles with split-K slabs,
the persistent form) and fc_gemm.hip.

As in test_kernels_resnet50_gpu.py every output is compared element-wise with
a float64 reference on the same (bf16 / e4m3) operands under the derived bar
of tests/_kernel_bar.py (threshold 1.0; K = KH KW Cin, 3 KH KW for the stem,
whatever the slicing: split-K is still a sum of K exact products in fp32 in
some order), keeps the project's relative-L2 bar (5e-3 bf16 / fp32, 0.04
e4m3) and carries negative controls: a reference with one modelled fault
(kb.gemm_controls, kb.fc_controls: chunk swap at the last pixel, batch shift,
the partial last M tile taking the previous tile's rows, a K tile missing, a
split-K slice missing, pad columns spilling into the next row) must be
rejected. Every output is pre-filled with NaN. The cases live in
_kernel_bar.py (IGEMM_CASES, E4M3_CASES, BIGTILE_CASES, FC_*), where
test_kernel_bar_cpu.py checks the bar and every control on the same operands
without a GPU.

Every code path also has an exact case: small integer operands for which
every fp32 partial sum is exact (kb.gemm_operands(exact=True)), so the output
must equal the float64 result bit for bit whatever the tile, slice count or
hand-off order; e4m3 outputs compare bytes, ties and the saturation at 448
included.

What the shapes are for is said at each test. Not covered: a row stride
ldo > N, which the Python wrappers do not express.

Recorded on an MI355X (worst |err| / bar over a kernel's cases; its weakest
control ratio and which control), not thresholds:
  conv_igemm bf16, tiles 0..10      0.94 (Cout 100, tile 0)   176 (K tile missing, 5x5)
  conv_igemm split-K                0.44; fp32 output < 0.01   25 (K tile missing, 2 slices, tile 3)
  conv_igemm persistent             0.77                      114 (K tile missing, tile 8)
  conv_igemm stem                   0.97 (7x7 / s2)          4968 (chunk swap, 11x11 / s4)
  conv_igemm e4m3 in / e4m3 out     0.91 (256x64; persistent 0.91)   96 (K tile missing, 128x128)
  conv_igemm bf16 in / e4m3 out     0.94 (128x128)           6127 (K tile missing, 128x128)
  conv_igemm e4m3 in / bf16 out     0.59 (256x64)             102 (K tile missing, 128x128)
  conv_bigtile cfg 0 / 1, slabs     0.82 (cfg 0, 1 slice)     115 (K tile missing, stride 2)
  conv_bigtile persistent           0.81 (28x28, grid 1)      149 (K tile missing, 13x13, grid 1)
  fc_gemm bf16 / fp32               0.90 (K = 512) / < 0.01   154 (stale ring slot, M = 1, N = 1000)
Largest relative L2 1.7e-3 (bf16 outputs), 1.9e-7 (fp32), 2.7e-2 (e4m3). All
28 exact cases: 0 values differ. The split-K ratios are small because K =
4608 makes the summation term the larger part of the bar; a single missing K
tile (64 of 4608 products) is still 25 bars away. An fp32 output has no
rounding term, so a correct kernel sits far below its bar (K 2^-23 mag against
an error of a few 2^-24 mag); its exact cases carry the weight there.
"""
import pytest
import torch

import dmlc
from dmlc import ops

import _kernel_bar as kb

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn


def _nan(shape, gpu, dtype):
    if dtype == FP8:
        return torch.full(shape, 0x7F, dtype=torch.uint8, device=gpu).view(FP8)
    return torch.full(shape, float("nan"), dtype=dtype, device=gpu)


def _dev(t_nchw, gpu, e4m3):
    """NCHW float64 (bf16 values or e4m3 codes) -> NHWC on the device (exact)."""
    t = kb.nhwc(t_nchw).float()
    return (t.to(FP8) if e4m3 else t.bfloat16()).to(gpu)


def _pack8(o, gpu):
    """e4m3 weight codes [Cout, Cin, k, k] -> packed [Npad, K], k = (kh KW + kw) Cin + c."""
    w = o["w"]
    wk = torch.zeros(kb.npad(w.shape[0]), o["K"])
    wk[:w.shape[0]] = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).float()
    return wk.to(FP8).to(gpu)


def _out_shape(o):
    B, N, Ho, Wo = o["ref"][0].shape
    return (B, Ho, Wo, N)


def _launch(o, gpu, tile, split_k=1, max_blocks=0, out_f32=False):
    """One bf16 conv2d launch (conv_igemm or conv_bigtile by `tile`) on a
    NaN-filled output: the output, NHWC on the device."""
    k, s, p = o["k"], o["stride"], o["pad"]
    y = _nan(_out_shape(o), gpu, torch.float32 if out_f32 else torch.bfloat16)
    res = None if o["r"] is None else _dev(o["r"], gpu, False)
    bias = o["bias"].float().to(gpu)
    if o["stem"]:
        Ho, Wo = y.shape[1:3]
        H, W = o["x"].shape[2:]
        need = ((Wo - 1) * s * 3 + (3 * k + 7) // 8 * 8 + 2) // 3
        xp = ops.stem_image(kb.nhwc(o["x"]).float(), p, (max(W + 2 * p, need) + 7) // 8 * 8).bfloat16().to(gpu)
        wp = ops.pack_conv_weight(o["w"].float(), stem=True, device=gpu)
        out = ops.conv2d(xp, wp, o["N"], k, k, s, p, bias=bias, relu=True, stem=True, out_hw=(Ho, Wo), tile=tile, out=y)
    else:
        wp = ops.pack_conv_weight(o["w"].float(), device=gpu)
        out = ops.conv2d(_dev(o["x"], gpu, False), wp, o["N"], k, k, s, p, bias=bias, res=res, relu=True,
                         out_f32=out_f32, split_k=split_k, tile=tile, out=y, max_blocks=max_blocks)
    assert out.data_ptr() == y.data_ptr()
    torch.cuda.synchronize()
    return y


def _launch8(o, gpu, tile, max_blocks=0):
    """One conv2d_fp8 launch on a NaN-filled output."""
    in8, out8 = o["in8"], o["out8"]
    y = _nan(_out_shape(o), gpu, FP8 if out8 else torch.bfloat16)
    w = _pack8(o, gpu) if in8 else ops.pack_conv_weight(o["w"].float(), device=gpu)
    res = None if o["r"] is None else _dev(o["r"], gpu, out8)
    ops.conv2d_fp8(_dev(o["x"], gpu, in8), w, None if o["alpha"] is None else o["alpha"].float().to(gpu), o["N"],
                   o["k"], o["k"], o["stride"], o["pad"], bias=o["bias"].float().to(gpu), res=res,
                   res_scale=o["res_scale"], relu=True, out_scale=o["out_scale"], tile=tile, out=y,
                   max_blocks=max_blocks)
    torch.cuda.synchronize()
    return y


def _check(o, y, what, controls, out_f32=False):
    """The bar, the L2 bar and the controls on one NHWC output."""
    v, mag = o["ref"]
    want, bnd, l2 = kb.gemm_bar(o, v, mag, out_f32)
    got = kb.nchw(y.cpu().double())
    kb.assert_close(got, want, bnd, what, l2=l2)
    assert len(controls) >= 2, what
    for name, wrong in controls:
        kb.assert_rejects(got, kb.gemm_bar(o, wrong, mag, out_f32)[0], bnd, f"{what} [{name}]")


def _check_exact(o, y, what):
    v = o["ref"][0]
    if o["out8"]:
        want = kb.e4m3_bytes(v * kb.f32(1.0 / o["out_scale"]))
        got = kb.nchw(y.cpu().view(torch.uint8))
        assert int((want == 0x7E).sum()) > 0 and int((want == 0).sum()) > 0  # saturated values and ReLU zeros
    else:
        want, got = torch.relu(v), kb.nchw(y.cpu().double())
        assert float(want.max()) <= 256
    bad = int((got != want).sum())
    print(f"{what} exact: {bad} of {want.numel()} values differ")
    assert torch.equal(got, want), f"{what}: {bad} values differ, first at {(got != want).nonzero()[:4].tolist()}"


# ---------------------------------------------------------------- conv_igemm, bf16
@pytest.mark.parametrize("case", kb.IGEMM_CASES, ids=[c[0] for c in kb.IGEMM_CASES])
def test_conv_igemm(gpu, case):
    """base: 3x13x13x64, 3x3 / p1, with a residual, at every tile: M = 507 is
    no multiple of 64, 128 or 256, 9 K tiles outlast every ring depth, every
    border has padding taps; 256 channels give >= 2 N tiles (512 for BN = 256).
    Tiles 7..10 take the register epilogue (wave tiles narrower than 64).
    stride 2, 5x5 (Npad = 192: tile 1), 1x1 with 8 K tiles.
    Cout 100: N % 8 != 0 and N < Npad = 128: the register epilogue's column
    guard, rows of 200 B.
    split-K: 1x7x7x512 -> 512, 72 K tiles, tiles 3 and 5 (the engine's small-M
    plan); the launcher gives each slice ceil(72 / split_k) K tiles, so 5
    leaves an uneven last slice, 13 runs 12 slices (the reduce's 8- and 4-wide
    loops), 15 runs 15 (8 + 4 + 3: all three loops, a last slice of 2), 32
    runs 24; one run with fp32 output.
    persistent: 5x13x13x192 -> 384 with a residual on 8 blocks, every block
    walking several tiles across tile boundaries (tile 2 at 512 channels)."""
    name, shape, res, tile, split_k, max_blocks, out_f32 = case
    o = kb.gemm_case_operands(shape, res, kb.case_seed(kb.IGEMM_CASES, name))
    bm, bn = kb.GEMM_TILES[tile]
    slices = kb.igemm_slices(o["K"] // 64, split_k)
    y = _launch(o, gpu, tile, split_k, max_blocks, out_f32)
    _check(o, y, f"conv_igemm {name}", kb.gemm_controls(o, bm, bn, slices), out_f32)


@pytest.mark.parametrize("case", kb.IGEMM_EXACT, ids=[c[0] for c in kb.IGEMM_EXACT])
def test_conv_igemm_exact(gpu, case):
    """Every tile at the base shape, the split-K reduce at 12 and 15 slices
    and the persistent walk on integer operands: bit-equal to float64."""
    name, shape, res, tile, split_k, max_blocks, out_f32 = case
    o = kb.gemm_case_operands(shape, res, kb.case_seed(kb.IGEMM_CASES, name), exact=True)
    _check_exact(o, _launch(o, gpu, tile, split_k, max_blocks, out_f32), f"conv_igemm {name}")


@pytest.mark.parametrize("k,s,p", kb.STEM_CASES)
def test_conv_igemm_stem(gpu, k, s, p):
    """The packed-RGB stem (K = 3 k k products per output, the register
    epilogue, 256x64 tiles) at 2x57x61: odd sizes, several M tiles and a tail."""
    o = kb.gemm_operands(2, *kb.STEM_HW, 3, 64, k, s, p, seed=490 + k)
    _check(o, _launch(o, gpu, -1), f"conv_igemm stem {k}x{k}/s{s}", kb.gemm_controls(o, 256, 64))


def test_conv_igemm_stem_exact(gpu):
    o = kb.gemm_operands(2, *kb.STEM_HW, 3, 64, 7, 2, 3, seed=497, exact=True)
    _check_exact(o, _launch(o, gpu, -1), "conv_igemm stem 7x7/s2")


# ---------------------------------------------------------------- conv_igemm, e4m3
@pytest.mark.parametrize("case", kb.E4M3_CASES, ids=[c[0] for c in kb.E4M3_CASES])
def test_conv_igemm_e4m3(gpu, case):
    """The six e4m3 instantiations by dtype pair and tile (128x128; 256x64
    through Npad = 192 and tile = 1) at 2x14x14 (M = 392: two M tiles and a
    tail): e4m3 in / out with an e4m3 residual on the e4m3 bar, bf16 in / e4m3
    out (1x1, K = 64), e4m3 in / bf16 out on the bf16 bar with alpha in mag.
    persistent: e4m3 in / out at 5x13x13x256 -> 384 on 8 blocks, as the bf16
    persistent case (the LDS epilogue runs while the next tile's DMA lands)."""
    name, shape, in8, out8, res, tile = case[:6]
    o = kb.gemm_case_operands(shape, res, kb.case_seed(kb.E4M3_CASES, name), in8=in8, out8=out8)
    bm, bn = (256, 64) if tile == 1 else (128, 128)
    _check(o, _launch8(o, gpu, tile, *case[6:]), f"conv_igemm {name}", kb.gemm_controls(o, bm, bn))


@pytest.mark.parametrize("case", kb.E4M3_CASES, ids=[c[0] for c in kb.E4M3_CASES])
def test_conv_igemm_e4m3_exact(gpu, case):
    """Integer codes, alpha in {1, 2, 4}, res_scale 4, out_scale 2: the output
    bytes (bf16 values) equal the float64 result's."""
    name, shape, in8, out8, res, tile = case[:6]
    o = kb.gemm_case_operands(shape, res, kb.case_seed(kb.E4M3_CASES, name), exact=True, in8=in8, out8=out8)
    _check_exact(o, _launch8(o, gpu, tile, *case[6:]), f"conv_igemm {name}")


# ---------------------------------------------------------------- conv_bigtile
def _launch_bigtile(o, gpu, tile, n, what):
    """tile 11 / 12 with n K slices (twice: no hand-off time-out, the flags
    left clean, the same bits again), tile 13 on a grid of n workgroups."""
    if tile == 13:
        return _launch(o, gpu, tile, max_blocks=n)
    y = _launch(o, gpu, tile, split_k=n)
    assert not ops.bigtile_error(gpu), f"{what}: split-K hand-off timed out"
    y2 = _launch(o, gpu, tile, split_k=n)
    assert not ops.bigtile_error(gpu), f"{what}: split-K hand-off timed out"
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), f"{what}: a second launch differs in bits"
    return y


@pytest.mark.parametrize("case", kb.BIGTILE_CASES, ids=[c[0] for c in kb.BIGTILE_CASES])
def test_conv_bigtile(gpu, case):
    """cfg 0 (256x256) at 2x13x13x128 -> 512: M = 338 is two M tiles with a
    tail of 82 rows, two N tiles, 18 K tiles in 1, 2 and 5 (uneven) slices;
    cfg 1 (256x128) on the same input -> 128; stride 2 at 4x14x14x256 -> 512;
    the persistent form on 1 and 3 workgroups (10 tiles of one N tile; 4 M
    tiles x 3 N tiles with a tail), every workgroup walking several tiles."""
    name, shape, res, tile, n = case
    o = kb.gemm_case_operands(shape, res, kb.case_seed(kb.BIGTILE_CASES, name))
    bm, bn = kb.GEMM_TILES[tile]
    slices = kb.bigtile_slices(o["K"] // 64, n) if tile != 13 else None
    what = f"conv_bigtile {name}"
    _check(o, _launch_bigtile(o, gpu, tile, n, what), what, kb.gemm_controls(o, bm, bn, slices))


@pytest.mark.parametrize("case", kb.BIGTILE_EXACT, ids=[c[0] for c in kb.BIGTILE_EXACT])
def test_conv_bigtile_exact(gpu, case):
    """cfg 0 at 5 slices, cfg 1 at 2 and the persistent form on one workgroup,
    integer operands: bit-equal to float64 whatever the hand-off order."""
    name, shape, res, tile, n = case
    o = kb.gemm_case_operands(shape, res, kb.case_seed(kb.BIGTILE_CASES, name), exact=True)
    what = f"conv_bigtile {name}"
    _check_exact(o, _launch_bigtile(o, gpu, tile, n, what), what)


# ---------------------------------------------------------------- fc_gemm
GUARD = 16
SENTINEL = -12345.0  # a bf16 value


def _launch_fc(o, gpu, splits, out_f32, relu):
    """ops.fc into the first M rows of a sentinel-filled [M + 16, N] tensor."""
    M, N = o["ref"][0].shape
    wp = ops.pack_conv_weight(o["w"].float().view(N, o["K"], 1, 1), device=gpu)
    assert wp.shape == (kb.npad(N), o["K"]) and wp.shape[0] % kb.FC_BN == 0
    y = torch.full((M + GUARD, N), SENTINEL, dtype=torch.float32 if out_f32 else torch.bfloat16, device=gpu)
    y[:M] = float("nan")
    out = ops.fc(o["x"].float().bfloat16().to(gpu), wp, N, bias=o["bias"].float().to(gpu), relu=relu, out_f32=out_f32,
                 splits=splits, out=y[:M])
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    assert bool((y[M:] == SENTINEL).all()), "fc_gemm wrote past row M (the zero-page rows)"
    return y[:M].cpu().double()


@pytest.mark.parametrize("N", kb.FC_NS)
@pytest.mark.parametrize("M", kb.FC_MS)
def test_fc_gemm(gpu, M, N):
    """M = 1 (one row), 17 (no multiple of 16), 200 (a ragged last row group),
    256 (full); K = 1024: 16 K blocks through the 3-slot ring in 1, 2, 4 slices
    and the engine's pick; N = 1000 leaves 24 pad columns in the last
    128-column group. bf16 output with ReLU and fp32 output without. The rows
    past M, read from the zero page, must not reach y: 16 guard rows keep
    their sentinel."""
    o = kb.fc_operands(M, kb.FC_K, N, seed=600 + M + N)
    v, mag = o["ref"]
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    for splits in (1, 2, 4, 0):
        used = splits or dmlc.native().fc_gemm_splits(M, kb.FC_K, kb.npad(N), cus)
        controls = kb.fc_controls(o, used)
        for out_f32 in (False, True):
            relu = not out_f32
            f = torch.relu if relu else (lambda t: t)
            what = f"fc_gemm M={M} N={N} splits={splits} ({used}) {'fp32' if out_f32 else 'bf16'}"
            got = _launch_fc(o, gpu, splits, out_f32, relu)
            bnd = kb.bound(f(v), mag, kb.FC_K, out_bf16=not out_f32)
            kb.assert_close(got, f(v), bnd, what)
            for name, wrong in controls:
                kb.assert_rejects(got, f(wrong), bnd, f"{what} [{name}]")


def test_fc_gemm_min_slice(gpu):
    """K = 512 in 2 slices: 4 K blocks a slice, the documented minimum (the
    ring wraps once)."""
    o = kb.fc_operands(200, 512, 1000, seed=650)
    v, mag = o["ref"]
    got = _launch_fc(o, gpu, 2, False, True)
    bnd = kb.bound(torch.relu(v), mag, 512)
    kb.assert_close(got, torch.relu(v), bnd, "fc_gemm K=512 splits=2")
    for name, wrong in kb.fc_controls(o, 2):
        kb.assert_rejects(got, torch.relu(wrong), bnd, f"fc_gemm K=512 splits=2 [{name}]")


@pytest.mark.parametrize("out_f32", [False, True])
def test_fc_gemm_exact(gpu, out_f32):
    o = kb.fc_operands(17, kb.FC_K, 1000, seed=660, exact=True)
    want = o["ref"][0] if out_f32 else torch.relu(o["ref"][0])
    assert float(want.abs().max()) <= 256
    got = _launch_fc(o, gpu, 4, out_f32, not out_f32)
    bad = int((got != want).sum())
    print(f"fc_gemm exact: {bad} of {want.numel()} values differ")
    assert torch.equal(got, want), f"{bad} values differ, first at {(got != want).nonzero()[:4].tolist()}"


# ---------------------------------------------------------------- host-side argument checks
def _args(gpu, Cin=64, N=64, k=1, hw=8, B=1, **over):
    """Raw arguments of a small valid launch (kept alive in the dict's "_keep")."""
    C = dmlc.native()
    pad = k // 2
    keep = {"x": torch.zeros(B, hw, hw, Cin, dtype=torch.bfloat16, device=gpu),
            "w": torch.zeros(kb.npad(N), C.conv_kpad(Cin, k, k), dtype=torch.bfloat16, device=gpu),
            "y": _nan((B, hw, hw, N), gpu, torch.bfloat16)}
    a = dict(x=keep["x"].data_ptr(), w=keep["w"].data_ptr(), bias=0, res=0, y=keep["y"].data_ptr(), B=B, H=hw, W=hw,
             Cin=Cin, KH=k, KW=k, stride=1, pad=pad, N=N, Npad=kb.npad(N), Kpad=keep["w"].shape[1], ldo=N, relu=False,
             out_f32=False, split_k=1, ws=0, tile=-1, zero=ops._zero_page(gpu).data_ptr(), stem=False, Ho=hw, Wo=hw,
             max_blocks=0, stream=torch.cuda.current_stream().cuda_stream)
    a.update(over)
    return a, keep


def _rejected(C, a, keep, what):
    with pytest.raises(ValueError):
        C.conv2d(**a)
    torch.cuda.synchronize()
    assert bool(torch.isnan(keep["y"]).all()), f"{what}: something was launched"


def test_conv_igemm_rejects(gpu):
    """Bad Kpad, N % 4 != 0, fp8 with split-K, a misaligned x, split-K without
    a workspace: each raises and launches nothing; the same launch without
    the fault runs."""
    C = dmlc.native()
    a, keep = _args(gpu)
    C.conv2d(**a)
    torch.cuda.synchronize()
    assert bool((keep["y"] == 0).all())
    ws = torch.zeros(2 * 64 * 64, dtype=torch.float32, device=gpu)
    for what, over in [("bad Kpad", dict(Kpad=128)), ("N % 4", dict(N=62, ldo=62)),
                       ("fp8 with split-K", dict(out_fp8=True, split_k=2, ws=ws.data_ptr())),
                       ("misaligned x", {}), ("split-K without a workspace", dict(split_k=2))]:
        b, keep = _args(gpu, **over)
        if what == "misaligned x":
            b["x"] = keep["x"].data_ptr() + 2
        _rejected(C, b, keep, what)


def test_conv_bigtile_rejects(gpu):
    """splits > K tiles, a workspace that is too small, N % 8 != 0."""
    C = dmlc.native()
    ws = ops._bigtile_ws(gpu, C.conv_bigtile_ws_bytes(4))
    base = dict(Cin=128, N=256, k=3, tile=C.CONV_BIGTILE0, bt_ws=ws.data_ptr(), bt_ws_bytes=ws.numel(), bt_splits=2)
    a, keep = _args(gpu, **base)
    C.conv2d(**a)
    torch.cuda.synchronize()
    assert bool((keep["y"] == 0).all()) and not ops.bigtile_error(gpu)
    for what, over in [("splits > K tiles", dict(bt_splits=19)),
                       ("workspace too small", dict(bt_ws_bytes=C.conv_bigtile_ws_bytes(0))),
                       ("N % 8", dict(N=252, ldo=252))]:
        b, keep = _args(gpu, **{**base, **over})
        _rejected(C, b, keep, what)


def test_fc_gemm_rejects(gpu):
    """A residual, K blocks % splits != 0, B > 256."""
    C = dmlc.native()
    ws = torch.zeros(4 * 257 * 128, dtype=torch.float32, device=gpu)
    base = dict(Cin=1024, N=128, hw=1, B=8, tile=C.CONV_FC, split_k=2, ws=ws.data_ptr())
    a, keep = _args(gpu, **base)
    C.conv2d(**a)
    torch.cuda.synchronize()
    assert bool((keep["y"] == 0).all())
    for what, over in [("a residual", dict(res=ws.data_ptr())), ("K blocks % splits", dict(split_k=3)),
                       ("B > 256", dict(B=257))]:
        b, keep = _args(gpu, **{**base, **over})
        _rejected(C, b, keep, what)

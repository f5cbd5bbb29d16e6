"""Python entry points to the hand-written gfx950 HIP kernels (csrc/kernels).

Every op runs the native kernel on the caller's current HIP stream; there is
no PyTorch fallback. Calling on CPU tensors, or without the built extension,
raises — a GPU test can never pass on a silent eager path.

Layout conventions: activations are bf16 NHWC; conv/linear weights are packed
``[Npad, Kpad]`` bf16 with k = (kh*KW + kw)*Cin + c (see ``pack_conv_weight``).
"""
from __future__ import annotations


import torch

from .. import native


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("dmlc.ops kernels need CUDA/HIP tensors (no CPU fallback)")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def conv_kpad(cin: int, kh: int, kw: int, stem: bool = False) -> int:
    return native().conv_kpad(cin, kh, kw, stem)


def stem_row_width(size: int, pad: int, kw: int, stride: int) -> int:
    return native().stem_row_width(size, pad, kw, stride)


def conv_npad(n: int) -> int:
    return native().conv_npad(n)


_ZERO = {}


def _zero_page(device) -> torch.Tensor:
    z = _ZERO.get(device)
    if z is None:
        z = _ZERO[device] = torch.zeros(64, dtype=torch.float32, device=device)
    return z


def pack_conv_weight(w: torch.Tensor, scale: torch.Tensor | None = None, stem: bool = False,
                     device=None) -> torch.Tensor:
    """[Cout, Cin, KH, KW] fp32 -> packed bf16 [Npad, Kpad] (per-row scale
    folded in, e.g. a BN scale). k = (kh*KW + kw)*Cin + c; for the 3-channel
    stem k = kh*CPK*8 + kw*3 + c with CPK = ceil(3*KW/8)."""
    cout, cin, kh, kw = w.shape
    kpad, npad = conv_kpad(cin, kh, kw, stem), conv_npad(cout)
    w = w.float()
    if scale is not None:
        w = w * scale.float().view(-1, 1, 1, 1)
    out = torch.zeros(npad, kpad)
    if stem:
        cpk = (kw * 3 + 7) // 8
        wp = torch.zeros(cout, kh, cpk * 8)
        wp[:, :, : kw * 3] = w.permute(0, 2, 3, 1).reshape(cout, kh, kw * 3)
        out[:cout, : kh * cpk * 8] = wp.reshape(cout, -1)
    else:
        out[:cout, : kh * kw * cin] = w.permute(0, 2, 3, 1).reshape(cout, -1)
    return out.to(torch.bfloat16).to(device) if device is not None else out.to(torch.bfloat16)


def stem_image(x_nhwc3: torch.Tensor, pad: int, row_width: int) -> torch.Tensor:
    """Reference construction of the stem's input: [B, H+2p, row_width, 3]
    with the image at (p, p) and zeros elsewhere."""
    B, H, W, _ = x_nhwc3.shape
    out = torch.zeros(B, H + 2 * pad, row_width, 3, dtype=x_nhwc3.dtype, device=x_nhwc3.device)
    out[:, pad:pad + H, pad:pad + W] = x_nhwc3
    return out.contiguous()


def fc(x: torch.Tensor, w_packed: torch.Tensor, cout: int, bias: torch.Tensor | None = None, relu: bool = False,
       out_f32: bool = False, splits: int = 0, out: torch.Tensor | None = None) -> torch.Tensor:
    """Fully connected layer at M <= 256 rows on fc_gemm.hip: x bf16 [M, K]
    (K = w_packed.shape[1], a multiple of 64), w_packed [Npad, K] (Npad % 128
    == 0) -> [M, cout] bf16 (fp32 with out_f32). splits: K slices (0: the
    engine's choice), fp32 partials reduced with the bias and ReLU. ``out``:
    the [M, cout] tensor to write."""
    _need_cuda(x, w_packed, bias)
    C = native()
    M, K = x.shape
    if K != w_packed.shape[1]:
        raise ValueError("fc: x's K must equal the packed weight's K")
    if splits <= 0:
        splits = C.fc_gemm_splits(M, K, w_packed.shape[0], torch.cuda.get_device_properties(x.device).multi_processor_count)
    ws = torch.empty(splits * M * w_packed.shape[0], device=x.device, dtype=torch.float32)
    return conv2d(x.contiguous().view(M, 1, 1, K), w_packed, cout, 1, 1, bias=bias, relu=relu, out_f32=out_f32,
                  split_k=splits, tile=C.CONV_FC, ws=ws,
                  out=None if out is None else _out_tensor(out, (M, cout), torch.float32 if out_f32 else
                                                           torch.bfloat16, x.device, "fc")).view(M, cout)


def conv2d(x: torch.Tensor, w_packed: torch.Tensor, cout: int, kh: int, kw: int, stride: int = 1,
           pad: int = 0, bias: torch.Tensor | None = None, res: torch.Tensor | None = None,
           relu: bool = False, out_f32: bool = False, split_k: int = 1, tile: int = -1,
           out: torch.Tensor | None = None, stem: bool = False, out_hw: tuple | None = None,
           max_blocks: int = 0, ws: torch.Tensor | None = None, num_cus: int = 0,
           x2: torch.Tensor | None = None) -> torch.Tensor:
    """Implicit-GEMM conv on MFMA. x: bf16 NHWC [B,H,W,Cin] (Cin % 64 == 0),
    or with ``stem`` the padded packed RGB image (``stem_image``) plus the
    output size ``out_hw`` (the padding is already in the image).
    Returns [B,Ho,Wo,cout] (bf16, or fp32 if out_f32).

    tile=CONV_1X1 only: ``num_cus`` sizes the persistent grid (0: the
    device's count), and ``x2`` [B,H,W,cin2] is a second bf16 input
    concatenated along K (w_packed = [W | W2], K = Cin + cin2)."""
    _need_cuda(x, w_packed, bias, res, x2)
    C = native()
    B, H, W, Cin = x.shape
    if stem:
        Ho, Wo = out_hw
    else:
        Ho, Wo = C.conv_out_dim(H, kh, stride, pad), C.conv_out_dim(W, kw, stride, pad)
    if out is None:
        out = torch.empty(B, Ho, Wo, cout, device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    if bias is not None:
        bias = bias.float().contiguous()
        if bias.numel() < w_packed.shape[0]:
            bias = torch.nn.functional.pad(bias, (0, w_packed.shape[0] - bias.numel()))
    bt_ws, bt_bytes, bt_splits = None, 0, 1
    if C.CONV_BIGTILE0 <= tile < C.CONV_BIGTILE0 + 2:  # 8-wave big-tile kernel (conv_bigtile.hip); split_k = K slices (0: engine's choice)
        bt_splits = split_k if split_k > 0 else C.conv_bigtile_splits(
            B, Ho, Wo, w_packed.shape[0], w_packed.shape[1], tile - C.CONV_BIGTILE0,
            torch.cuda.get_device_properties(x.device).multi_processor_count)
        split_k = 1
        bm, bn = 256, (256 if tile == C.CONV_BIGTILE0 else 128)
        slabs = -(-B * Ho * Wo // bm) * (w_packed.shape[0] // bn) * (bt_splits - 1)
        bt_ws = _bigtile_ws(x.device, C.conv_bigtile_ws_bytes(slabs))
        bt_bytes = bt_ws.numel()
    if ws is None and split_k > 1:
        ws = torch.empty(split_k * B * Ho * Wo * w_packed.shape[0], device=x.device, dtype=torch.float32)
    C.conv2d(x=_ptr(x.contiguous()), w=_ptr(w_packed), bias=_ptr(bias), res=_ptr(res), y=_ptr(out), B=B, H=H,
             W=W, Cin=Cin, KH=kh, KW=kw, stride=stride, pad=pad, N=cout, Npad=w_packed.shape[0],
             Kpad=w_packed.shape[1], ldo=cout, relu=relu, out_f32=out_f32, split_k=split_k, ws=_ptr(ws),
             tile=tile, zero=_ptr(_zero_page(x.device)), stem=stem, Ho=Ho, Wo=Wo, max_blocks=max_blocks,
             stream=_stream(), bt_ws=_ptr(bt_ws), bt_ws_bytes=bt_bytes, bt_splits=bt_splits, num_cus=num_cus,
             x2=_ptr(None if x2 is None else _second_input(x, x2)), cin2=0 if x2 is None else x2.shape[-1])
    return out


def _second_input(x: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    if x2.dim() != 4 or tuple(x2.shape[:3]) != tuple(x.shape[:3]) or x2.dtype != x.dtype or not x2.is_contiguous():
        raise ValueError("conv2d: x2 must be a contiguous [B,H,W,cin2] tensor of x's dtype")
    return x2


_BT_WS: dict = {}
BT_STAMPS = None
_PHASE_STAMPS = False


def set_phase_stamps(on: bool) -> None:
    """Record per-workgroup phase stamps (start / prologue / loop / epilogue,
    100 MHz) of every following conv3x3_stream launch into BT_STAMPS (a
    measurement hook for tools/conv_bench.py; off by default)."""
    global _PHASE_STAMPS
    _PHASE_STAMPS = bool(on)


def _bigtile_ws(device: torch.device, nbytes: int) -> torch.Tensor:
    """Per-device big-tile split-K workspace (hand-off flags zeroed once, then
    fp32 slabs); grown on demand."""
    C = native()
    t = _BT_WS.get(device.index)
    if t is None or t.numel() < nbytes:
        if t is not None:
            torch.cuda.synchronize(device)
        t = torch.empty(max(nbytes, C.conv_bigtile_ws_bytes(0)), dtype=torch.uint8, device=device)
        t[:C.conv_bigtile_ws_header_bytes()].zero_()
        _BT_WS[device.index] = t
    return t


def bigtile_error(device: torch.device) -> bool:
    """True if a big-tile split-K hand-off timed out on `device` (results invalid)."""
    C = native()
    t = _BT_WS.get(device.index)
    if t is None:
        return False
    hdr = C.conv_bigtile_ws_header_bytes()
    return int(t[hdr - 256:hdr - 252].view(torch.int32).item()) != 0


def conv3x3_rows(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, res: torch.Tensor | None = None,
                 relu: bool = True, strip: int | None = None, frag: bool = False) -> torch.Tensor:
    """Direct 3x3/s1/p1 conv (conv3x3_rows.hip) on NHWC bf16 [B,56,56,64] with
    the conv2d packed weights [64, 576]; + bias (+ residual), ReLU. frag: the
    register-weight variant (weights in fragment order, 2 workgroups per CU)."""
    _need_cuda(x, w_packed, bias, res)
    C = native()
    B, H, W, Cin = x.shape
    if not C.conv3x3_rows_supported(H, W, Cin, w_packed.shape[0]):
        raise ValueError("conv3x3_rows: unsupported shape")
    if strip is None:
        cus = torch.cuda.get_device_properties(x.device).multi_processor_count
        strip = C.conv3x3_rows_pick_strip(B, H, 2 * cus if frag else cus)
    y = torch.empty_like(x)
    wf = stream_weight_frag(w_packed) if frag else None
    C.conv3x3_rows(_ptr(x.contiguous()), _ptr(w_packed.contiguous()), _ptr(bias.float().contiguous()),
                   _ptr(None if res is None else res.contiguous()), _ptr(y), _ptr(_zero_page(x.device)), B, H, W,
                   Cin, relu, strip, _stream(), _ptr(wf))
    return y


def conv3x3_block(x: torch.Tensor, w1_packed: torch.Tensor, b1: torch.Tensor, w2_packed: torch.Tensor,
                  b2: torch.Tensor) -> torch.Tensor:
    """A whole 56x56x64 basic block (conv3x3_block.hip) on NHWC bf16:
    relu(conv2(relu(conv1(x) + b1)) + b2 + x), the intermediate kept in LDS
    (rounded to bf16 like a stored activation). w*_packed: conv2d packed
    weights [64, 576]."""
    _need_cuda(x, w1_packed, b1, w2_packed, b2)
    C = native()
    B, H, W, Cin = x.shape
    if not C.conv3x3_block_supported(H, W, Cin) or w1_packed.shape[0] != Cin or w2_packed.shape[0] != Cin:
        raise ValueError("conv3x3_block: unsupported shape")
    x = x.contiguous()
    y = torch.empty_like(x)
    wf1, wf2 = stream_weight_frag(w1_packed), stream_weight_frag(w2_packed)
    C.conv3x3_block(_ptr(x), _ptr(wf1), _ptr(b1.float().contiguous()), _ptr(wf2), _ptr(b2.float().contiguous()),
                    _ptr(y), _ptr(_zero_page(x.device)), B, _stream())
    return y


def conv3x3_s2rows(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, wd_packed: torch.Tensor | None,
                   bd: torch.Tensor | None, relu: bool = True):
    """ResNet layer2.0's stride-2 3x3 conv [B,56,56,64] -> [B,28,28,128]
    and its 1x1/s2 downsample in one row-streaming kernel
    (conv3x3_s2rows.hip): returns (relu?(conv3x3(x) + bias), conv1x1_s2(x)
    + bd). w_packed: conv2d packed weights [128, 576]; wd_packed [128, 64].
    wd_packed = bd = None: the conv alone (the downsample then belongs to
    ``conv3x3_rows28(downsample=)``), returns y only."""
    _need_cuda(x, w_packed, bias, wd_packed, bd)
    C = native()
    B, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    if (wd_packed is None) != (bd is None):
        raise ValueError("conv3x3_s2rows: wd_packed and bd go together")
    if (not C.conv3x3_s2rows_supported(H, W, Cin, Cout) or tuple(w_packed.shape) != (Cout, 9 * Cin)
            or (wd_packed is not None and tuple(wd_packed.shape) != (Cout, Cin))):
        raise ValueError("conv3x3_s2rows: unsupported shape")
    x = x.contiguous()
    y = torch.empty(B, H // 2, W // 2, Cout, dtype=x.dtype, device=x.device)
    yd = torch.empty_like(y) if wd_packed is not None else None
    wf = stream_weight_frag(w_packed)
    wdf = stream_weight_frag(wd_packed) if wd_packed is not None else None
    C.conv3x3_s2rows(_ptr(x), _ptr(wf), _ptr(bias.float().contiguous()), _ptr(wdf),
                     _ptr(None if bd is None else bd.float().contiguous()), _ptr(y), _ptr(yd),
                     _ptr(_zero_page(x.device)), B, relu, _stream())
    return y if wd_packed is None else (y, yd)


def conv3x3_s2rows128(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, relu: bool = True,
                      out_inv_scale: float = 0.0):
    """ResNet50 layer2.0.conv2, [B,56,56,128] -> [B,28,28,128] stride 2, one
    row-streaming weight-stationary workgroup per image
    (conv3x3_s2rows.hip, its 128-channel shape). Returns bf16, or e4m3 bytes (uint8) of
    relu?(conv + bias) * out_inv_scale when out_inv_scale > 0."""
    _need_cuda(x, w_packed, bias)
    C = native()
    B, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    if not C.conv3x3_s2rows128_supported(H, W, Cin, Cout) or tuple(w_packed.shape) != (Cout, 9 * Cin):
        raise ValueError("conv3x3_s2rows128: unsupported shape")
    x = x.contiguous()
    dt = torch.uint8 if out_inv_scale > 0 else x.dtype
    y = torch.empty(B, H // 2, W // 2, Cout, dtype=dt, device=x.device)
    wf = stream_weight_frag(w_packed)
    C.conv3x3_s2rows128(_ptr(x), _ptr(wf), _ptr(bias.float().contiguous()), _ptr(y), B, relu, float(out_inv_scale),
                        _stream())
    return y


def conv_small(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, res: torch.Tensor | None = None,
               relu: bool = True, stride: int = 1, wd_packed: torch.Tensor | None = None,
               bd: torch.Tensor | None = None, mf: int | None = None):
    """Query-batch 3x3/p1 conv (conv_small.hip) on NHWC bf16 [B,H,W,CI]:
    relu?(conv3x3(x) + bias (+ res)). w_packed: conv2d packed weights
    [Cout, 9 CI]. With stride 2 and wd_packed [Cout, CI] / bd also returns the
    1x1/s2 downsample conv1x1_s2(x) + bd: (y, yd)."""
    _need_cuda(x, w_packed, bias, res, wd_packed, bd)
    C = native()
    B, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    if not C.conv_small_supported(H, W, Cin, Cout, stride) or tuple(w_packed.shape) != (Cout, 9 * Cin):
        raise ValueError("conv_small: unsupported shape")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if res is not None and tuple(res.shape) != (B, Ho, Wo, Cout):
        raise ValueError("conv_small: residual shape")
    if wd_packed is not None and (stride != 2 or bd is None or tuple(wd_packed.shape) != (Cout, Cin)):
        raise ValueError("conv_small: downsample needs stride 2, bd and [Cout, Cin] weights")
    if mf is None:
        cus = torch.cuda.get_device_properties(x.device).multi_processor_count
        mf = C.conv_small_pick_mf(B, H, W, Cin, Cout, stride, cus)
    x = x.contiguous()
    y = torch.empty(B, Ho, Wo, Cout, dtype=x.dtype, device=x.device)
    yd = torch.empty_like(y) if wd_packed is not None else None
    wdf = stream_weight_frag(wd_packed) if wd_packed is not None else None
    C.conv_small(_ptr(x), _ptr(stream_weight_frag(w_packed)), _ptr(bias.float().contiguous()),
                 _ptr(None if res is None else res.contiguous()), _ptr(y), B, H, W, Cin, Cout, stride, relu, mf,
                 _stream(), _ptr(wdf), _ptr(None if bd is None else bd.float().contiguous()), _ptr(yd))
    return (y, yd) if wd_packed is not None else y


def conv3x3_rows28(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, res: torch.Tensor | None = None,
                   relu: bool = True, downsample: tuple | None = None, out_inv_scale: float = 0.0) -> torch.Tensor:
    """Weight-stationary row-streaming 3x3/s1/p1 conv on [B,28,28,128] ->
    128 channels (conv3x3_rows28.hip): relu?(conv(x) + bias (+ res)).
    w_packed: conv2d packed weights [128, 1152].

    downsample=(x56 [B,56,56,64], wd_packed [128, 64], bd): the block's 1x1/s2
    downsample of x56 as 2 more K steps of this conv, in place of a residual:
    relu?(conv(x) + bias + conv1x1_s2(x56) + bd).

    out_inv_scale > 0: returns e4m3 bytes (uint8) of relu?(conv(x) + bias) *
    out_inv_scale; no residual and no downsample with it."""
    _need_cuda(x, w_packed, bias, res)
    C = native()
    B, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    if not C.conv3x3_rows28_supported(H, W, Cin, Cout) or tuple(w_packed.shape) != (Cout, 9 * Cin):
        raise ValueError("conv3x3_rows28: unsupported shape")
    if res is not None and tuple(res.shape) != (B, H, W, Cout):
        raise ValueError("conv3x3_rows28: residual shape")
    if out_inv_scale > 0 and (res is not None or downsample is not None):
        raise ValueError("conv3x3_rows28: e4m3 output takes neither a residual nor a downsample")
    x = x.contiguous()
    xds = wds = bds = None
    if downsample is not None:
        if res is not None:
            raise ValueError("conv3x3_rows28: the downsample takes the residual's place")
        x56, wd_packed, bd = downsample
        _need_cuda(x56, wd_packed, bd)
        if tuple(x56.shape) != (B, 2 * H, 2 * W, Cin // 2) or x56.dtype != x.dtype \
                or tuple(wd_packed.shape) != (Cout, Cin // 2) or bd.numel() != Cout:
            raise ValueError("conv3x3_rows28: downsample needs x56 [B, 56, 56, 64], wd_packed [128, 64], bd [128]")
        xds, wds, bds = x56.contiguous(), stream_weight_frag(wd_packed), bd.float().contiguous()
    y = torch.empty(B, H, W, Cout, dtype=torch.uint8 if out_inv_scale > 0 else x.dtype, device=x.device)
    C.conv3x3_rows28(_ptr(x), _ptr(stream_weight_frag(w_packed)), _ptr(bias.float().contiguous()),
                     _ptr(None if res is None else res.contiguous()), _ptr(y), B, relu, _stream(),
                     float(out_inv_scale), _ptr(xds), _ptr(wds), _ptr(bds))
    return y


def stream_weight_frag(w_packed: torch.Tensor, cout: int | None = None) -> torch.Tensor:
    """Packed conv weights [Npad, K] -> the stream conv's fragment order
    [Cout/32][K/32][2][64 lanes][8]: lane l of fragment nf of channel group g,
    K-tile t holds channel 32g + perm32(16nf + (l & 15)), k = 32t + 8(l >> 4)
    + e, perm32(n) = 8((n & 15) >> 2) + 4(n >> 4) + (n & 3)."""
    cout = w_packed.shape[0] if cout is None else cout
    K = w_packed.shape[1]
    n = torch.arange(32)
    perm = 8 * ((n & 15) >> 2) + 4 * (n >> 4) + (n & 3)            # tile row -> channel
    lane = torch.arange(64)
    rows = perm[(torch.arange(2).view(2, 1) * 16 + (lane & 15).view(1, 64))]  # [nf, lane] -> channel in group
    w = w_packed[:cout].view(cout // 32, 32, K // 32, 4, 8)          # [g, ch, t, kq, e]
    kq = (lane >> 4).view(1, 64).expand(2, 64)
    # advanced indices separated by a slice go first: [nf, lane, g, t, e]
    out = w[:, rows.to(w.device), :, kq.to(w.device), :]
    return out.permute(2, 3, 0, 1, 4).contiguous()


def conv3x3_stream(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, res: torch.Tensor | None = None,
                   relu: bool = True, stride: int = 1, downsample: tuple | None = None,
                   frag: bool | torch.Tensor = False, pool: bool = False, store_y: bool = True,
                   out: torch.Tensor | None = None):
    """Direct 3x3/p1 conv (conv3x3_stream.hip) on NHWC bf16 with the conv2d
    packed weights; + bias (+ residual), ReLU. Stride 1: [B,28,28,128],
    [B,14,14,256], [B,7,7,512]; stride 2: [B,56,56,64] -> 128 channels,
    [B,28,28,128] -> 256, [B,14,14,256] -> 512.

    downsample=(wd_packed [Cout, Cin], bd[, wd_frag]): stride 2 only; also
    computes the 1x1/s2 conv + bias from the same resident input and returns
    (y, yd); wd_frag = stream_weight_frag(wd_packed), precomputed for graph
    capture.

    pool (the 7x7x512 stride-1 conv only): also returns the global average
    pool of the bf16 output, bf16 [B, Cout]: (y, pooled). With store_y=False
    the activation is not written (y, or ``out`` if given, is left as it was)."""
    _need_cuda(x, w_packed, bias, res, out)
    C = native()
    B, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    if not C.conv3x3_stream_supported(H, W, Cin, Cout, stride):
        raise ValueError("conv3x3_stream: unsupported shape")
    if (pool or not store_y) and not C.conv3x3_stream_pool_supported(H, W, Cin, Cout, stride):
        raise ValueError("conv3x3_stream: the fused average pool needs the 7x7x512 stride-1 conv")
    if not store_y and not pool:
        raise ValueError("conv3x3_stream: store_y=False without pool computes nothing")
    if (pool or not store_y) and downsample is not None:
        raise ValueError("conv3x3_stream: no fused average pool with a downsample")
    if out is None:
        y = torch.empty(B, H // stride, W // stride, Cout, dtype=x.dtype, device=x.device)
    else:
        if tuple(out.shape) != (B, H // stride, W // stride, Cout) or out.dtype != x.dtype or not out.is_contiguous():
            raise ValueError("conv3x3_stream: out must be a contiguous [B, Ho, Wo, Cout] tensor of x's dtype")
        y = out
    pooled = torch.empty(B, Cout, dtype=x.dtype, device=x.device) if pool else None
    stamps = 0
    if _PHASE_STAMPS:  # per-workgroup phase stamps of the stream conv (tools/conv_bench.py --stamps)
        global BT_STAMPS
        if BT_STAMPS is None:
            BT_STAMPS = torch.zeros(1 << 16, dtype=torch.int64, device=x.device)
        stamps = _ptr(BT_STAMPS)
    yd = wd = bd = None
    if downsample is not None:
        wd, bd = downsample[0].contiguous(), downsample[1].float().contiguous()
        _need_cuda(wd, bd)
        if stride != 2 or tuple(wd.shape) != (Cout, Cin):
            raise ValueError("conv3x3_stream: downsample needs stride 2 and weights [Cout, Cin]")
        yd = torch.empty_like(y)
    wf = None
    if frag is not False and frag is not None:  # True, or the fragment-order weights (graph capture)
        if not C.conv3x3_stream_uses_frag(H, W, Cin, Cout, stride):
            raise ValueError("conv3x3_stream: no register-weight variant for this shape")
        wf = frag if isinstance(frag, torch.Tensor) else stream_weight_frag(w_packed)
    wdf = None
    if wf is not None and wd is not None:
        wdf = downsample[2] if len(downsample) > 2 else stream_weight_frag(wd)
    C.conv3x3_stream(_ptr(x.contiguous()), _ptr(w_packed.contiguous()), _ptr(bias.float().contiguous()),
                     _ptr(None if res is None else res.contiguous()), _ptr(y), _ptr(_zero_page(x.device)), B, H, W,
                     Cin, Cout, stride, relu, _stream(), stamps, _ptr(wd), _ptr(bd), _ptr(yd), _ptr(wf), _ptr(wdf),
                     pool=_ptr(pooled), store_y=store_y)
    if pool:
        return y, pooled
    return y if downsample is None else (y, yd)


FP8 = torch.float8_e4m3fn  # OCP e4m3 (gfx950), max 448
FP8_MAX = 448.0


def quantize_fp8(t: torch.Tensor, scale: float) -> torch.Tensor:
    """e4m3(t / scale), saturating."""
    return (t.float() / scale).clamp(-FP8_MAX, FP8_MAX).to(FP8)


def pack_conv_weight_fp8(w: torch.Tensor, device=None) -> tuple[torch.Tensor, torch.Tensor]:
    """[Cout, Cin, KH, KW] -> (e4m3 [Npad, Kpad] with a per-output-channel
    scale, fp32 scales [Npad]); k = (kh*KW + kw)*Cin + c as for bf16."""
    cout, cin, kh, kw = w.shape
    kpad, npad = conv_kpad(cin, kh, kw), conv_npad(cout)
    wk = torch.zeros(npad, kpad)
    wk[:cout, : kh * kw * cin] = w.float().permute(0, 2, 3, 1).reshape(cout, -1)
    s = (wk.abs().amax(1) / FP8_MAX).clamp_min(1e-12)
    q = quantize_fp8(wk / s[:, None], 1.0)
    return (q.to(device), s.to(device)) if device is not None else (q, s)


def conv2d_fp8(x: torch.Tensor, w_q: torch.Tensor, alpha: torch.Tensor, cout: int, kh: int, kw: int,
               stride: int = 1, pad: int = 0, bias: torch.Tensor | None = None, res: torch.Tensor | None = None,
               res_scale: float = 1.0, relu: bool = False, out_scale: float | None = None,
               tile: int = -1, out: torch.Tensor | None = None, num_cus: int = 0,
               x2: torch.Tensor | None = None, max_blocks: int = 0) -> torch.Tensor:
    """fp8 implicit-GEMM conv (block-scaled e4m3 MFMA). x: e4m3 NHWC
    (Cin % 128 == 0) or bf16 (then w_q is bf16-packed and alpha unused).
    alpha = s_x * s_w[n]; residual e4m3 scaled by res_scale; output e4m3
    with scale out_scale (or bf16 when out_scale is None). ``out``: the
    output tensor to write; ``num_cus`` / ``x2`` / ``max_blocks``: as for
    ``conv2d``."""
    _need_cuda(x, w_q, alpha, bias, res, out, x2)
    C = native()
    B, H, W, Cin = x.shape
    in8 = x.dtype == FP8
    Ho, Wo = C.conv_out_dim(H, kh, stride, pad), C.conv_out_dim(W, kw, stride, pad)
    out8 = out_scale is not None
    y = _out_tensor(out, (B, Ho, Wo, cout), FP8 if out8 else torch.bfloat16, x.device, "conv2d_fp8")
    if bias is not None:
        bias = bias.float().contiguous()
        if bias.numel() < w_q.shape[0]:
            bias = torch.nn.functional.pad(bias, (0, w_q.shape[0] - bias.numel()))
    al = alpha.float().contiguous() if alpha is not None else None
    C.conv2d(x=_ptr(x.contiguous()), w=_ptr(w_q), bias=_ptr(bias), res=_ptr(res), y=_ptr(y), B=B, H=H, W=W, Cin=Cin,
             KH=kh, KW=kw, stride=stride, pad=pad, N=cout, Npad=w_q.shape[0], Kpad=w_q.shape[1], ldo=cout,
             relu=relu, out_f32=False, split_k=1, ws=0, tile=tile, zero=_ptr(_zero_page(x.device)), stem=False,
             Ho=Ho, Wo=Wo, max_blocks=max_blocks, stream=_stream(), in_fp8=in8, out_fp8=out8, alpha=_ptr(al),
             res_scale=res_scale, out_inv_scale=(1.0 / out_scale) if out8 else 1.0, num_cus=num_cus,
             x2=_ptr(None if x2 is None else _second_input(x, x2)), cin2=0 if x2 is None else x2.shape[-1])
    return y


def _out_tensor(out, shape, dtype, device, what: str) -> torch.Tensor:
    """``out`` checked (contiguous, shape, dtype; e4m3 also as uint8 bytes), or a new tensor."""
    if out is None:
        return torch.empty(*shape, device=device, dtype=dtype)
    _need_cuda(out)
    ok = out.dtype == dtype or (dtype == FP8 and out.dtype == torch.uint8)
    if tuple(out.shape) != tuple(shape) or not ok or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous {tuple(shape)} tensor of {dtype}")
    return out


def _e4m3(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype not in (FP8, torch.uint8):
        raise ValueError(f"{what} must be e4m3 (float8_e4m3fn, or its bytes as uint8)")
    return t.contiguous()


def _f32(t: torch.Tensor, n: int, what: str) -> torch.Tensor:
    if t.numel() < n:
        raise ValueError(f"{what} holds {n} values")
    return t.float().contiguous()


def bottleneck56(x: torch.Tensor, w1_q: torch.Tensor, a1: torch.Tensor, b1: torch.Tensor, w2_packed: torch.Tensor,
                 b2: torch.Tensor, w3_packed: torch.Tensor, b3: torch.Tensor, res_scale: float, out_scale: float,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """ResNet50's layer1 identity bottleneck as one kernel (bottleneck56.hip)
    on e4m3 NHWC [B,56,56,256] (value = code * res_scale):
      t1 = bf16(relu(conv1x1(x codes, w1_q codes) * a1 + b1))   64 channels
      t2 = bf16(relu(conv3x3(t1, w2) + b2))                     64 channels
      y  = e4m3(relu(conv1x1(t2, w3) + b3 + x) / out_scale)     256 channels
    w1_q / a1: ``pack_conv_weight_fp8`` of the [64,256,1,1] weights, a1 =
    s_x * s_w1; w2_packed [64, 576] and w3_packed [256, 64]: ``pack_conv_weight``
    (bf16). conv3's weights are re-rounded to bf16 after the multiplication
    by 1 / out_scale (kernels.h). ``out``: the e4m3 output to write."""
    _need_cuda(x, w1_q, a1, b1, w2_packed, b2, w3_packed, b3, out)
    C = native()
    if x.dim() != 4:
        raise ValueError("bottleneck56: x is e4m3 NHWC [B,56,56,256]")
    B, H, W, Cin = x.shape
    if not C.bottleneck56_supported(H, W, Cin, 64) or tuple(w1_q.shape[-2:]) != (64, 256) \
            or tuple(w2_packed.shape) != (64, 576) or tuple(w3_packed.shape) != (256, 64) \
            or w2_packed.dtype != torch.bfloat16 or w3_packed.dtype != torch.bfloat16:
        raise ValueError("bottleneck56: unsupported shape / dtype")
    x, w1_q = _e4m3(x, "bottleneck56: x"), _e4m3(w1_q, "bottleneck56: w1_q")
    y = _out_tensor(out, (B, H, W, Cin), FP8, x.device, "bottleneck56")
    if y.data_ptr() == x.data_ptr():
        raise ValueError("bottleneck56: in-place not supported")
    wf2, wf3 = stream_weight_frag(w2_packed), stream_weight_frag(w3_packed)
    C.bottleneck56(_ptr(x), _ptr(w1_q), _ptr(_f32(a1, 64, "a1")), _ptr(_f32(b1, 64, "b1")), _ptr(wf2),
                   _ptr(_f32(b2, 64, "b2")), _ptr(wf3), _ptr(_f32(b3, 256, "b3")), _ptr(y), float(res_scale),
                   1.0 / float(out_scale), B, _stream())
    return y


def bottleneck56_head(x: torch.Tensor, w1_packed: torch.Tensor, b1: torch.Tensor, w2_packed: torch.Tensor,
                      b2: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """ResNet50 layer1.0's reduce 1x1 + 3x3 convs as one kernel
    (bottleneck56.hip) on bf16 NHWC [B,56,56,64]:
    relu(conv3x3(bf16(relu(conv1x1(x) + b1))) + b2), bf16 [B,56,56,64].
    w1_packed [64, 64], w2_packed [64, 576]: ``pack_conv_weight``."""
    _need_cuda(x, w1_packed, b1, w2_packed, b2, out)
    C = native()
    if x.dim() != 4:
        raise ValueError("bottleneck56_head: x is bf16 NHWC [B,56,56,64]")
    B, H, W, Cin = x.shape
    if not C.bottleneck56_supported(H, W, 4 * Cin, Cin) or x.dtype != torch.bfloat16 \
            or tuple(w1_packed.shape) != (64, 64) or tuple(w2_packed.shape) != (64, 576) \
            or w1_packed.dtype != torch.bfloat16 or w2_packed.dtype != torch.bfloat16:
        raise ValueError("bottleneck56_head: unsupported shape / dtype")
    x = x.contiguous()
    y = _out_tensor(out, (B, H, W, Cin), torch.bfloat16, x.device, "bottleneck56_head")
    if y.data_ptr() == x.data_ptr():
        raise ValueError("bottleneck56_head: in-place not supported")
    C.bottleneck56_head(_ptr(x), _ptr(w1_packed.contiguous()), _ptr(_f32(b1, 64, "b1")),
                        _ptr(stream_weight_frag(w2_packed)), _ptr(_f32(b2, 64, "b2")), _ptr(y), B, _stream())
    return y


def conv1x1_chain(x: torch.Tensor, w_q: torch.Tensor, alpha: torch.Tensor, bias: torch.Tensor, res: torch.Tensor,
                  res_scale: float, out_scale: float, w2_q: torch.Tensor, alpha2: torch.Tensor, bias2: torch.Tensor,
                  out_scale2: float, num_cus: int = 0, out: torch.Tensor | None = None,
                  out2: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """A bottleneck's e4m3 expand conv and the next bottleneck's reduce conv on
    its output in one launch (conv1x1.hip's chained form), both 1x1 / stride 1
    with ReLU: y = e4m3(relu(x . w * alpha + bias + res * res_scale) /
    out_scale) [B,H,W,512] from x [B,H,W,128], y2 = e4m3(relu(y codes . w2 *
    alpha2 + bias2) / out_scale2) [B,H,W,128] (alpha2 = out_scale * s_w2).
    w_q / w2_q: ``pack_conv_weight_fp8``. num_cus sizes the persistent grid
    (0: the device's count). Returns (y, y2); ``out`` / ``out2`` to write."""
    _need_cuda(x, w_q, alpha, bias, res, w2_q, alpha2, bias2, out, out2)
    C = native()
    if x.dim() != 4 or w_q.dim() != 2 or w2_q.dim() != 2:
        raise ValueError("conv1x1_chain: x is e4m3 NHWC, the weights are packed [N, K]")
    B, H, W, Cin = x.shape
    N, N2 = w_q.shape[0], w2_q.shape[0]
    if w_q.shape[1] != Cin or w2_q.shape[1] != N or tuple(res.shape) != (B, H, W, N):
        raise ValueError("conv1x1_chain: operand shapes")
    x, res = _e4m3(x, "conv1x1_chain: x"), _e4m3(res, "conv1x1_chain: res")
    w_q, w2_q = _e4m3(w_q, "conv1x1_chain: w_q"), _e4m3(w2_q, "conv1x1_chain: w2_q")
    y = _out_tensor(out, (B, H, W, N), FP8, x.device, "conv1x1_chain")
    y2 = _out_tensor(out2, (B, H, W, N2), FP8, x.device, "conv1x1_chain")
    args = dict(x=_ptr(x), w=_ptr(w_q), alpha=_ptr(_f32(alpha, N, "alpha")), bias=_ptr(_f32(bias, N, "bias")),
                res=_ptr(res), y=_ptr(y), w2=_ptr(w2_q), alpha2=_ptr(_f32(alpha2, N2, "alpha2")),
                bias2=_ptr(_f32(bias2, N2, "bias2")), y2=_ptr(y2), B=B, H=H, W=W, Cin=Cin, N=N, N2=N2,
                res_scale=float(res_scale), out_inv_scale=1.0 / float(out_scale),
                out_inv_scale2=1.0 / float(out_scale2), relu=True, relu2=True, zero=_ptr(_zero_page(x.device)))
    if not C.conv1x1_chain_supported(**args):
        raise ValueError("conv1x1_chain: unsupported pair of convs")
    C.conv1x1_chain(**args, num_cus=num_cus, stream=_stream())
    return y, y2


def stream8_weight_frag(w_q: torch.Tensor, cout: int) -> torch.Tensor:
    """e4m3 packed conv weights [Npad, K] (pack_conv_weight_fp8) -> the e4m3
    3x3 conv's fragment order (conv3x3_stream8.hip): [Cout/32][K/128][2 nf][2
    h][64 lanes][16 B], lane l of (group g, K-tile t, nf, h) holding
    W[32g + perm32(16nf + (l & 15))][128t + 32fq + 16(h ^ (fq & 1)) + 0..15],
    fq = l >> 4 (the odd-fq half swap matches the kernel's X reads)."""
    w = w_q[:cout].view(torch.uint8)
    K = w.shape[1]
    n = torch.arange(32)
    perm = 8 * ((n & 15) >> 2) + 4 * (n >> 4) + (n & 3)
    lane = torch.arange(64)
    fq = lane >> 4
    G, T = cout // 32, K // 128
    g = torch.arange(G).view(G, 1, 1, 1, 1, 1)
    t = torch.arange(T).view(1, T, 1, 1, 1, 1)
    nf = torch.arange(2).view(1, 1, 2, 1, 1, 1)
    h = torch.arange(2).view(1, 1, 1, 2, 1, 1)
    ln = lane.view(1, 1, 1, 1, 64, 1)
    e = torch.arange(16).view(1, 1, 1, 1, 1, 16)
    row = 32 * g + perm[16 * nf + (ln & 15)]
    col = 128 * t + 32 * (ln >> 4) + 16 * (h ^ ((ln >> 4) & 1)) + e
    del fq
    row, col = torch.broadcast_tensors(row, col)
    return w[row.to(w.device), col.to(w.device)].contiguous()


def conv3x3_stream8(x: torch.Tensor, w_q: torch.Tensor, alpha: torch.Tensor, bias: torch.Tensor, relu: bool = True,
                    out_scale: float = 1.0, frag: torch.Tensor | None = None, stride: int = 1) -> torch.Tensor:
    """e4m3 3x3/p1 conv (conv3x3_stream8.hip) on e4m3 NHWC: stride 1 on
    [B,14,14,256] / [B,7,7,512], stride 2 on [B,28,28,256] / [B,14,14,512]:
    e4m3(relu?(acc * alpha + bias) / out_scale) with acc = conv of the e4m3
    values. w_q / alpha: pack_conv_weight_fp8 (alpha = s_x * s_w)."""
    _need_cuda(x, w_q, alpha, bias)
    C = native()
    B, H, W, Cin = x.shape
    cout = Cin
    if x.dtype != FP8 or not C.conv3x3_stream8_supported(H, W, Cin, cout, stride) or w_q.shape[1] != 9 * Cin:
        raise ValueError("conv3x3_stream8: unsupported shape / dtype")
    wf = stream8_weight_frag(w_q, cout) if frag is None else frag
    y = torch.empty(B, H // stride, W // stride, cout, dtype=FP8, device=x.device)
    C.conv3x3_stream8(_ptr(x.contiguous()), _ptr(wf), _ptr(alpha.float().contiguous()), _ptr(bias.float().contiguous()),
                      _ptr(y), _ptr(_zero_page(x.device)), B, H, W, Cin, cout, stride, relu, 1.0 / out_scale,
                      _stream())
    return y


def maxpool2d(x: torch.Tensor, k: int = 3, stride: int = 2, pad: int = 1) -> torch.Tensor:
    _need_cuda(x)
    C = native()
    B, H, W, Ch = x.shape
    Ho, Wo = C.conv_out_dim(H, k, stride, pad), C.conv_out_dim(W, k, stride, pad)
    y = torch.empty(B, Ho, Wo, Ch, device=x.device, dtype=torch.bfloat16)
    C.maxpool2d(_ptr(x.contiguous()), _ptr(y), B, H, W, Ch, k, stride, pad, _stream())
    return y


def avgpool_global(x: torch.Tensor) -> torch.Tensor:
    _need_cuda(x)
    B, H, W, Ch = x.shape
    y = torch.empty(B, Ch, device=x.device, dtype=torch.bfloat16)
    native().avgpool_global(_ptr(x.contiguous()), _ptr(y), B, H * W, Ch, _stream())
    return y


def avgpool_adaptive(x: torch.Tensor, ho: int, wo: int) -> torch.Tensor:
    _need_cuda(x)
    B, H, W, Ch = x.shape
    y = torch.empty(B, ho, wo, Ch, device=x.device, dtype=torch.bfloat16)
    native().avgpool_adaptive(_ptr(x.contiguous()), _ptr(y), B, H, W, Ch, ho, wo, _stream())
    return y


def preprocess_u8(images: torch.Tensor, size: int = 224, pad: int = 0, row_width: int | None = None,
                  paired: bool = False) -> torch.Tensor:
    """u8 [B,H,W,3] -> bf16 packed RGB [B, size+2p, row_width, 3] (resize,
    crop, normalise; zero border; see ``stem_image``). With ``paired`` the
    result is [B, size+2p, row_width/2, 8]: pixel pairs as [r g b r g b 0 0]
    (``paired_image``), the fused stem's input."""
    _need_cuda(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError("preprocess_u8 expects uint8 [B,H,W,3]")
    B, H, W, _ = images.shape
    P = size + 2 * pad
    Wr = row_width or (P + 7) // 8 * 8
    shape = (B, P, Wr // 2, 8) if paired else (B, P, Wr, 3)
    y = torch.empty(*shape, device=images.device, dtype=torch.bfloat16)
    native().preprocess_u8(_ptr(images.contiguous()), _ptr(y), B, H, W, size, pad, Wr, _stream(), paired)
    return y


_TENSOR_DTYPES = {torch.float32: "F32", torch.float16: "F16", torch.bfloat16: "BF16"}


def tensor_input(x: torch.Tensor, size: int | None = None):
    """Check a float image tensor [B,3,S,S] (S = ``size`` if given) in
    float32 / float16 / bfloat16, laid out contiguous or ``torch.channels_last``,
    and return (native dtype, channels_last). Anything else is a ValueError."""
    want = f"float32/float16/bfloat16 [B,3,{size or 'S'},{size or 'S'}], contiguous or channels_last"
    if x.dtype not in _TENSOR_DTYPES or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] \
            or (size is not None and x.shape[2] != size):
        raise ValueError(f"expected {want}, got {x.dtype} {tuple(x.shape)}")
    # the layout is what the strides say: both checks compare strides with the shape
    if x.is_contiguous():
        channels_last = False
    elif x.is_contiguous(memory_format=torch.channels_last):
        channels_last = True
    else:
        raise ValueError(f"expected {want}, got strides {tuple(x.stride())} for shape {tuple(x.shape)}")
    return getattr(native().TensorDType, _TENSOR_DTYPES[x.dtype]), channels_last


def pack_tensor(x: torch.Tensor, pad: int, row_width: int | None = None, paired: bool = False) -> torch.Tensor:
    """float32 / float16 / bfloat16 [B,3,S,S] (contiguous or channels_last)
    -> the bf16 packed RGB image ``preprocess_u8`` writes for the same
    (S, pad, row_width, paired), from the values as given: no resize, no
    normalisation, rounded to bf16 to nearest even, zero border."""
    if not x.is_cuda:
        raise ValueError("pack_tensor needs a CUDA/HIP tensor (no CPU fallback)")
    dt, channels_last = tensor_input(x)
    B, _, S, _ = x.shape
    P = S + 2 * pad
    Wr = row_width or (P + 7) // 8 * 8
    if pad < 0 or Wr % 8 or Wr < P:
        raise ValueError(f"pack_tensor: row_width {Wr} must be a multiple of 8 and >= S + 2 pad = {P} (pad >= 0)")
    shape = (B, P, Wr // 2, 8) if paired else (B, P, Wr, 3)
    y = torch.empty(*shape, device=x.device, dtype=torch.bfloat16)
    if B:
        native().pack_tensor(_ptr(x), dt, channels_last, _ptr(y), B, S, pad, Wr, paired, _stream())
    return y


def paired_image(x_nhwc3: torch.Tensor, pad: int = 3, pairs: int | None = None) -> torch.Tensor:
    """Reference construction of the fused stem's input: the zero-padded
    image [B, H+2p, 2*pairs, 3] regrouped as [B, H+2p, pairs, 8] with
    chunk = [r g b r g b 0 0] of pixels (2q, 2q+1)."""
    B, H, W, _ = x_nhwc3.shape
    pairs = pairs or ((W + 2 * pad + 7) // 8 * 4)
    img = stem_image(x_nhwc3, pad, 2 * pairs)
    out = torch.zeros(B, H + 2 * pad, pairs, 8, dtype=x_nhwc3.dtype, device=x_nhwc3.device)
    out[..., :6] = img.reshape(B, H + 2 * pad, pairs, 6)
    return out


def pack_stem_pool_weight(w: torch.Tensor, scale: torch.Tensor | None = None, device=None) -> torch.Tensor:
    """[64, 3, 7, 7] fp32 -> bf16 [64, 224] for ``stem_conv_pool``:
    k = kh*32 + q*8 + e with kw = 2q + e//3, c = e%3 (e < 6, kw < 7)."""
    cout, cin, kh, kw = w.shape
    if (cout, cin, kh, kw) != (64, 3, 7, 7):
        raise ValueError("stem_conv_pool packs a [64, 3, 7, 7] weight")
    w = w.float()
    if scale is not None:
        w = w * scale.float().view(-1, 1, 1, 1)
    wk = torch.zeros(64, 7, 8, 3)  # [n, kh, kw (8 slots), c]
    wk[:, :, :7] = w.permute(0, 2, 3, 1)
    out = torch.zeros(64, 7, 4, 8)
    out[..., :6] = wk.reshape(64, 7, 4, 6)
    out = out.reshape(64, 224).to(torch.bfloat16)
    return out.to(device) if device is not None else out


def stem_dense_cell(j: int, fq: int) -> tuple[int, int, bool]:
    """(kernel row dy, window dword u, zero-weight pad) that lane group fq
    reads in dword slot j of the dense-K stem: kernels.h stem_dense_cell."""
    if j < 15:
        return 2 * (j // 5) + (fq & 1), 2 * (j % 5) + (fq >> 1), False
    hp, m = 2 * (j - 15) + (fq >> 1), fq & 1
    if hp < 3:
        return 2 * hp + m, 10, False
    if hp < 6:
        return (5 if m else 6), hp - 3, m == 1
    return 6, 3 + 2 * (hp - 6) + m, False


def pack_stem_dense_weight(w: torch.Tensor, scale: torch.Tensor | None = None, device=None) -> torch.Tensor:
    """[64, 3, 7, 7] fp32 -> bf16 [64, 160] in the dense-K order of the
    one-image-per-workgroup stem (stem_pool.hip V & 2): K index k = 32 s +
    8 fq + 2 i + h holds element 2 u + h of kernel row dy's 22-element window
    (kw-major rgb + 1 zero slot), (dy, u) = stem_dense_cell(4 s + i, fq);
    pad slots and element 21 are zero."""
    cout, cin, kh, kw = w.shape
    if (cout, cin, kh, kw) != (64, 3, 7, 7):
        raise ValueError("stem_conv_pool packs a [64, 3, 7, 7] weight")
    w = w.float()
    if scale is not None:
        w = w * scale.float().view(-1, 1, 1, 1)
    win = torch.zeros(64, 7, 22)
    win[:, :, :21] = w.permute(0, 2, 3, 1).reshape(64, 7, 21)  # [n, kh, kw*3 + c]
    out = torch.zeros(64, 160)
    for k in range(160):
        s, fq, i, h = k // 32, (k % 32) // 8, (k % 8) // 2, k % 2
        dy, u, pad = stem_dense_cell(4 * s + i, fq)
        if not pad:
            out[:, k] = win[:, dy, 2 * u + h]
    out = out.to(torch.bfloat16)
    return out.to(device) if device is not None else out


def stem_conv_pool(x_paired: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, size: int = 224,
                   strip: int | None = None) -> torch.Tensor:
    """Fused conv7x7/s2 + bias + ReLU + maxpool3x3/s2/p1 on the paired image
    (``preprocess_u8(..., pad=3, paired=True)``). Returns [B, size/4, size/4, 64]."""
    _need_cuda(x_paired, w_packed, bias)
    C = native()
    B, P, Wq, eight = x_paired.shape
    if eight != 8 or P != size + 6:
        raise ValueError("stem_conv_pool expects a paired [B, size+6, Wq, 8] image")
    ph = size // 4
    if strip is None:
        strip = C.stem_pool_pick_strip(B, ph, torch.cuda.get_device_properties(x_paired.device).multi_processor_count)
    y = torch.empty(B, ph, ph, 64, device=x_paired.device, dtype=torch.bfloat16)
    C.stem_conv_pool(_ptr(x_paired.contiguous()), _ptr(w_packed.contiguous()), _ptr(bias.float().contiguous()),
                     _ptr(y), B, size, Wq, strip, _stream())
    return y


def stem_conv_pool_u8(images: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor,
                      strip: int | None = None, w_dense: torch.Tensor | None = None) -> torch.Tensor:
    """The fused stem with the preprocess fused too: u8 [B, S, S, 3] images
    (already at the model size) -> [B, S/4, S/4, 64]. Same values as
    ``stem_conv_pool(preprocess_u8(images, S, 3, paired=True), ...)`` (up to
    fp32 summation order with ``w_dense``: pack_stem_dense_weight of the same
    weights, which the one-image-per-workgroup kernel then uses)."""
    _need_cuda(images, w_packed, bias)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or images.shape[1] != images.shape[2]:
        raise ValueError("stem_conv_pool_u8 expects uint8 [B, S, S, 3]")
    C = native()
    B, S = images.shape[0], images.shape[1]
    ph = S // 4
    if strip is None:
        strip = C.stem_pool_u8_pick_strip(B, ph, torch.cuda.get_device_properties(images.device).multi_processor_count)
    y = torch.empty(B, ph, ph, 64, device=images.device, dtype=torch.bfloat16)
    if w_dense is not None:
        _need_cuda(w_dense)
        if w_dense.shape != (64, 160) or w_dense.dtype != torch.bfloat16 or not w_dense.is_contiguous():
            raise ValueError("w_dense must be pack_stem_dense_weight's contiguous bf16 [64, 160]")
    C.stem_conv_pool_u8(_ptr(images.contiguous()), _ptr(w_packed.contiguous()), _ptr(bias.float().contiguous()),
                        _ptr(y), B, S, strip, _stream(), _ptr(w_dense) if w_dense is not None else 0)
    return y


def pack_alex_stem_weight(w: torch.Tensor, scale: torch.Tensor | None = None, device=None) -> torch.Tensor:
    """[64, 3, 11, 11] fp32 -> bf16 [64, ALEX_STEM_K] for ``alex_stem``: weight
    (n, c, kh, kw) at k = alex_stem_k(kh, kw, c) = (6 kh + kw // 2) * 8 +
    3 (kw % 2) + c (the paired-chunk order of alex_stem.hip), zeros elsewhere."""
    C = native()
    cout, cin, kh, kw = w.shape
    if (cout, cin, kh, kw) != (64, 3, 11, 11):
        raise ValueError("alex_stem packs a [64, 3, 11, 11] weight")
    w = w.float()
    if scale is not None:
        w = w * scale.float().view(-1, 1, 1, 1)
    k = torch.tensor([[[C.alex_stem_k(i, j, c) for j in range(kw)] for i in range(kh)] for c in range(cin)])
    out = torch.zeros(cout, C.ALEX_STEM_K)
    out[:, k.reshape(-1)] = w.reshape(cout, -1)
    out = out.to(torch.bfloat16)
    return out.to(device) if device is not None else out


def alex_stem(images: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """AlexNet features.0-2 in one kernel (alex_stem.hip): u8 [B, 224, 224, 3]
    -> ImageNet normalisation (``preprocess_u8``'s values) -> conv 11x11/s4/p2 +
    bias -> ReLU -> maxpool 3x3/s2 -> bf16 [B, 27, 27, 64]. w:
    ``pack_alex_stem_weight``'s bf16 [64, ALEX_STEM_K]."""
    _need_cuda(images, w, bias)
    C = native()
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or images.shape[1] != images.shape[2] \
            or not C.alex_stem_supported(images.shape[1]):
        raise ValueError("alex_stem expects uint8 [B, 224, 224, 3]")
    if tuple(w.shape) != (64, C.ALEX_STEM_K) or w.dtype != torch.bfloat16 or not w.is_contiguous():
        raise ValueError("alex_stem: w must be pack_alex_stem_weight's contiguous bf16 [64, ALEX_STEM_K]")
    if bias.numel() < 64:
        raise ValueError("alex_stem: bias holds 64 values")
    B = images.shape[0]
    y = torch.empty(B, 27, 27, 64, device=images.device, dtype=torch.bfloat16)
    C.alex_stem_u8(_ptr(images.contiguous()), _ptr(w), _ptr(bias.float().contiguous()), _ptr(y), B, _stream())
    return y


def conv5x5_27(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, pool: bool = False) -> torch.Tensor:
    """AlexNet features.3 (conv_direct.hip): relu(conv 5x5/s1/p2 + bias) on bf16
    [B, 27, 27, 64] -> [B, 27, 27, 192]; with ``pool`` the following 3x3/s2
    max-pool is fused and [B, 13, 13, 192] returned instead. w_packed: conv2d
    packed weights [>= 192, 1600]."""
    _need_cuda(x, w_packed, bias)
    C = native()
    B, H, W, Cin = x.shape
    Cout = 192
    if x.dtype != torch.bfloat16 or not C.conv5x5_27_supported(H, W, Cin, Cout, 2) or w_packed.shape[0] < Cout \
            or w_packed.shape[1] != 25 * Cin or w_packed.dtype != torch.bfloat16 or bias.numel() < Cout:
        raise ValueError("conv5x5_27: unsupported shape")
    wf = stream_weight_frag(w_packed, Cout)
    y = torch.empty((B, 13, 13, Cout) if pool else (B, H, W, Cout), dtype=x.dtype, device=x.device)
    C.conv5x5_27(_ptr(x.contiguous()), _ptr(wf), _ptr(bias.float().contiguous()), _ptr(y), _ptr(_zero_page(x.device)),
                 B, _stream(), _ptr(y) if pool else 0)
    return y


def conv3x3_13(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, relu: bool, pool: bool = False) -> torch.Tensor:
    """AlexNet features.6 / .8 / .10 (conv_direct.hip): relu?(conv 3x3/s1/p1 +
    bias) on bf16 [B, 13, 13, Cin] for (Cin, Cout) = (192, 384), (384, 256),
    (256, 256). With ``pool`` (256 -> 256 with ReLU only) the following 3x3/s2
    max-pool is fused and [B, 6, 6, 256] returned instead. w_packed: conv2d
    packed weights [Cout, 9 Cin]."""
    _need_cuda(x, w_packed, bias)
    C = native()
    B, H, W, Cin = x.shape
    Cout = w_packed.shape[0]
    if x.dtype != torch.bfloat16 or not C.conv3x3_13_supported(H, W, Cin, Cout) or w_packed.shape[1] != 9 * Cin \
            or w_packed.dtype != torch.bfloat16 or bias.numel() < Cout:
        raise ValueError("conv3x3_13: unsupported shape")
    if pool and (not relu or not C.conv3x3_13_pool_supported(Cin, Cout)):
        raise ValueError("conv3x3_13: the fused max-pool needs ReLU and Cin = Cout = 256")
    wf = stream_weight_frag(w_packed, Cout)
    y = torch.empty((B, 6, 6, Cout) if pool else (B, H, W, Cout), dtype=x.dtype, device=x.device)
    C.conv3x3_13(_ptr(x.contiguous()), _ptr(wf), _ptr(bias.float().contiguous()), _ptr(y), _ptr(_zero_page(x.device)),
                 B, Cin, Cout, relu, _stream(), _ptr(y) if pool else 0)
    return y


def fc_small(x: torch.Tensor, w_packed: torch.Tensor, n: int, bias: torch.Tensor, relu: bool = False,
             out_f32: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """Fully connected layer at B <= 16 rows (fc_small.hip): act(x . w[n] +
    bias[n]). x bf16 [B, K] with unit column stride (its row stride may exceed
    K: a column slice of a wider activation), K % 32 == 0; w_packed bf16
    [Npad, ldw] with ldw >= K and Npad >= n rounded up to 16. Returns [B, n]
    bf16 (fp32 with out_f32), written into ``out[:B, :n]`` if given."""
    _need_cuda(x, w_packed, bias, out)
    C = native()
    if x.dim() != 2 or w_packed.dim() != 2 or x.dtype != torch.bfloat16 or w_packed.dtype != torch.bfloat16:
        raise ValueError("fc_small expects bf16 x [B, K] and w_packed [Npad, ldw]")
    B, K = x.shape
    npad, ldw = w_packed.shape
    if B == 0 or x.stride(1) != 1 or not w_packed.is_contiguous():
        raise ValueError("fc_small: x needs rows and unit column stride, w_packed must be contiguous")
    ldx = x.stride(0) if B > 1 else max(x.stride(0), K)
    if not C.fc_small_supported(B, K, ldx, ldw) or n < 1 or npad < (n + 15) // 16 * 16 or bias.numel() < n \
            or x.data_ptr() % 16:
        raise ValueError("fc_small: unsupported shape")
    dt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty(B, n, device=x.device, dtype=dt)
    elif out.dim() != 2 or out.dtype != dt or out.shape[0] < B or out.shape[1] < n or out.stride(1) != 1 \
            or out.stride(0) < n:
        raise ValueError("fc_small: out must be a [>= B, >= n] tensor of the output type with unit column stride")
    C.fc_small(_ptr(x), ldx, _ptr(w_packed), ldw, _ptr(bias.float().contiguous()), _ptr(out), out.stride(0), out_f32,
               B, K, n, npad, relu, _stream())
    return out[:B, :n]


_HEAD_WS: dict = {}


def _head_ws(device: torch.device, batch: int) -> torch.Tensor:
    """Per-device head workspace (partials + group counters), zeroed once at
    allocation (the kernel re-arms its counters) and reused across calls."""
    t = _HEAD_WS.get(device.index)
    if t is None or t.numel() < native().head_ws_bytes(batch):
        if t is not None:
            torch.cuda.synchronize(device)
        t = _HEAD_WS[device.index] = torch.zeros(native().head_ws_bytes(max(batch, 256)), dtype=torch.uint8,
                                                 device=device)
    return t


def head(x: torch.Tensor, w_packed: torch.Tensor, n: int, bias: torch.Tensor, pooled: bool = False,
         in_fp8_scale: float | None = None, splits: int = 0):
    """The classifier head in one launch (head.hip): global average pool of
    bf16 x [B, HW, C] (or [B, H, W, C]; e4m3 dequantised by ``in_fp8_scale``,
    C >= 2048) + fc + bias + softmax + top-1. With ``pooled`` x is the already
    pooled bf16 [B, C] (16 images per workgroup) and ``splits`` > 0 overrides
    the number of class splits. w_packed: bf16 [Npad, ldw], ldw >= C. Returns
    (logits fp32 [B, n], idx int32 [B], prob fp32 [B])."""
    _need_cuda(x, w_packed, bias)
    C = native()
    fp8 = in_fp8_scale is not None
    if pooled:
        if fp8 or x.dim() != 2 or x.dtype != torch.bfloat16:
            raise ValueError("head: a pooled input is bf16 [B, C]")
        B, Ch = x.shape
        HW = 1
    else:
        if x.dim() not in (3, 4) or x.dtype != (FP8 if fp8 else torch.bfloat16):
            raise ValueError("head expects bf16 (e4m3 with in_fp8_scale) [B, HW, C]")
        if splits:
            raise ValueError("head: splits applies to a pooled input only")
        B, Ch = x.shape[0], x.shape[-1]
        HW = x.numel() // max(B * Ch, 1)
    if w_packed.dim() != 2 or w_packed.dtype != torch.bfloat16 or not w_packed.is_contiguous():
        raise ValueError("head: w_packed must be contiguous bf16 [Npad, ldw]")
    npad, ldw = w_packed.shape
    if B < 1 or HW < 1 or n < 1 or not C.head_supported(Ch, n, ldw, npad) or bias.numel() < n or splits < 0 \
            or (fp8 and Ch < 2048):
        raise ValueError("head: unsupported shape")
    bias = bias.float().contiguous()
    if bias.numel() < npad:
        bias = torch.nn.functional.pad(bias, (0, npad - bias.numel()))
    ws = _head_ws(x.device, B)
    logits = torch.empty(B, n, device=x.device, dtype=torch.float32)
    idx = torch.empty(B, device=x.device, dtype=torch.int32)
    prob = torch.empty(B, device=x.device, dtype=torch.float32)
    cus = torch.cuda.get_device_properties(x.device).multi_processor_count
    if pooled:
        C.head_pooled(_ptr(x.contiguous()), _ptr(w_packed), _ptr(bias), B, Ch, n, ldw, npad, _ptr(logits), _ptr(idx),
                      _ptr(prob), _ptr(ws), ws.numel(), cus, _stream(), ns=splits)
    else:
        C.head_fused(_ptr(x.contiguous()), _ptr(w_packed), _ptr(bias), B, HW, Ch, n, ldw, npad, _ptr(logits),
                     _ptr(idx), _ptr(prob), _ptr(ws), ws.numel(), cus, _stream(), in_fp8=fp8,
                     scale=float(in_fp8_scale) if fp8 else 1.0)
    return logits, idx, prob


def softmax_top1(logits: torch.Tensor, n: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    _need_cuda(logits)
    if logits.dtype != torch.float32:
        raise ValueError("softmax_top1 expects fp32 logits")
    B, ld = logits.shape
    n = ld if n is None else n
    idx = torch.empty(B, device=logits.device, dtype=torch.int32)
    prob = torch.empty(B, device=logits.device, dtype=torch.float32)
    native().softmax_top1(_ptr(logits.contiguous()), B, n, ld, _ptr(idx), _ptr(prob), _stream())
    return idx, prob


def softmax_topk(logits: torch.Tensor, k: int, n: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """The k largest of the first n columns of fp32 logits [B, ld], per row:
    (idx int32 [B, k], prob f32 [B, k]) in descending order, equal logits by
    ascending class; prob is the softmax over those n columns. Column 0 is
    bit-equal to ``softmax_top1``. 1 <= k <= min(n, MAX_TOPK)."""
    _need_cuda(logits)
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError("softmax_topk expects 2-D fp32 logits")
    B, ld = logits.shape
    n = ld if n is None else n
    C = native()
    if not 1 <= n <= ld:
        raise ValueError(f"softmax_topk: n = {n} outside 1..{ld}")
    if not isinstance(k, int) or not 1 <= k <= min(n, C.MAX_TOPK):
        raise ValueError(f"softmax_topk: k = {k} outside 1..min(n = {n}, {C.MAX_TOPK})")
    idx = torch.empty(B, k, device=logits.device, dtype=torch.int32)
    prob = torch.empty(B, k, device=logits.device, dtype=torch.float32)
    C.softmax_topk(_ptr(logits.contiguous()), B, n, ld, k, _ptr(idx), _ptr(prob), _stream())
    return idx, prob


def embed_rows(x: torch.Tensor, normalize: bool = False, scale: float | None = None,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """The feature rows of bf16 ``x`` [B,C], or the global average of bf16 /
    e4m3 (uint8 or float8_e4m3fn, value = e4m3 * ``scale``) ``x`` [B,HW,C]
    exactly as ``avgpool_global`` rounds it to bf16, as fp32 [B,C];
    ``normalize``: every row divided by max(its L2 norm, 1e-12), like
    ``F.normalize`` (csrc/kernels/embed.hip). C % 8 == 0, C <= 8192. ``out``:
    a contiguous fp32 [B,C] tensor on x's device to write instead of a new one."""
    _need_cuda(x)
    fp8 = x.dtype in (torch.uint8, FP8)
    if not fp8 and x.dtype != torch.bfloat16:
        raise ValueError(f"embed_rows expects bf16 or e4m3 (uint8) rows, got {x.dtype}")
    if x.dim() not in (2, 3) or (fp8 and x.dim() != 3):
        raise ValueError(f"embed_rows expects bf16 [B,C] / [B,HW,C] or e4m3 [B,HW,C], got {tuple(x.shape)}")
    if fp8 and scale is None:
        raise ValueError("embed_rows: an e4m3 input needs its scale")
    if not fp8 and scale is not None:
        raise ValueError("embed_rows: scale goes with an e4m3 input")
    B, C = x.shape[0], x.shape[-1]
    HW = x.shape[1] if x.dim() == 3 else 1
    nat = native()
    if not nat.embed_rows_supported(HW, C) or (fp8 and HW == 1):
        raise ValueError(f"embed_rows: needs HW >= 1 (> 1 for e4m3), C % 8 == 0 and C <= 8192, got HW={HW} C={C}")
    x = x.contiguous()
    if out is None:
        out = torch.empty(B, C, device=x.device, dtype=torch.float32)
    elif (out.device != x.device or out.dtype != torch.float32 or tuple(out.shape) != (B, C)
          or not out.is_contiguous()):
        raise ValueError(f"embed_rows: out must be contiguous float32 [{B},{C}] on {x.device}")
    nat.embed_rows(_ptr(x), _ptr(out), B, HW, C, fp8, float(scale) if fp8 else 1.0, bool(normalize), _stream())
    return out


# ---------------------------------------------------------------- nearest-neighbour search
_SIM_WS: dict = {}


def _sim_ws(device: torch.device, nbytes: int) -> torch.Tensor:
    """Per-device search workspace, grown on demand (no initial contents needed)."""
    t = _SIM_WS.get(device.index)
    if t is None or t.numel() < nbytes:
        if t is not None:
            torch.cuda.synchronize(device)
        t = _SIM_WS[device.index] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return t


def query_rows(q: torch.Tensor, dim: int | None, device, what: str):
    """Check search queries: contiguous float32 / bfloat16 [B, dim] on ``device``. Returns the native dtype."""
    if q.dtype not in (torch.float32, torch.bfloat16) or q.dim() != 2 or (dim is not None and q.shape[1] != dim) \
            or q.device != device or not q.is_contiguous():
        raise ValueError(f"{what}: expected contiguous float32 / bfloat16 [B,{dim if dim is not None else 'D'}] on "
                         f"{device}, got {q.dtype} {tuple(q.shape)} (strides {tuple(q.stride())}) on {q.device}")
    return getattr(native().TensorDType, _TENSOR_DTYPES[q.dtype])


def topk_out(out, B: int, k: int, device, what: str):
    """The (idx int32 [B,k], score float32 [B,k]) pair of a search: ``out`` checked, or new tensors."""
    if out is None:
        return (torch.empty(B, k, dtype=torch.int32, device=device),
                torch.empty(B, k, dtype=torch.float32, device=device))
    idx, score = out
    for t, dt in ((idx, torch.int32), (score, torch.float32)):
        if t.device != device or t.dtype != dt or tuple(t.shape) != (B, k) or not t.is_contiguous():
            raise ValueError(f"{what}: out expects contiguous {dt} [{B},{k}] on {device}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    return idx, score


def sim_topk(queries: torch.Tensor, gallery: torch.Tensor, k: int, q_scale: torch.Tensor | None = None,
             g_scale: torch.Tensor | None = None, out=None, slices: int | None = None,
             g_label: torch.Tensor | None = None, q_want: torch.Tensor | None = None):
    """The k gallery rows nearest to each query (csrc/kernels/sim_topk.hip):
    (idx int32 [B,k], score f32 [B,k]), score(b, n) = (sum_d bf16(q[b,d])
    g[n,d]) q_scale[b] g_scale[n] in descending order, equal scores by
    ascending n. queries: float32 (rounded to bf16) or bfloat16 [B,D];
    gallery: bfloat16 [N,D], D % 32 == 0, 32 <= D <= 4096; the scales:
    float32 [B] / [N] or None (1). 1 <= k <= min(N, MAX_TOPK). ``out``: the
    (idx, score) pair to write; ``slices``: how many runs of whole 128-row
    tiles the gallery is cut into (default: about one per CU) - the answer's
    bits do not depend on it.

    The row filter: ``g_label`` int32 [N], row n is a candidate only if
    g_label[n] >= 0 (negative: a removed row); ``q_want`` int32 [B], only with
    g_label: query b accepts only rows labelled q_want[b] where that is >= 0,
    any live row otherwise. A query with fewer than k candidates gets idx =
    -1, score = -inf at the ranks left over, after the real ones. Without
    g_label: the unfiltered kernel, as before."""
    _need_cuda(queries, gallery, q_scale, g_scale, g_label, q_want)
    C = native()
    dev = gallery.device
    if gallery.dtype != torch.bfloat16 or gallery.dim() != 2 or not gallery.is_contiguous():
        raise ValueError(f"sim_topk: gallery must be contiguous bfloat16 [N,D], got {gallery.dtype} "
                         f"{tuple(gallery.shape)}")
    N, D = gallery.shape
    if not C.sim_topk_supported(D):
        raise ValueError(f"sim_topk: needs D % 32 == 0 and 32 <= D <= 4096, got D = {D}")
    qdt, B, slices, cus, idx, score = _sim_args("sim_topk", queries, N, D, dev, k, q_scale, g_scale, out, slices,
                                                g_label, q_want)
    if B == 0:
        return idx, score
    ws = _sim_ws(dev, C.sim_topk_ws_bytes(B, k, slices))
    C.sim_topk(_ptr(queries), qdt, _ptr(q_scale), _ptr(gallery), _ptr(g_scale), B, N, D, k, _ptr(idx), _ptr(score),
               _ptr(ws), ws.numel(), cus, _stream(), slices=slices, g_label=_ptr(g_label), q_want=_ptr(q_want))
    return idx, score


def _sim_args(what, queries, N, D, dev, k, q_scale, g_scale, out, slices, g_label, q_want):
    """The checks sim_topk and sim_topk8 share, once the gallery's own are done:
    (query dtype, B, slices, CUs, idx, score)."""
    C = native()
    qdt = query_rows(queries, D, dev, what)
    B = queries.shape[0]
    if not isinstance(k, int) or not 1 <= k <= min(N, C.MAX_TOPK):
        raise ValueError(f"{what}: k = {k} outside 1..min(N = {N}, {C.MAX_TOPK})")
    for t, n, name in ((q_scale, B, "q_scale"), (g_scale, N, "g_scale")):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (n,) or t.device != dev
                              or not t.is_contiguous()):
            raise ValueError(f"{what}: {name} must be contiguous float32 [{n}] on {dev}")
    if q_want is not None and g_label is None:
        raise ValueError(f"{what}: q_want needs g_label")
    for t, n, name in ((g_label, N, "g_label"), (q_want, B, "q_want")):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (n,) or t.device != dev
                              or not t.is_contiguous()):
            raise ValueError(f"{what}: {name} must be contiguous int32 [{n}] on {dev}")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if slices is None:
        slices = C.sim_topk_slices(B, N, cus)
    elif not isinstance(slices, int) or not 1 <= slices <= C.sim_topk_max_slices(N):
        raise ValueError(f"{what}: slices = {slices} outside 1..{C.sim_topk_max_slices(N)}")
    idx, score = topk_out(out, B, k, dev, what)
    return qdt, B, slices, cus, idx, score


def sim_topk8(queries: torch.Tensor, gallery: torch.Tensor, g_scale: torch.Tensor, k: int, metric: str = "cosine",
              out=None, slices: int | None = None, g_label: torch.Tensor | None = None,
              q_want: torch.Tensor | None = None):
    """``sim_topk`` over an e4m3 gallery on the block-scaled fp8 MFMA.
    gallery: float8_e4m3fn codes [N,D] and g_scale float32 [N], as
    ``gallery_pack8(rows, metric)`` returns them; D % 128 == 0, 128 <= D <=
    4096. queries: float32 or bfloat16 [B,D], quantised by the same rule on
    the way in. score(b, n) = ((sum_d cq[b,d] cg[n,d]) q_scale[b]) g_scale[n]:
    "dot": the dot product of the dequantised vectors; "cosine": the codes'
    cosine. k, ``out``, ``slices``, ``g_label`` and ``q_want`` as for
    ``sim_topk``; the answer's bits do not depend on the slice count."""
    _need_cuda(queries, gallery, g_scale, g_label, q_want)
    C = native()
    dev = gallery.device
    if metric not in ("cosine", "dot"):
        raise ValueError(f"sim_topk8: metric is 'cosine' or 'dot', got {metric!r}")
    if gallery.dtype != torch.float8_e4m3fn or gallery.dim() != 2 or not gallery.is_contiguous():
        raise ValueError(f"sim_topk8: gallery must be contiguous float8_e4m3fn [N,D], got {gallery.dtype} "
                         f"{tuple(gallery.shape)}")
    N, D = gallery.shape
    if not C.sim_topk8_supported(D):
        raise ValueError(f"sim_topk8: needs D % 128 == 0 and 128 <= D <= 4096, got D = {D}")
    if g_scale is None:
        raise ValueError("sim_topk8: an e4m3 gallery needs its g_scale")
    qdt, B, slices, cus, idx, score = _sim_args("sim_topk8", queries, N, D, dev, k, None, g_scale, out, slices,
                                                g_label, q_want)
    if B == 0:
        return idx, score
    ws = _sim_ws(dev, C.sim_topk8_ws_bytes(B, k, slices))
    C.sim_topk8(_ptr(queries), qdt, _ptr(gallery), _ptr(g_scale), metric == "cosine", B, N, D, k, _ptr(idx),
                _ptr(score), _ptr(ws), ws.numel(), cus, _stream(), slices=slices, g_label=_ptr(g_label),
                q_want=_ptr(q_want))
    return idx, score


def gallery_pack8(rows: torch.Tensor, metric: str = "cosine"):
    """float32 or bfloat16 rows [M,D] -> (codes float8_e4m3fn [M,D], scale
    float32 [M]), as an e4m3 gallery stores them. Per row: amax = max |v|, e
    the largest integer with amax 2^e <= 448 (clamped to +-126; 0 for a zero
    row), codes = e4m3(v 2^e) to nearest even; scale = 2^-e ("dot") or 1 /
    max(sqrt(sum codes^2), 1e-12) ("cosine"). D % 128 == 0, 128 <= D <= 4096."""
    _need_cuda(rows)
    if metric not in ("cosine", "dot"):
        raise ValueError(f"gallery_pack8: metric is 'cosine' or 'dot', got {metric!r}")
    if rows.dtype not in (torch.float32, torch.bfloat16) or rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError(f"gallery_pack8 expects contiguous float32 / bfloat16 [M,D], got {rows.dtype} "
                         f"{tuple(rows.shape)}")
    M, D = rows.shape
    C = native()
    if not C.sim_topk8_supported(D):
        raise ValueError(f"gallery_pack8: needs D % 128 == 0 and 128 <= D <= 4096, got D = {D}")
    codes = torch.empty(M, D, dtype=torch.float8_e4m3fn, device=rows.device)
    scale = torch.empty(M, dtype=torch.float32, device=rows.device)
    C.gallery_pack8(_ptr(rows), getattr(C.TensorDType, _TENSOR_DTYPES[rows.dtype]), _ptr(codes), _ptr(scale),
                    metric == "cosine", M, D, _stream())
    return codes, scale


def knn_vote(idx: torch.Tensor, score: torch.Tensor, g_label: torch.Tensor, weighted: bool = False, out=None):
    """The k-NN vote over a search's answer (csrc/kernels/knn_vote.hip):
    (label int32 [B], share f32 [B]). idx int32 / score float32 [B,k], k <=
    MAX_TOPK; g_label int32 [N]. Rank j votes iff 0 <= idx[b,j] < N, with
    label g_label[idx[b,j]] and weight 1 or, ``weighted``, max(score[b,j], 0).
    A label's total is the fp32 sum of its ranks' weights in ascending rank
    order; the largest total wins, equal totals by the best rank; share = that
    total / the fp32 sum of all voting weights (0 if that is 0). No voter:
    (-1, 0). ``out``: the (label, share) pair to write."""
    _need_cuda(idx, score, g_label)
    dev = idx.device
    C = native()
    if idx.dtype != torch.int32 or idx.dim() != 2 or not idx.is_contiguous() or not 1 <= idx.shape[1] <= C.MAX_TOPK:
        raise ValueError(f"knn_vote: idx must be contiguous int32 [B,k], k in 1..{C.MAX_TOPK}, got {idx.dtype} "
                         f"{tuple(idx.shape)}")
    B, k = idx.shape
    if score.dtype != torch.float32 or tuple(score.shape) != (B, k) or score.device != dev \
            or not score.is_contiguous():
        raise ValueError(f"knn_vote: score must be contiguous float32 [{B},{k}] on {dev}")
    if g_label.dtype != torch.int32 or g_label.dim() != 1 or g_label.shape[0] < 1 or g_label.device != dev \
            or not g_label.is_contiguous():
        raise ValueError(f"knn_vote: g_label must be contiguous int32 [N >= 1] on {dev}")
    label, share = vote_out(out, B, dev, "knn_vote")
    if B:
        C.knn_vote(_ptr(idx), _ptr(score), _ptr(g_label), g_label.shape[0], B, k, bool(weighted), _ptr(label),
                   _ptr(share), _stream())
    return label, share


def vote_out(out, B: int, device, what: str):
    """The (label int32 [B], share float32 [B]) pair of a vote: ``out`` checked, or new tensors."""
    if out is None:
        return (torch.empty(B, dtype=torch.int32, device=device), torch.empty(B, dtype=torch.float32, device=device))
    label, share = out
    for t, dt in ((label, torch.int32), (share, torch.float32)):
        if t.device != device or t.dtype != dt or tuple(t.shape) != (B,) or not t.is_contiguous():
            raise ValueError(f"{what}: out expects contiguous {dt} [{B}] on {device}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    return label, share


def gallery_pack(rows: torch.Tensor, with_norms: bool = False):
    """float32 rows [M,D] -> bfloat16 [M,D] (nearest even), as a gallery stores
    them; with_norms: also float32 [M], 1 / max(sqrt(sum v^2), 1e-12) of the
    rounded values v (the cosine metric's scales). D % 8 == 0, D <= 8192."""
    _need_cuda(rows)
    if rows.dtype != torch.float32 or rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError(f"gallery_pack expects contiguous float32 [M,D], got {rows.dtype} {tuple(rows.shape)}")
    M, D = rows.shape
    if D < 8 or D % 8 or D > 8192:
        raise ValueError(f"gallery_pack: needs D % 8 == 0 and 8 <= D <= 8192, got D = {D}")
    g = torch.empty(M, D, dtype=torch.bfloat16, device=rows.device)
    inv = torch.empty(M, dtype=torch.float32, device=rows.device) if with_norms else None
    native().gallery_pack(_ptr(rows), _ptr(g), _ptr(inv), M, D, _stream())
    return (g, inv) if with_norms else g


# ---------------------------------------------------------------- split JPEG decode
def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


def _upload(parts, device) -> tuple[torch.Tensor, list[int]]:
    """numpy arrays -> ONE pinned staging buffer (each part 256-byte aligned)
    -> one host-to-device copy on the current stream. Returns the device
    buffer and the parts' byte offsets."""
    import numpy as np
    offs, total = [], 0
    for p in parts:
        offs.append(total)
        total += _align(p.nbytes)
    stage = torch.empty(max(total, 256), dtype=torch.uint8, pin_memory=True)
    view = stage.numpy()
    for p, o in zip(parts, offs):
        view[o:o + p.nbytes] = np.ascontiguousarray(p).reshape(-1).view(np.uint8)
    return stage.to(device, non_blocking=True), offs


def resize_u8_ragged(images, size: int = 224, antialias: bool = False) -> torch.Tensor:
    """Differently sized u8 [H, W, 3] images on one GPU -> one u8 batch
    [B, size, size, 3] in one launch (csrc/kernels/resize.hip): short side ->
    size, long side floor(size * long / short), centre crop, bilinear with
    half-pixel centres, rounded to u8; a size x size image is copied. With
    ``antialias`` the triangle filter is stretched by max(scale, 1) per axis
    (torch's ``antialias=True``), so shrinking averages the source instead of
    sampling four pixels per output; ``native().resize_u8_host`` is the host
    reference of both."""
    import numpy as np
    images = list(images)
    if not images:
        raise ValueError("resize_u8_ragged: no images")
    if not isinstance(size, int) or size <= 0 or size % 4 != 0:
        raise ValueError(f"resize_u8_ragged: size = {size} is not a positive multiple of 4")
    _need_cuda(*images)
    dev = images[0].device
    for t in images:
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"resize_u8_ragged expects uint8 [H, W, 3] images, got {t.dtype} {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError("resize_u8_ragged expects contiguous images")
        if t.device != dev:
            raise ValueError("resize_u8_ragged expects every image on the same device")
    C = native()
    descs = np.zeros(len(images), dtype=np.dtype([("ptr", "<u8"), ("h", "<i4"), ("w", "<i4")]))
    assert descs.dtype.itemsize == C.IMAGE_DESC_BYTES
    for i, t in enumerate(images):
        descs[i] = (t.data_ptr(), t.shape[0], t.shape[1])
    with torch.cuda.device(dev):
        d, _ = _upload([descs], dev)
        out = torch.empty(len(images), size, size, 3, device=dev, dtype=torch.uint8)
        C.resize_u8_ragged(_ptr(d), _ptr(out), len(images), size, _stream(), bool(antialias))
    return out


def jpeg_idct(coeffs, qt, bw: int, bh: int, device="cuda") -> torch.Tensor:
    """Stage 1 of the GPU JPEG finish on one plane: quantised int16
    coefficients [bh][bw][64] (natural order) and a quantisation table (64
    values, natural order) -> the u8 plane [8 bh, 8 bw] (dequantise, AAN
    inverse DCT in fp32, + 128, round half up, clamp)."""
    import numpy as np
    nat = native()
    dev = coeffs.device if isinstance(coeffs, torch.Tensor) else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("dmlc.ops kernels need CUDA/HIP tensors (no CPU fallback)")
    co = torch.as_tensor(coeffs).to(device=dev, dtype=torch.int16).contiguous().reshape(-1)
    if co.numel() != bw * bh * 64:
        raise ValueError("jpeg_idct: coeffs must hold bw * bh * 64 values")
    layout = {"width": 8 * bw, "height": 8 * bh, "hmax": 1, "vmax": 1,
              "comps": [{"h": 1, "v": 1, "bw": bw, "bh": bh, "qt": np.asarray(qt, dtype=np.uint16).reshape(64)}]}
    descs, tables, ncoef, pbytes = nat.jpeg_gpu_plan([layout], [0])
    with torch.cuda.device(dev):
        d, (od, ot) = _upload([descs, tables], dev)
        plane = torch.empty(8 * bh, 8 * bw, dtype=torch.uint8, device=dev)
        nat.jpeg_idct_planes(descs, d.data_ptr() + od, d.data_ptr() + ot, tables.shape[0], co.data_ptr(), ncoef,
                             plane.data_ptr(), pbytes, _stream())
    return plane


def jpeg_planes_to_rgb(planes, layout: dict, device="cuda") -> torch.Tensor:
    """Stage 2 of the GPU JPEG finish on one image: its u8 component planes
    ([8 bh, 8 bw] each) -> u8 [height, width, 3]; bit-identical to
    ``native().ycc_planes_to_rgb`` on the same planes."""
    nat = native()
    if not nat.jpeg_gpu_supported(layout):
        raise ValueError("jpeg_planes_to_rgb: unsupported layout")
    ps = [torch.as_tensor(p) for p in planes]
    dev = ps[0].device if ps[0].is_cuda else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("dmlc.ops kernels need CUDA/HIP tensors (no CPU fallback)")
    comps = layout["comps"]
    if len(ps) != len(comps):
        raise ValueError("jpeg_planes_to_rgb: one plane per component")
    for p, c in zip(ps, comps):
        if p.dtype != torch.uint8 or tuple(p.shape) != (8 * c["bh"], 8 * c["bw"]):
            raise ValueError("jpeg_planes_to_rgb: planes are uint8 [8 bh, 8 bw]")
    H, W = layout["height"], layout["width"]
    with torch.cuda.device(dev):
        scratch = torch.cat([p.to(dev).reshape(-1) for p in ps])
        rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        descs, _, _, pbytes = nat.jpeg_gpu_plan([layout], [rgb.data_ptr()])
        d, (od,) = _upload([descs], dev)
        nat.jpeg_planes_to_rgb(descs, d.data_ptr() + od, scratch.data_ptr(), pbytes, _stream())
    return rgb


def jpeg_decode(blobs, device="cuda") -> list[torch.Tensor]:
    """JPEG files (bytes) -> u8 HWC tensors on ``device``: Huffman decoding on
    the host, then ONE upload (descriptors, tables and coefficients of the
    whole list) and ONE launch pair (inverse DCT, colour) for the whole ragged
    list. An image whose layout the GPU path does not handle
    (``native().jpeg_gpu_supported``) is decoded by the CPU decoder and
    uploaded as pixels."""
    import numpy as np
    nat = native()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("dmlc.ops kernels need CUDA/HIP tensors (no CPU fallback)")
    out: list = [None] * len(blobs)
    which, layouts, coefs = [], [], []
    for i, b in enumerate(blobs):
        b = bytes(b)
        lay, co = nat.decode_jpeg_coeffs(b)
        if nat.jpeg_gpu_supported(lay):
            which.append(i)
            layouts.append(lay)
            coefs.append(co)
        else:
            out[i] = torch.from_numpy(nat.decode_jpeg(b)).to(dev)
    if not which:
        return out
    with torch.cuda.device(dev):
        offs, total = [], 0
        for lay in layouts:
            offs.append(total)
            total += _align(lay["height"] * lay["width"] * 3)
        rgb = torch.empty(total, dtype=torch.uint8, device=dev)
        descs, tables, ncoef, pbytes = nat.jpeg_gpu_plan(layouts, [rgb.data_ptr() + o for o in offs])
        d, (od, ot, oc) = _upload([descs, tables, np.concatenate(coefs)], dev)
        planes = torch.empty(pbytes, dtype=torch.uint8, device=dev)
        nat.jpeg_idct_planes(descs, d.data_ptr() + od, d.data_ptr() + ot, tables.shape[0], d.data_ptr() + oc, ncoef,
                             planes.data_ptr(), pbytes, _stream())
        nat.jpeg_planes_to_rgb(descs, d.data_ptr() + od, planes.data_ptr(), pbytes, _stream())
    for i, lay, o in zip(which, layouts, offs):
        h, w = lay["height"], lay["width"]
        out[i] = rgb[o:o + h * w * 3].view(h, w, 3)
    return out

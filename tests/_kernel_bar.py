"""The element-wise bar of the op tests (test_kernels_fused_gpu.py,
test_kernels_resnet_gpu.py, test_kernels_resnet50_gpu.py,
test_kernels_gemm_gpu.py, test_kernel_bar_cpu.py): a kernel's output against
the float64 result on the same bf16-rounded operands.

A rounding argument, not a measurement. A bf16-output conv or fc with K
products per output, exact bf16 x bf16 products and fp32 accumulation in any
order satisfies, to first order,

    |got - ref64| <= u |ref64| + (K - 1) 2^-24 sum|terms|

(the output rounding plus the summation), u being bf16's unit roundoff. The
bar is

    |got - ref64| <= 2^-8 |ref64| + K 2^-23 mag,

mag being the same operation on |x|, |w|, |bias| (+ |res|). fp32 outputs drop
the first term. bf16 keeps 8 significant bits, so u = 2^-8 (half an ulp of a
value just above a power of two), not 2^-9: the bar's rounding term is the
first-order worst case itself and only its summation term is doubled. A
correct kernel therefore comes close to 1 on outputs just above a power of
two (the float64 reference rounded to bf16 reaches 0.75 against itself,
test_kernel_bar_cpu.py). ReLU is 1-Lipschitz and keeps zero, so the bar holds
with the ReLU applied to ref64.

A fused max-pool (`assert_close_pooled`): max is monotone and 1-Lipschitz and
commutes with the (monotone) bf16 rounding, so the pooled output meets the
window maximum of the bar against the pool of the *unrounded* reference.
Against the pool of the bf16-rounded reference that bar is missed by correct
arithmetic (an fp32 conv rounded to bf16 and pooled reaches 1.7): the
reference's own rounding, another 2^-8 |ref64|, is not inside it, the two
roundings can fall on different sides of a tie and then differ by a whole
bf16 ulp. That comparison is kept too, with that term added.

Roundings beyond that derivation, each stated where it is used:
 * the classifier heads round the pooled vector to bf16 before the fc: the
   logits' bar is (2^-8 + C 2^-23) mag (`head_bound`);
 * conv3x3_stream's fused average pool sums the bf16-rounded activations (as
   the unfused avgpool kernel reads them) and rounds the mean to bf16: the
   mean of the activations' own bars (their rounding is the first 2^-8), plus
   2^-8 |pool| for the pooled value's rounding, plus 49 2^-23 mean|y| for the
   49-term fp32 sum (`avgpool_bound`);
 * conv3x3_block keeps its intermediate t = relu(conv1(x) + b1) in LDS as
   bf16 (`chained`). The kernel's fp32 value of t lies within s1 = K 2^-23 mag1
   of the float64 v, rounding is monotone, and t >= 0, so the stored t lies
   element-wise in [bf16r(relu(v - s1)), bf16r(relu(v + s1))]: where the two
   ends agree (most elements) t is known exactly, elsewhere it is one of two
   neighbouring bf16 values. With delta the width of that interval the
   reference relu(conv2(bf16r(v)) + b2 + x) is off by at most conv2(delta,
   |w2|) on that account, which is added to conv2's own bar. `chain` is the
   same argument for n stages (bottleneck56: an e4m3 conv1 with a per-channel
   alpha, a 3x3, and an e4m3 conv3 with a residual; bottleneck56_head);
 * an e4m3 output relu(v) inv_scale (`e4m3_bound`): e4m3 keeps 4 significant
   bits, unit roundoff 2^-4 of the value by the argument above; below its
   smallest normal 2^-6 the values step by 2^-9, half a step is 2^-10. In the
   output's own units the bar is K 2^-23 mag inv_scale + max(2^-4 |ref|
   inv_scale, 2^-10), for values that stay below e4m3's largest, 448.

A fused max-pool with padding pads with -inf, which after a ReLU selects what
a zero padding selects (every window holds a value >= 0).

Measured on an MI355X: the worst |err| / bar of any kernel is 0.99 (the 1x1
downsample outputs, K = 64; alex_stem 0.95), per kernel in the docstrings of
test_kernels_fused_gpu.py, test_kernels_resnet_gpu.py and
test_kernels_resnet50_gpu.py. The general matrix family
(test_kernels_gemm_gpu.py): conv_igemm 0.94 over its 11 tiles, 0.44 with
split-K, 0.77 persistent, 0.97 the stem, 0.91 / 0.94 / 0.59 the e4m3 in / out,
bf16 in / e4m3 out and e4m3 in / bf16 out forms; conv_bigtile 0.82 with slabs,
0.81 persistent; fc_gemm 0.90; every fp32 output below 0.01.

Next to the bar every test keeps the project's relative-L2 bar for bf16
outputs (5e-3), and a negative control: a reference with one realistic kernel
fault (`fault_*`) must be rejected by the same bar.
"""
import torch
import torch.nn.functional as F

EPS_OUT = 2.0 ** -8   # bf16's unit roundoff
EPS_SUM = 2.0 ** -23  # twice fp32's unit roundoff, per product
L2_BF16 = 5e-3


def bf16r(t):
    """Round to bf16, back in float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def conv_ref(x, w, bias, stride=1, pad=0, res=None):
    """float64 conv + bias (+ res) of NCHW x (bf16-representable values) and
    its magnitude sum: (ref64, mag), both NCHW float64."""
    x, w, bias = x.double(), w.double(), bias.double()
    ref = F.conv2d(x, w, bias, stride, pad)
    mag = F.conv2d(x.abs(), w.abs(), bias.abs(), stride, pad)
    if res is not None:
        ref = ref + res.double()
        mag = mag + res.double().abs()
    return ref, mag


def fc_ref(x, w, bias):
    """float64 x . w^T + bias and its magnitude sum."""
    x, w, bias = x.double(), w.double(), bias.double()
    return x @ w.t() + bias, x.abs() @ w.abs().t() + bias.abs()


def bound(ref, mag, K, out_bf16=True):
    b = K * EPS_SUM * mag
    return b + EPS_OUT * ref.abs() if out_bf16 else b


def head_bound(mag, C):
    """fp32 logits of a head whose pooled input is rounded to bf16 (2^-8 each)
    before C products per class."""
    return (EPS_OUT + C * EPS_SUM) * mag


def avgpool_bound(y, y_bound, HW=49):
    """conv3x3_stream's pool over the HW pixels (dim 1 of [B, HW, C]) of the
    activation y (float64, before its bf16 rounding) whose own bar is y_bound."""
    return y_bound.mean(1) + EPS_OUT * y.mean(1).abs() + HW * EPS_SUM * y.abs().mean(1)


def maxpool(t, k=3, s=2, pad=0):
    """NCHW max-pool, `pad` rows / columns of -inf on every side."""
    return F.max_pool2d(t, k, s, pad)


E4M3_EPS = 2.0 ** -4        # e4m3's unit roundoff (4 significant bits)
E4M3_HALF_STEP = 2.0 ** -10  # half the step of its subnormals (below 2^-6)
E4M3_MAX = 448.0


def e4m3_bound(ref, mag, K, inv_scale):
    """e4m3(ref inv_scale) in the output's units: ref (ReLU applied) and mag
    as for `bound`. See the module text."""
    v = ref.abs() * inv_scale
    assert float(v.max()) < E4M3_MAX, "the scale saturates e4m3"
    return K * EPS_SUM * mag * inv_scale + (E4M3_EPS * v).clamp_min(E4M3_HALF_STEP)


def chain(x, stages, alpha=None, res=None, e4m3_inv=None):
    """n chained stride-1 convs with bf16 intermediates (conv3x3_block,
    bottleneck56, bottleneck56_head). stages: [(w, bias, K, pad), ...], the
    last one's output bf16, or e4m3 with `e4m3_inv` (its inv_scale); every
    other stage i leaves t_i = bf16r(relu(v_i)). Returns (ref64 before the
    last ReLU, its bar, [delta_i], [t_i]), NCHW float64.

    The interval argument of the module text, stage by stage: the kernel's
    fp32 value of t_i lies within s_i of the float64 v_i, s_i the conv's own
    summation slack K_i 2^-23 mag_i plus what the uncertainty of its input
    can move it, conv_i(delta_{i-1}, |w_i|); so the stored t_i lies in
    [bf16r(relu(v_i - s_i)), bf16r(relu(v_i + s_i))], of width delta_i, which
    goes through the next conv's |w| into that conv's slack and, at the last
    stage, onto its bar (times inv_scale for an e4m3 output).

    alpha (per output channel, with an e4m3 first input: conv1 of
    bottleneck56): the first stage is relu(acc alpha + bias), one fp32 fma on
    the fp32 sum of exact products, inside K 2^-23 mag with mag = conv(|x|,
    |w|) |alpha| + |bias|. res (NCHW float64, already scaled): the last
    stage's residual, in its mag."""
    t, delta, deltas, ts = x, None, [], []
    for i, (w, bias, K, pad) in enumerate(stages):
        last = i == len(stages) - 1
        r = res if last else None
        if i == 0 and alpha is not None:
            a, b = alpha.double().view(1, -1, 1, 1), bias.double().view(1, -1, 1, 1)
            v = F.conv2d(t.double(), w.double(), None, 1, pad) * a + b
            mag = F.conv2d(t.double().abs(), w.double().abs(), None, 1, pad) * a.abs() + b.abs()
            if r is not None:
                v, mag = v + r.double(), mag + r.double().abs()
        else:
            v, mag = conv_ref(t, w, bias, 1, pad, res=r)
        if last:
            if e4m3_inv is None:
                bnd = bound(torch.relu(v), mag, K)
                if delta is not None:
                    bnd = bnd + F.conv2d(delta, w.double().abs(), None, 1, pad)
            else:
                bnd = e4m3_bound(torch.relu(v), mag, K, e4m3_inv)
                if delta is not None:
                    bnd = bnd + F.conv2d(delta, w.double().abs(), None, 1, pad) * e4m3_inv
            return v, bnd, deltas, ts
        s = K * EPS_SUM * mag
        if delta is not None:
            s = s + F.conv2d(delta, w.double().abs(), None, 1, pad)
        lo, hi = bf16r(torch.relu(v - s)), bf16r(torch.relu(v + s))
        t = bf16r(torch.relu(v))
        assert bool((lo <= t).all()) and bool((t <= hi).all())
        delta = hi - lo
        deltas.append(delta)
        ts.append(t)


def chained(x, w1, b1, w2, b2, K=576, pad=1):
    """Two chained 3x3 convs with a bf16 intermediate and the input as the
    residual (conv3x3_block): (ref64 before the last ReLU, its bar, delta,
    the intermediate bf16r(v)), NCHW float64. See the module text."""
    ref, bnd, deltas, ts = chain(x, [(w1, b1, K, pad), (w2, b2, K, pad)], res=x)
    return ref, bnd, deltas[0], ts[0]


def block_operands(B, seed):
    """conv3x3_block's test operands (the GPU test and the CPU check of its
    controls share them): x, w1, b1, w2, b2, NCHW float64, bf16 values."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 64, 56, 56, generator=g).bfloat16().double()
    w1 = (torch.randn(64, 64, 3, 3, generator=g) / 24).bfloat16().double()
    w2 = (torch.randn(64, 64, 3, 3, generator=g) / 24).bfloat16().double()
    b1 = (torch.randn(64, generator=g) * 0.1).float().double()
    b2 = (torch.randn(64, generator=g) * 0.1).float().double()
    return x, w1, b1, w2, b2


def worst(got, ref, bnd):
    """(largest |got - ref| / bnd, relative L2). Where the bar is 0 (an exact
    zero is expected) any difference counts as infinite."""
    got, ref = got.double(), ref.double()
    d = (got - ref).abs()
    ratio = torch.where(bnd > 0, d / bnd.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")),
                                                                       torch.zeros_like(d)))
    return ratio.max().item(), (d.norm() / ref.norm().clamp_min(1e-300)).item()


def assert_close(got, ref, bnd, what, l2=L2_BF16):
    assert got.shape == ref.shape == bnd.shape, (what, got.shape, ref.shape, bnd.shape)
    assert bool(torch.isfinite(got.double()).all()), what
    ratio, rel = worst(got, ref, bnd)
    print(f"{what}: worst |err|/bound {ratio:.3f}, rel L2 {rel:.2e}")
    assert ratio <= 1.0, f"{what}: |err| / bound = {ratio}"
    assert rel < l2, f"{what}: relative L2 {rel}"
    return ratio, rel


def assert_close_pooled(got, r, bnd, what, k=3, s=2, pad=0):
    """A fused max-pool's output against the NCHW reference r (float64, ReLU
    applied, not rounded) and its bar before the pool: see the module text."""
    out = assert_close(got, maxpool(r, k, s, pad), maxpool(bnd, k, s, pad), what)
    assert_close(got, maxpool(bf16r(r), k, s, pad), maxpool(bnd + EPS_OUT * r.abs(), k, s, pad),
                 what + " (bf16-rounded reference)")
    return out


def assert_rejects(got, wrong_ref, bnd, what):
    """The negative control: `got` must miss the bar against a faulty reference."""
    ratio, _ = worst(got, wrong_ref, bnd)
    print(f"{what}: control |err|/bound {ratio:.1f}")
    assert ratio > 1.0, f"{what}: the bar does not see this fault ({ratio})"


# ---------------------------------------------------------------- modelled kernel faults (NCHW float64 references)
def fault_border_taps(ref, x, w, pad, at=0):
    """An off-by-one border test: output row `at + pad` loses its kh = 0 taps
    (the ones on image row `at`; at = 0: next to the top padding, at > 0: a
    seam between two workgroups' strips)."""
    lost = F.conv2d(x.double()[:, :, at:at + 1, :], w.double()[:, :, 0:1, :], None, 1, (0, pad))
    out = ref.clone()
    out[:, :, at + pad:at + pad + 1, :] -= lost
    return out


def fault_border_taps_s2(ref, x, w, at=0):
    """The same for a 3x3/s2/p1 conv: the output row whose kh = 1 taps lie on
    the even image row `at` loses them (at = 0: output row 0, whose kh = 0
    taps are the top padding)."""
    lost = F.conv2d(x.double()[:, :, at:at + 1, :], w.double()[:, :, 1:2, :], None, (1, 2), (0, 1))
    out = ref.clone()
    out[:, :, at // 2:at // 2 + 1, :] -= lost
    return out


def fault_chunk_swap(ref, b=0, h=None, w=None, chunk=1, width=8):
    """One 8-channel chunk (16 B of bf16; width = 16: 16 B of e4m3) of one
    pixel swapped with its right neighbour's (a swizzle slip)."""
    h = ref.shape[2] // 2 if h is None else h
    w = ref.shape[3] // 2 if w is None else w
    out = ref.clone()
    c = slice(width * chunk, width * chunk + width)
    out[b, c, h, w], out[b, c, h, w + 1] = ref[b, c, h, w + 1], ref[b, c, h, w]
    return out


def fault_chunk_swap_at_max(ref, b=0, chunk=1):
    """The same slip at the pixel that holds the chunk's first channel's
    largest value (for pooled outputs: a window's maximum surely changes)."""
    H, W = ref.shape[2], ref.shape[3]
    h, w = divmod(int(ref[b, 8 * chunk].argmax()), W)
    return fault_chunk_swap(ref, b, h, w if w + 1 < W else w - 1, chunk)


def fault_batch_shift(ref):
    """Image b's result at b + 1 (batch of at least 2)."""
    return torch.roll(ref, 1, 0)


def fault_ring_row(ref, x, w, row, ring, stride=1, pad=1):
    """A ring slot read before its row landed: output row `row` takes its last
    kernel row's input (image row stride * row + k - 1 - pad, the newest one it
    needs) from the image row `ring` rows earlier, which held that slot."""
    k = w.shape[2]
    r = stride * row + k - 1 - pad
    assert ring <= r < x.shape[2], (row, r, ring)
    x, w = x.double(), w.double()
    stale = x[:, :, r - ring:r - ring + 1, :] - x[:, :, r:r + 1, :]
    out = ref.clone()
    out[:, :, row:row + 1, :] += F.conv2d(stale, w[:, :, k - 1:k, :], None, (1, stride), (0, pad))
    return out


def fault_strided_parity(ref, x, w, col, pad):
    """A stride-2 conv whose output column `col` reads input column 2 c + 1
    where it should read 2 c (every tap one column to the right)."""
    x = x.double()
    xs = torch.zeros_like(x)
    xs[..., :-1] = x[..., 1:]
    out = ref.clone()
    out[..., col] += F.conv2d(xs - x, w.double(), None, 2, pad)[..., col]
    return out


def kernel_const(hip_file, name):
    """The integer `constexpr int <name> = <n>;` of csrc/kernels/<hip_file>:
    the modelled faults take ring lengths from the kernels' own constants."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc", "kernels", hip_file)
    with open(path) as f:
        m = re.search(r"constexpr int %s = (\d+);" % re.escape(name), f.read())
    assert m, (hip_file, name)
    return int(m.group(1))


def block_controls(x, w1, b1, w2, b2, ring):
    """conv3x3_block's faulty references (before the last ReLU), each fault
    on conv1's output (the producer) and on conv2's (the consumer)."""
    B = x.shape[0]
    v, _ = conv_ref(x, w1, b1, 1, 1)
    t = bf16r(torch.relu(v))
    ref, _ = conv_ref(t, w2, b2, 1, 1, res=x)

    def faults(r, xin, w):
        out = [("border taps", fault_border_taps(r, xin, w, 1)),
               ("chunk swap", fault_chunk_swap(r, b=B - 1, h=r.shape[2] - 1, w=r.shape[3] - 2, chunk=3)),
               ("ring row", fault_ring_row(r, xin, w, 4 * (ring // 4) + 1, ring))]
        if B > 1:
            out.append(("batch shift", fault_batch_shift(r)))
        return out

    out = [("conv1 " + n, conv_ref(bf16r(torch.relu(vw)), w2, b2, 1, 1, res=x)[0]) for n, vw in faults(v, x, w1)]
    return out + [("conv2 " + n, r) for n, r in faults(ref, t, w2)]


# ---------------------------------------------------------------- bottleneck56 / bottleneck56_head (ResNet50 layer1)
def f32(v):
    """A Python float rounded to fp32 (a kernel argument), as a float."""
    return float(torch.tensor(v, dtype=torch.float32))


def e4m3_weights(w):
    """ops.pack_conv_weight_fp8's quantisation of [Cout, Cin, 1, 1] weights:
    (codes as float64 [Cout, Cin, 1, 1], fp32 per-row scales [Cout])."""
    w2 = w.float().reshape(w.shape[0], -1)
    s = (w2.abs().amax(1) / E4M3_MAX).clamp_min(1e-12)
    q = (w2 / s[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.double().reshape(w.shape), s


def bottleneck_operands(B, seed):
    """bottleneck56's random operands (the GPU bar test and the CPU check of
    its controls share them), NCHW float64: x, w1 e4m3 codes (x >= 0 like the
    post-ReLU activation it is), a1 = s_x s_w1 (fp32), bf16 w2 / w3, fp32
    biases (b1 with a positive offset: its ReLU is what wrong padding holds),
    and an output scale that is no power of two, chosen so that the largest
    output sits at 400 of e4m3's 448."""
    g = torch.Generator().manual_seed(seed)
    xv = torch.rand(B, 256, 56, 56, generator=g) * 4
    sx = f32(float(xv.max()) / E4M3_MAX)
    o = {"x": (xv / sx).clamp(0, E4M3_MAX).to(torch.float8_e4m3fn).double(), "res_scale": sx}
    o["w1"], s1 = e4m3_weights(torch.randn(64, 256, 1, 1, generator=g) / 32)
    o["a1"] = (sx * s1).float().double()
    o["b1"] = (torch.randn(64, generator=g) * 0.1 + 0.25).float().double()
    o["w2"] = (torch.randn(64, 64, 3, 3, generator=g) / 24).bfloat16().double()
    o["b2"] = (torch.randn(64, generator=g) * 0.1).float().double()
    o["w3"] = (torch.randn(256, 64, 1, 1, generator=g) / 8).bfloat16().double()
    o["b3"] = (torch.randn(256, generator=g) * 0.1).float().double()
    o["out_scale"] = 1.0
    top = float(torch.relu(bottleneck_ref(o)[0]).max())
    o["out_scale"] = top / 400.0
    return o


def bottleneck_last(o):
    """bottleneck56's last stage in the output's units, as the kernel forms
    it (kernels.h): (bf16r(fp32(w3) fp32(inv)), fp32(b3 inv), the residual
    x fp32(res_scale inv)), inv = fp32(1 / out_scale)."""
    inv = torch.tensor(1.0 / o["out_scale"], dtype=torch.float32)
    w3s = bf16r(o["w3"].float() * inv)
    b3s = (o["b3"].float() * inv).double()
    rsi = (torch.tensor(o["res_scale"], dtype=torch.float32) * inv).double()
    return w3s, b3s, o["x"] * rsi


def bottleneck_ref(o, bar=True):
    """(ref64 in the output's units before the last ReLU, its bar, deltas,
    [t1, t2]) of bottleneck56. bar = False (operands that saturate e4m3: the
    exact-integer ones): the second item is not the output's bar."""
    w3s, b3s, res = bottleneck_last(o)
    return chain(o["x"], [(o["w1"], o["b1"], 256, 0), (o["w2"], o["b2"], 576, 1), (w3s, b3s, 64, 0)],
                 alpha=o["a1"], res=res, e4m3_inv=1.0 if bar else None)


def head_operands(B, seed):
    """bottleneck56_head's random operands, NCHW float64 (bf16 values)."""
    g = torch.Generator().manual_seed(seed)
    o = {"x": torch.relu(torch.randn(B, 64, 56, 56, generator=g)).bfloat16().double()}
    o["w1"] = (torch.randn(64, 64, 1, 1, generator=g) / 8).bfloat16().double()
    o["b1"] = (torch.randn(64, generator=g) * 0.1 + 0.25).float().double()
    o["w2"] = (torch.randn(64, 64, 3, 3, generator=g) / 24).bfloat16().double()
    o["b2"] = (torch.randn(64, generator=g) * 0.1).float().double()
    return o


def head_ref(o):
    return chain(o["x"], [(o["w1"], o["b1"], 64, 0), (o["w2"], o["b2"], 576, 1)])


def fault_t1_padding(v2, t1, w2, b1, rows):
    """conv2 (3x3 / p1 on t1) whose padding rows (rows = True: t1 rows -1 and
    H) or columns (-1 and W) hold bf16r(relu(b1)), a conv1 of zeros, where
    they should hold 0."""
    fill = bf16r(torch.relu(b1.double())).view(1, -1, 1, 1)
    tp = F.pad(t1, (1, 1, 1, 1))
    extra = torch.zeros_like(tp)
    if rows:
        extra[:, :, 0, 1:-1] = fill[..., 0]
        extra[:, :, -1, 1:-1] = fill[..., 0]
    else:
        extra[:, :, 1:-1, 0] = fill[..., 0]
        extra[:, :, 1:-1, -1] = fill[..., 0]
    return v2 + F.conv2d(extra, w2.double(), None, 1, 0)


def conv2_faults(v2, t1, w2, b1, ring, seam=28):
    """The faults of the bottleneck kernels' 3x3 conv on the t1 ring, as
    faulty float64 conv2 outputs (before its ReLU): border taps next to the
    top padding and at a step seam (t1 row `seam` = 4k, the last row the
    previous step's conv1 wrote), padding that is not zero, a ring row stale
    by `ring`."""
    return [("border taps row 0", fault_border_taps(v2, t1, w2, 1)),
            ("border taps seam", fault_border_taps(v2, t1, w2, 1, at=seam)),
            ("t1 padding rows", fault_t1_padding(v2, t1, w2, b1, True)),
            ("t1 padding columns", fault_t1_padding(v2, t1, w2, b1, False)),
            ("ring row", fault_ring_row(v2, t1, w2, 4 * (ring // 4) + 1, ring))]


def bottleneck_controls(o, ring):
    """bottleneck56's faulty references in the output's units (before the
    last ReLU): conv2's faults carried through conv3, and the faults of the
    output itself."""
    w3s, b3s, res = bottleneck_last(o)
    ref, _, _, (t1, t2) = bottleneck_ref(o, bar=False)
    v2, _ = conv_ref(t1, o["w2"], o["b2"], 1, 1)
    out = [(n, conv_ref(bf16r(torch.relu(w)), w3s, b3s, 1, 0, res=res)[0])
           for n, w in conv2_faults(v2, t1, o["w2"], o["b1"], ring)]
    B = ref.shape[0]
    out.append(("y chunk swap", fault_chunk_swap(ref, b=B - 1, h=55, w=54, chunk=5, width=16)))
    inv = f32(1.0 / o["out_scale"])
    out.append(("residual without res_scale", ref - res + o["x"] * inv))
    if B > 1:
        out.append(("batch shift", fault_batch_shift(ref)))
    return out


def head_controls(o, ring):
    ref, _, _, (t1,) = head_ref(o)
    out = conv2_faults(ref, t1, o["w2"], o["b1"], ring)
    if ref.shape[0] > 1:
        out.append(("batch shift", fault_batch_shift(ref)))
    return out


def _sparse(cout, cin, k, entries, g):
    """[cout, cin, k, k] float64 with `entries` non-zero integer weights per
    output channel, walking the input channels and the taps in turn so that
    every one of them is used."""
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64)
    vals = torch.tensor([1.0, -1.0, 2.0, 1.0, -2.0])
    for n in range(cout):
        for j in range(entries):
            e = n * entries + j
            tap = (e + n // 9) % (k * k)
            w[n, (e * 5) % cin, tap // k, tap % k] = vals[int(torch.randint(0, 5, (1,), generator=g))]
    return w


def bottleneck_exact_operands(B, seed=0):
    """Small dyadic integers for which every fp32 value inside bottleneck56
    is exact, so its output bytes are known exactly: x codes 1..3, sparse
    integer weights, a1 in {1, 2, 4}, integer biases (b1 up to 6: non-zero t1
    padding shows), res_scale = 4 and 1 / out_scale = 1 / 2 (powers of two);
    t1 <= 54 and t2 <= 256 are integers, exact in bf16. The final values
    include negatives, ties of the e4m3 grid and a few above 448."""
    g = torch.Generator().manual_seed(seed)
    o = {"x": torch.randint(1, 4, (B, 256, 56, 56), generator=g).double(), "res_scale": 4.0, "out_scale": 2.0}
    o["w1"] = _sparse(64, 256, 1, 4, g).sign()
    o["a1"] = torch.tensor([1.0, 2.0, 4.0, 2.0], dtype=torch.float64).repeat(16)
    o["b1"] = torch.randint(-2, 7, (64,), generator=g).double()
    o["w2"] = _sparse(64, 64, 3, 3, g)
    o["b2"] = torch.randint(-8, 9, (64,), generator=g).double()
    o["w3"] = _sparse(256, 64, 1, 3, g) * 2
    o["w3"][::32] = o["w3"][::32].abs() * 8  # (a few values reach past 448)
    o["b3"] = torch.randint(-16, 17, (256,), generator=g).double()
    return o


def head_exact_operands(B, seed=1):
    """The same for bottleneck56_head: x in 0..3, integer t1 and t2 <= 256."""
    g = torch.Generator().manual_seed(seed)
    o = {"x": torch.randint(0, 4, (B, 64, 56, 56), generator=g).double()}
    o["w1"] = _sparse(64, 64, 1, 4, g)
    o["b1"] = torch.randint(-2, 7, (64,), generator=g).double()
    o["w2"] = _sparse(64, 64, 3, 3, g)
    o["b2"] = torch.randint(-8, 9, (64,), generator=g).double()
    return o


def e4m3_bytes(v):
    """relu(v) saturated at 448 and rounded to e4m3 (tests/_e4m3_ref.py's
    rule: torch's fp32 -> float8_e4m3fn conversion, nearest even), as bytes.
    v must be exact in fp32."""
    import _e4m3_ref
    return _e4m3_ref.round_bytes(v.clamp(0, E4M3_MAX))


def fault_ds_missing(ref, x56, wd, b=0, frag=3):
    """The 1x1/s2 downsample's products left out of one 16-pixel fragment
    (pixels 16 frag .. 16 frag + 15 of image b, row-major) of a conv that
    takes the downsample as extra K steps."""
    ds = F.conv2d(x56.double(), wd.double(), None, 2, 0)
    out = ref.clone()
    flat, dsf = out.view(out.shape[0], out.shape[1], -1), ds.reshape(ds.shape[0], ds.shape[1], -1)
    flat[b, :, 16 * frag:16 * frag + 16] -= dsf[b, :, 16 * frag:16 * frag + 16]
    return out


def prob_without_split(logits, lo, hi):
    """Top-1 softmax probability with classes lo..hi-1 left out of the sum (a
    split's partial that never reached the merge)."""
    z = logits.double()
    m = z.max(-1, keepdim=True).values
    e = (z - m).exp()
    e[:, lo:hi] = 0
    return 1.0 / e.sum(-1)


# ---------------------------------------------------------------- conv1x1's block loop (conv1x1.hip), in matrix form
C1_KEYS = [(False, False, False, 1), (False, False, True, 1), (False, False, False, 2), (True, False, False, 1),
           (False, True, False, 1), (False, True, True, 1), (True, True, False, 2), (True, True, False, 1),
           (True, True, True, 1)]  # (in8, out8, residual, stride): the launcher's switch
C1_MSTRIDE = 8  # block stride of a workgroup on a grid of 8 workgroups per channel slice


def c1_forms():
    """(in8, out8, res, stride, rb) for every key and staged row class the
    launcher takes (stride 2 stops at 512-B rows)."""
    return [k + (rb,) for k in C1_KEYS for rb in (128, 256, 512, 1024) if not (k[3] == 2 and rb > 512)]


def c1_operands(nblocks, in8, out8, res, stride, rb, N=256, seed=0, cin2=0):
    """A 1x1 conv over nblocks pixel blocks (64 pixels, 32 for 1-KB rows), one
    block an image: 8x8 outputs (16x16 inputs at stride 2), 4x8 for 1-KB rows.
    x / x2: NHWC float64 (e4m3 codes or bf16 values); X: the [M, K] rows the
    conv reads, in block order; w [N, K]; alpha / bias [N]; r: residual [M, N]
    (e4m3 codes times res_scale, or bf16 values); out_scale puts the largest
    output at 400 (e4m3 output), and is no power of two."""
    g = torch.Generator().manual_seed(seed)
    esz = 1 if in8 else 2
    K = rb // esz
    Cin = K - cin2
    bm = 64 if rb <= 512 else 32
    Ho, Wo = bm // 8, 8
    o = {"in8": in8, "out8": out8, "stride": stride, "bm": bm, "S": 3 if rb <= 256 else 2, "K": K, "N": N,
         "alpha": None, "r": None, "res_scale": 1.0, "x2": None, "out_scale": None}
    shape = (nblocks, stride * Ho, stride * Wo)
    if in8:
        xv = torch.rand(*shape, Cin, generator=g) * 4
        sx = f32(float(xv.max()) / E4M3_MAX)
        o["x"] = (xv / sx).clamp(0, E4M3_MAX).to(torch.float8_e4m3fn).double()
        w, sw = e4m3_weights(torch.randn(N, K, 1, 1, generator=g) / K ** 0.5)
        o["w"], o["alpha"] = w.reshape(N, K), (sx * sw).float().double()
    else:
        o["x"] = torch.randn(*shape, Cin, generator=g).bfloat16().double()
        o["w"] = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().double()
        if cin2:
            o["x2"] = torch.randn(*shape, cin2, generator=g).bfloat16().double()
    o["bias"] = (torch.randn(N, generator=g) * 0.1).float().double()
    X = o["x"][:, ::stride, ::stride].reshape(-1, Cin)
    o["X"] = X if not cin2 else torch.cat([X, o["x2"].reshape(-1, cin2)], 1)
    if res:
        rv = torch.randn(nblocks * bm, N, generator=g)
        if out8:
            o["res_scale"] = f32(float(rv.abs().max()) / E4M3_MAX)
            o["r"] = (rv / o["res_scale"]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).double()
        else:
            o["r"] = rv.bfloat16().double()
    if out8:
        o["out_scale"] = float(torch.relu(c1_ref(o)[0]).max()) / 400.0
    return o


def c1_ref(o, X=None, r=None):
    """(ref64 before the ReLU, mag), [M, N], of `c1_operands` (X / r: a
    control's rows in their place)."""
    X = o["X"] if X is None else X
    r = o["r"] if r is None else r
    v, mag = X @ o["w"].t(), X.abs() @ o["w"].abs().t()
    if o["alpha"] is not None:
        v, mag = v * o["alpha"], mag * o["alpha"].abs()
    v, mag = v + o["bias"], mag + o["bias"].abs()
    if r is not None:
        v, mag = v + r * o["res_scale"], mag + r.abs() * o["res_scale"]
    return v, mag


def c1_bar(o, v, mag):
    """(the expected output in its own units, its bar, the relative-L2 bar)."""
    if o["out8"]:
        inv = f32(1.0 / o["out_scale"])
        return torch.relu(v) * inv, e4m3_bound(torch.relu(v), mag, o["K"], inv), 4e-2
    return torch.relu(v), bound(torch.relu(v), mag, o["K"]), L2_BF16


def _blocks(t, bm):
    return t.reshape(-1, bm, t.shape[-1])


def c1_controls(o):
    """Faulty references of the block loop (before the ReLU): a stage slot
    read before its DMA landed (block j from the rows of block j - S mstride,
    which held the slot), and the residual of the other register set (block
    j +- mstride's)."""
    bm, back = o["bm"], o["S"] * C1_MSTRIDE
    nb = o["X"].shape[0] // bm
    out = []
    if nb > back:
        Xb = _blocks(o["X"], bm).clone()
        Xb[back:] = _blocks(o["X"], bm)[:nb - back]
        out.append(("stale stage slot", c1_ref(o, X=Xb.reshape(o["X"].shape))[0]))
    if o["r"] is not None and nb > C1_MSTRIDE:
        rb_ = _blocks(o["r"], bm)
        rw = torch.cat([rb_[C1_MSTRIDE:], rb_[nb - 2 * C1_MSTRIDE:nb - C1_MSTRIDE]] if nb >= 2 * C1_MSTRIDE
                       else [rb_[C1_MSTRIDE:], rb_[:C1_MSTRIDE]])
        out.append(("residual of the other register set", c1_ref(o, r=rw.reshape(o["r"].shape))[0]))
    return out


def c1_cat_controls(o, cin):
    """Concatenated K: x2's K block read from x, and the two K blocks swapped."""
    X = o["X"]
    return [("x2's K block read from x", c1_ref(o, X=torch.cat([X[:, :cin], X[:, :cin]], 1))[0]),
            ("K blocks swapped", c1_ref(o, X=torch.cat([X[:, cin:], X[:, :cin]], 1))[0])]


def chain_operands(nblocks, seed=0):
    """conv1x1_chain: the expand conv (e4m3 128 -> 512, e4m3 residual) as
    `c1_operands`, and the reduce conv on its output codes (512 -> 128 e4m3):
    w2 codes [128, 512], alpha2 = out_scale s_w2, bias2, out_scale2 (the
    largest y2 at 400, from the float64 y rounded to e4m3)."""
    o = c1_operands(nblocks, True, True, True, 1, 128, N=512, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    w2, s2 = e4m3_weights(torch.randn(128, 512, 1, 1, generator=g) / 512 ** 0.5)
    o["w2"] = w2.reshape(128, 512)
    o["alpha2"] = (f32(o["out_scale"]) * s2).float().double()
    o["bias2"] = (torch.randn(128, generator=g) * 0.1).float().double()
    y = (torch.relu(c1_ref(o)[0]) * f32(1.0 / o["out_scale"])).float().to(torch.float8_e4m3fn).double()
    o["out_scale2"] = float(torch.relu(chain_reduce(o, y)[0]).max()) / 400.0
    return o


def chain_reduce(o, y):
    """(ref64 before the ReLU, mag) of the reduce conv on the y codes [M, 512]."""
    v, mag = y @ o["w2"].t() * o["alpha2"] + o["bias2"], y.abs() @ o["w2"].abs().t() * o["alpha2"].abs() + o["bias2"].abs()
    return v, mag


def chain_reduce_bar(o, y):
    v, mag = chain_reduce(o, y)
    inv = f32(1.0 / o["out_scale2"])
    return torch.relu(v) * inv, e4m3_bound(torch.relu(v), mag, 512, inv)


def chain_controls(o, y):
    """y2 of block j computed from block j - mstride's y (a stale ybuf)."""
    yb = _blocks(y, 64)
    if yb.shape[0] <= C1_MSTRIDE:
        return []
    stale = torch.cat([yb[:C1_MSTRIDE], yb[:-C1_MSTRIDE]]).reshape(y.shape)
    return [("stale ybuf", chain_reduce(o, stale)[0])]


# ---------------------------------------------------------------- the general matrix family
# conv_igemm.hip's tiles 0..10, conv_bigtile.hip's 11 / 12 (slabs) and 13 (persistent): (BM, BN)
GEMM_TILES = {0: (128, 128), 1: (256, 64), 2: (64, 256), 3: (128, 128), 4: (256, 64), 5: (64, 256), 6: (128, 128),
              7: (128, 64), 8: (64, 128), 9: (128, 64), 10: (64, 128), 11: (256, 256), 12: (256, 128), 13: (256, 128)}
L2_E4M3 = 4e-2


def npad(n):
    """conv_igemm.hip's conv_npad."""
    return 64 if n <= 64 else n if n % 64 == 0 else (n + 127) // 128 * 128


def rows(t):
    """NCHW -> the GEMM's [M, N] (m = (b Ho + ho) Wo + wo)."""
    return nhwc(t).reshape(-1, t.shape[1])


def unrows(r, like):
    B, C, H, W = like.shape
    return nchw(r.reshape(B, H, W, C))


def igemm_slices(k_tiles, split_k):
    """K-tile ranges of conv2d_igemm's slices: ceil(k_tiles / split_k) tiles
    each, so fewer slices than asked for when that does not come out even
    (72 K tiles at split_k = 13: 12 slices of 6)."""
    per = -(-k_tiles // max(1, split_k))
    return [(t, min(k_tiles, t + per)) for t in range(0, k_tiles, per)]


def bigtile_slices(k_tiles, splits):
    """conv_bt_kernel's: slice s = K tiles [k_tiles s / splits, k_tiles (s + 1) / splits)."""
    return [(k_tiles * s // splits, k_tiles * (s + 1) // splits) for s in range(splits)]


_GEMM_OPERANDS = {}


def gemm_operands(B, H, W, Cin, Cout, k, stride, pad, res=False, seed=0, exact=False, in8=False, out8=False):
    """A conv of the matrix family, NCHW float64 (made once per argument set
    and shared: do not modify). bf16 values, or with in8 e4m3 codes x >= 0 and
    w with alpha = s_x s_w; res: bf16 values, with out8 e4m3 codes times
    res_scale; out8: out_scale puts the largest output at 400 of 448 and is
    no power of two. Cin = 3: a stem (K = 3 k k).

    exact: integers for which every fp32 partial sum, the bias and residual
    adds and the scalings are exact in any order: x in -3..3 (codes 0..3), 6
    weights of +-1 / +-2 per output channel, alpha in {1, 2, 4}, biases and
    residual in -8..8 (res_scale 4), out_scale 2; |v| <= 160, integers, exact
    in bf16. With out8 every 32nd channel's bias is raised by 2000: those
    outputs saturate at 448."""
    key = (B, H, W, Cin, Cout, k, stride, pad, res, seed, exact, in8, out8)
    if key in _GEMM_OPERANDS:
        return _GEMM_OPERANDS[key]
    g = torch.Generator().manual_seed(seed)
    K = Cin * k * k
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    o = {"stride": stride, "pad": pad, "k": k, "K": K, "N": Cout, "in8": in8, "out8": out8, "alpha": None, "r": None,
         "res_scale": 1.0, "out_scale": None, "bk": 128 if in8 else 64, "stem": Cin == 3}
    if exact:
        o["x"] = torch.randint(0 if in8 else -3, 4, (B, Cin, H, W), generator=g).double()
        o["w"] = _sparse(Cout, Cin, k, 6, g)
        if in8:
            o["alpha"] = torch.tensor([1.0, 2.0, 4.0, 2.0], dtype=torch.float64).repeat(Cout // 4)
        o["bias"] = torch.randint(-8, 9, (Cout,), generator=g).double()
        if out8:
            o["bias"][::32] += 2000
            o["out_scale"] = 2.0
        if res:
            o["r"] = torch.randint(-8, 9, (B, Cout, Ho, Wo), generator=g).double()
            o["res_scale"] = 4.0 if out8 else 1.0
    else:
        if in8:
            xv = torch.rand(B, Cin, H, W, generator=g) * 4
            sx = f32(float(xv.max()) / E4M3_MAX)
            o["x"] = (xv / sx).clamp(0, E4M3_MAX).to(torch.float8_e4m3fn).double()
            o["w"], sw = e4m3_weights(torch.randn(Cout, Cin, k, k, generator=g) / K ** 0.5)
            o["alpha"] = (sx * sw).float().double()
        else:
            o["x"] = torch.randn(B, Cin, H, W, generator=g).bfloat16().double()
            o["w"] = (torch.randn(Cout, Cin, k, k, generator=g) / K ** 0.5).bfloat16().double()
        o["bias"] = (torch.randn(Cout, generator=g) * 0.1).float().double()
        if res:
            rv = torch.randn(B, Cout, Ho, Wo, generator=g)
            if out8:
                o["res_scale"] = f32(float(rv.abs().max()) / E4M3_MAX)
                o["r"] = (rv / o["res_scale"]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).double()
            else:
                o["r"] = rv.bfloat16().double()
        if out8:
            o["out_scale"] = float(torch.relu(gemm_ref(o)[0]).max()) / 400.0
    o["ref"] = gemm_ref(o)
    _GEMM_OPERANDS[key] = o
    return o


def gemm_ref(o):
    """(ref64 before the ReLU, mag), NCHW: conv(x, w) (alpha) + bias (+ r res_scale)."""
    x, w, s, p = o["x"], o["w"], o["stride"], o["pad"]
    v, mag = F.conv2d(x, w, None, s, p), F.conv2d(x.abs(), w.abs(), None, s, p)
    bias = o["bias"].view(1, -1, 1, 1)
    if o["alpha"] is not None:
        a = o["alpha"].view(1, -1, 1, 1)
        v, mag = v * a, mag * a.abs()
    v, mag = v + bias, mag + bias.abs()
    if o["r"] is not None:
        v, mag = v + o["r"] * o["res_scale"], mag + o["r"].abs() * o["res_scale"]
    return v, mag


def gemm_k_range(o, t0, t1):
    """What K tiles t0..t1-1 (o["bk"] wide, k = (kh KW + kw) Cin + c) add to
    the output, NCHW float64."""
    w = o["w"]
    wk = torch.zeros_like(w).permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    lo, hi = t0 * o["bk"], t1 * o["bk"]
    wk[:, lo:hi] = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)[:, lo:hi]
    wk = wk.reshape(w.shape[0], w.shape[2], w.shape[3], w.shape[1]).permute(0, 3, 1, 2)
    v = F.conv2d(o["x"], wk, None, o["stride"], o["pad"])
    return v if o["alpha"] is None else v * o["alpha"].view(1, -1, 1, 1)


def gemm_bar(o, v, mag, out_f32=False):
    """(the expected output in its own units, its bar, the relative-L2 bar)
    of a reference v (before the ReLU) with the operands' mag."""
    if o["out8"]:
        inv = f32(1.0 / o["out_scale"])
        return torch.relu(v) * inv, e4m3_bound(torch.relu(v), mag, o["K"], inv), L2_E4M3
    return torch.relu(v), bound(torch.relu(v), mag, o["K"], out_bf16=not out_f32), L2_BF16


def gemm_rounded(o, v, out_f32=False):
    """The float64 reference rounded to the output type: what an ideal kernel gives."""
    if o["out8"]:
        return (torch.relu(v) * f32(1.0 / o["out_scale"])).float().to(torch.float8_e4m3fn).double()
    return torch.relu(v).float().double() if out_f32 else bf16r(torch.relu(v))


def fault_tail_tile(R, bm):
    """An unclamped row index: the rows of the last, partial M tile ([M, N]
    rows, M % bm of them) take the previous tile's rows at the same offset."""
    M = R.shape[0]
    t = M % bm
    assert t and M > bm, (M, bm)
    out = R.clone()
    out[M - t:] = R[M - t - bm:M - bm]
    return out


def fault_k_tile_missing(R, lost, m0, bm, n0=0, bn=None):
    """One K tile's products (`lost`, [M, N]) left out of the M tile at row
    m0 (and of the N tile at column n0, if bn is given): a stage of the LDS
    ring consumed before it landed, or a slice's last K tile dropped."""
    out = R.clone()
    n1 = R.shape[1] if bn is None else n0 + bn
    out[m0:m0 + bm, n0:n1] -= lost[m0:m0 + bm, n0:n1]
    return out


def fault_slice_missing(R, lost, m0, bm, n0, bn):
    """One split-K slice (`lost`: its products, [M, N]) left out of the
    reduction for the output tile at (m0, n0): a slab that was not handed
    off, or the reduce loop's 8 / 4 / 1 remainder skipping a slice."""
    return fault_k_tile_missing(R, lost, m0, bm, n0, bn)


def fault_pad_columns(R, n_pad, row):
    """Rows of ldo == N with N < Npad: row `row - 1`'s pad columns N..Npad-1
    (zeros: zero weights, zero bias) land on row `row`'s first columns."""
    N = R.shape[1]
    assert n_pad > N and row >= 1
    out = R.clone()
    out[row, :n_pad - N] = 0
    return out


def gemm_controls(o, bm, bn, slices=None):
    """Faulty references (NCHW, before the ReLU) of a conv of the matrix
    family on (bm, bn) tiles with the split-K `slices` (K-tile ranges): a chunk
    swap at the last pixel of the last image, a batch shift, the partial last M
    tile, the last K tile missing from the last full M tile, the last slice
    missing from the tile at (0, last N tile), and pad columns spilling into
    the second M tile's first row."""
    v = o["ref"][0]
    B, N, Ho, Wo = v.shape
    M, R = B * Ho * Wo, rows(v)
    out = [("chunk swap", fault_chunk_swap(v, b=B - 1, h=Ho - 1, w=Wo - 2, chunk=1, width=16 if o["out8"] else 8))]
    if B > 1:
        out.append(("batch shift", fault_batch_shift(v)))
    if M > bm and M % bm:
        out.append(("tail tile", unrows(fault_tail_tile(R, bm), v)))
    if not o["stem"]:
        kt = o["K"] // o["bk"]
        m0 = max(0, M // bm - 1) * bm
        out.append(("K tile missing", unrows(fault_k_tile_missing(R, rows(gemm_k_range(o, kt - 1, kt)), m0, bm), v)))
        if slices is not None and len(slices) > 1:
            n0 = (npad(N) // bn - 1) * bn
            lost = rows(gemm_k_range(o, *slices[-1]))
            out.append(("slice missing", unrows(fault_slice_missing(R, lost, 0, bm, n0, bn), v)))
    if N < npad(N) and M > bm:
        out.append(("pad columns", unrows(fault_pad_columns(R, npad(N), bm), v)))
    return out


# The cases of tests/test_kernels_gemm_gpu.py (test_kernel_bar_cpu.py checks the
# bar and every control on the same operands without a GPU).
# (name, (B, H, W, Cin, Cout, k, stride, pad), res, tile, split_k, max_blocks, out_f32)
_BASE = (3, 13, 13, 64)
IGEMM_CASES = [("base tile %d" % t, _BASE + (512 if GEMM_TILES[t][1] == 256 else 256, 3, 1, 1), True, t, 1, 0, False)
               for t in range(11)]
IGEMM_CASES += [
    ("stride 2 tile 0", (3, 13, 13, 128, 256, 3, 2, 1), False, 0, 1, 0, False),
    ("stride 2 tile 7", (3, 13, 13, 128, 256, 3, 2, 1), False, 7, 1, 0, False),
    ("5x5 tile 1", (2, 27, 27, 64, 192, 5, 1, 2), False, 1, 1, 0, False),
    ("1x1 tile 0", (3, 14, 14, 512, 256, 1, 1, 0), False, 0, 1, 0, False),
    ("1x1 tile 4", (3, 14, 14, 512, 256, 1, 1, 0), True, 4, 1, 0, False),
    ("Cout 100 tile 0", _BASE + (100, 3, 1, 1), True, 0, 1, 0, False),
    ("Cout 100 tile 7", _BASE + (100, 3, 1, 1), True, 7, 1, 0, False),
]
# 72 K tiles: split_k 2 -> 2 slices, 5 -> 5 (15 15 15 15 12), 13 -> 12 of 6 (the reduce's 8- and 4-wide loops),
# 15 -> 15 of 5, the last of 2 (8 + 4 + 3: all three loops), 32 -> 24 of 3
IGEMM_CASES += [("split-K %d tile %d%s" % (s, t, " f32" if f else ""), (1, 7, 7, 512, 512, 3, 1, 1), True, t, s, 0, f)
                for t in (3, 5) for s, f in ((2, False), (5, False), (13, False), (15, False), (32, False), (13, True))]
# tile 2 (BN = 256) cannot take Npad = 384: its case runs at Cout = 512
IGEMM_CASES += [("persistent tile %d" % t, (5, 13, 13, 192, 512 if t == 2 else 384, 3, 1, 1), True, t, 1, 8, False)
                for t in (0, 1, 2, 7, 8)]
IGEMM_EXACT = [c for c in IGEMM_CASES if c[0].startswith("base") or c[0] in ("split-K 13 tile 3", "split-K 15 tile 5",
                                                                            "persistent tile 0")]
STEM_CASES = [(7, 2, 3), (11, 4, 2)]  # (k, stride, pad) at B = 2, hw (57, 61), 64 channels (tile 1)
STEM_HW = (57, 61)

# (name, shape, in8, out8, res, tile[, max_blocks]): conv2d_igemm's six e4m3 instantiations,
# and the e4m3 in / out form on a persistent grid of 8 blocks (21 and 24 tiles)
E4M3_CASES = [
    ("e4m3 in/out persistent 128x128", (5, 13, 13, 256, 384, 3, 1, 1), True, True, True, -1, 8),
    ("e4m3 in/out persistent 256x64", (5, 13, 13, 256, 384, 3, 1, 1), True, True, True, 1, 8),
    ("e4m3 in/out 128x128", (2, 14, 14, 256, 256, 3, 1, 1), True, True, True, -1),
    ("e4m3 in/out 256x64", (2, 14, 14, 256, 192, 3, 1, 1), True, True, True, 1),
    ("bf16 in e4m3 out 128x128", (2, 14, 14, 64, 256, 1, 1, 0), False, True, False, -1),
    ("bf16 in e4m3 out 256x64", (2, 14, 14, 64, 192, 1, 1, 0), False, True, False, 1),
    ("e4m3 in bf16 out 128x128", (2, 14, 14, 256, 256, 3, 1, 1), True, False, True, -1),
    ("e4m3 in bf16 out 256x64", (2, 14, 14, 256, 192, 3, 1, 1), True, False, False, 1),
]

# (name, shape, res, tile, splits or the persistent grid)
_BT = (2, 13, 13, 128)
BIGTILE_CASES = [("cfg 0 splits %d" % s, _BT + (512, 3, 1, 1), True, 11, s) for s in (1, 2, 5)]
BIGTILE_CASES += [("cfg 1 splits %d" % s, _BT + (128, 3, 1, 1), True, 12, s) for s in (1, 2)]
BIGTILE_CASES += [("stride 2 splits 2", (4, 14, 14, 256, 512, 3, 2, 1), False, 11, 2)]
BIGTILE_CASES += [("persistent %s grid %d" % (n, g), sh, True, 13, g)
                  for n, sh in (("28x28", (3, 28, 28, 128, 128, 3, 1, 1)), ("13x13", (5, 13, 13, 192, 384, 3, 1, 1)))
                  for g in (1, 3)]
BIGTILE_EXACT = [c for c in BIGTILE_CASES if c[0] in ("cfg 0 splits 5", "cfg 1 splits 2", "persistent 13x13 grid 1")]


def gemm_case_operands(shape, res, seed, exact=False, in8=False, out8=False):
    return gemm_operands(*shape, res=res, seed=seed, exact=exact, in8=in8, out8=out8)


def case_seed(cases, name):
    """Cases of one shape share their operands (and the float64 reference)."""
    key = [c[1:3] for c in cases if c[0] == name][0]
    return 500 + [c[1:3] for c in cases].index(key)


# ---------------------------------------------------------------- fc_gemm.hip
FC_KB = 64      # K block
FC_RING = 3     # LDS slots
FC_BN = 128     # columns per workgroup
FC_MS, FC_NS, FC_K = (1, 17, 200, 256), (256, 1000), 1024
_FC_OPERANDS = {}


def fc_operands(M, K, N, seed, exact=False):
    """x [M, K], w [N, K], bias [N] float64 (bf16 values; exact: integers as
    for `gemm_operands`), and "ref": (ref64 before the ReLU, mag)."""
    key = (M, K, N, seed, exact)
    if key in _FC_OPERANDS:
        return _FC_OPERANDS[key]
    g = torch.Generator().manual_seed(seed)
    if exact:
        x = torch.randint(-3, 4, (M, K), generator=g).double()
        w = _sparse(N, K, 1, 6, g).reshape(N, K)
        bias = torch.randint(-8, 9, (N,), generator=g).double()
    else:
        x = torch.randn(M, K, generator=g).bfloat16().double()
        w = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16().double()
        bias = (torch.randn(N, generator=g) * 0.1).float().double()
    o = {"x": x, "w": w, "bias": bias, "K": K, "ref": fc_ref(x, w, bias)}
    _FC_OPERANDS[key] = o
    return o


def fc_controls(o, splits):
    """Faulty references [M, N] of fc_gemm: K block 3 of the last slice read
    from block 0's slot (ring distance 3: block 0's rows still there) for the
    first 128 columns, the last slice missing from the last column group, rows
    16..31 taking rows 0..15."""
    x, w, K = o["x"], o["w"], o["K"]
    R = o["ref"][0]
    M, N = R.shape
    per = K // splits
    assert per // FC_KB > FC_RING
    k0 = K - per
    j, i = k0 + FC_RING * FC_KB, k0
    stale = (x[:, i:i + FC_KB] - x[:, j:j + FC_KB]) @ w[:, j:j + FC_KB].t()
    out = [("stale ring slot", fault_k_tile_missing(R, -stale, 0, M, 0, FC_BN))]
    if splits > 1:
        n0 = (N - 1) // FC_BN * FC_BN
        out.append(("slice missing", fault_slice_missing(R, x[:, k0:] @ w[:, k0:].t(), 0, M, n0, FC_BN)))
    if M > 16:
        s = R.clone()
        s[16:min(32, M)] = R[:min(32, M) - 16]
        out.append(("row group shift", s))
    return out

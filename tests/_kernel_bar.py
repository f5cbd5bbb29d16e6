"""The element-wise bar of the op tests (test_kernels_fused_gpu.py,
test_kernels_resnet_gpu.py, test_kernel_bar_cpu.py): a kernel's output against
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
   |w2|) on that account, which is added to conv2's own bar;
 * an e4m3 output relu(v) inv_scale (`e4m3_bound`): e4m3 keeps 4 significant
   bits, unit roundoff 2^-4 of the value by the argument above; below its
   smallest normal 2^-6 the values step by 2^-9, half a step is 2^-10. In the
   output's own units the bar is K 2^-23 mag inv_scale + max(2^-4 |ref|
   inv_scale, 2^-10), for values that stay below e4m3's largest, 448.

A fused max-pool with padding pads with -inf, which after a ReLU selects what
a zero padding selects (every window holds a value >= 0).

Measured on an MI355X: the worst |err| / bar of any kernel is 0.99 (the 1x1
downsample outputs, K = 64; alex_stem 0.95), per kernel in the docstrings of
test_kernels_fused_gpu.py and test_kernels_resnet_gpu.py.

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


def chained(x, w1, b1, w2, b2, K=576, pad=1):
    """Two chained 3x3 convs with a bf16 intermediate and the input as the
    residual (conv3x3_block): (ref64 before the last ReLU, its bar, delta,
    the intermediate bf16r(v)), NCHW float64. See the module text."""
    v, mag1 = conv_ref(x, w1, b1, 1, pad)
    s1 = K * EPS_SUM * mag1
    lo, hi = bf16r(torch.relu(v - s1)), bf16r(torch.relu(v + s1))
    t = bf16r(torch.relu(v))
    assert bool((lo <= t).all()) and bool((t <= hi).all())
    delta = hi - lo
    ref, mag2 = conv_ref(t, w2, b2, 1, pad, res=x)
    bnd = bound(torch.relu(ref), mag2, K) + F.conv2d(delta, w2.double().abs(), None, 1, pad)
    return ref, bnd, delta, t


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


def fault_chunk_swap(ref, b=0, h=None, w=None, chunk=1):
    """One 8-channel chunk of one pixel swapped with its right neighbour's (a
    swizzle slip)."""
    h = ref.shape[2] // 2 if h is None else h
    w = ref.shape[3] // 2 if w is None else w
    out = ref.clone()
    c = slice(8 * chunk, 8 * chunk + 8)
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

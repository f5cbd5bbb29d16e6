"""The element-wise bar of the fused-kernel op tests (test_kernels_fused_gpu.py,
test_kernel_bar_cpu.py): a kernel's output against the float64 result on the
same bf16-rounded operands.

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
   49-term fp32 sum (`avgpool_bound`).

Measured on an MI355X: the worst |err| / bar of any kernel is 0.95
(alex_stem), per kernel in the docstring of test_kernels_fused_gpu.py.

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


def maxpool(t, k=3, s=2):
    """NCHW max-pool without padding."""
    return F.max_pool2d(t, k, s)


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


def assert_close_pooled(got, r, bnd, what, k=3, s=2):
    """A fused max-pool's output against the NCHW reference r (float64, ReLU
    applied, not rounded) and its bar before the pool: see the module text."""
    out = assert_close(got, maxpool(r, k, s), maxpool(bnd, k, s), what)
    assert_close(got, maxpool(bf16r(r), k, s), maxpool(bnd + EPS_OUT * r.abs(), k, s), what + " (bf16-rounded reference)")
    return out


def assert_rejects(got, wrong_ref, bnd, what):
    """The negative control: `got` must miss the bar against a faulty reference."""
    ratio, _ = worst(got, wrong_ref, bnd)
    print(f"{what}: control |err|/bound {ratio:.1f}")
    assert ratio > 1.0, f"{what}: the bar does not see this fault ({ratio})"


# ---------------------------------------------------------------- modelled kernel faults (NCHW float64 references)
def fault_border_taps(ref, x, w, pad):
    """An off-by-one border test: output row `pad` loses its kh = 0 taps (the
    ones on image row 0, next to the top padding)."""
    lost = F.conv2d(x.double()[:, :, 0:1, :], w.double()[:, :, 0:1, :], None, 1, (0, pad))
    out = ref.clone()
    out[:, :, pad:pad + 1, :] -= lost
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


def prob_without_split(logits, lo, hi):
    """Top-1 softmax probability with classes lo..hi-1 left out of the sum (a
    split's partial that never reached the merge)."""
    z = logits.double()
    m = z.max(-1, keepdim=True).values
    e = (z - m).exp()
    e[:, lo:hi] = 0
    return 1.0 / e.sum(-1)

"""The checker of the nearest-neighbour search tests (test_search_gpu.py,
test_search_bar_cpu.py): a (idx, score) answer of csrc/kernels/sim_topk.hip
against float64 on the same bf16-rounded operands.

The bar is a rounding argument in _kernel_bar.py's terms, not a measurement.
The kernel's products are exact (bf16 x bf16 in fp32) and it sums D of them
in fp32 in some order, so to first order its dot product is within
(D - 1) 2^-24 mag of the float64 one, mag = |q| . |g|; the project doubles
the summation term:

    dot:     |got - ref64| <= D 2^-23 mag                       (fp32 output)

Under the cosine metric score = (dot rq) rg with rq = 1 / max(sqrt(sum q^2),
1e-12) computed in fp32 (csrc/kernels/sim_topk.hip's gallery_pack: the
square of a bf16 value has 16 significant bits, so it is exact in fp32; the
fp32 sum of D such non-negative terms is within D 2^-24 relative in any
order; an IEEE square root halves that and adds 2^-24; the IEEE divide adds
2^-24) and rg likewise, both in float64 here. Relative to mag rq rg, which
bounds |ref64|:

    the dot's summation                      D 2^-24
    two inverse norms, each D 2^-25 + 2 2^-24     (D + 4) 2^-24
    the two final multiplies                 2 2^-24
                                             (2 D + 6) 2^-24  <=  (D + 4) 2^-23

and all of it doubled, as the summation term is:

    cosine:  |got - ref64| <= (2 D + 8) 2^-23 mag rq rg.

(gallery_pack's own inverse norms are held to (D + 4) 2^-24 relative of
float64 by the same count: D 2^-25 for the halved sum, the root and the divide
at 2^-24 each, doubled.) The arithmetic is IEEE throughout: no approximate
reciprocal or reciprocal square root.

assert_topk's conditions, B queries, k answers each:
 (a) indices in 0..N-1 and distinct per row;
 (b) scores non-increasing, equal neighbours by ascending index;
 (c) every returned score within the bar of the float64 score of its index;
 (d) no row left out has a float64 score above the row's k-th returned
     float64 score by more than the two bars added;
 (e) positions where idx differs from the float64 stable ranking are at most
     1 % of B k, and each is a pair whose float64 scores differ by no more
     than the two bars added.
"""
import torch

EPS_SUM = 2.0 ** -23  # twice fp32's unit roundoff, per product (tests/_kernel_bar.py)
MAX_MISMATCH = 0.01


def bf16r(t):
    """Round to bf16 (nearest even), back in float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def inv_norm64(rows64):
    return 1.0 / rows64.pow(2).sum(-1).sqrt().clamp_min(1e-12)


_REFS = []  # (q, g, cosine, result) of the last few calls: tests check several answers against one reference


def reference(q, g, cosine):
    """(ref64 [B, N], bar [B, N]) of queries q (any float dtype, rounded to bf16 first) and gallery g (bf16 values).

    cosine: both inverse norms in float64, of the rounded rows. Computed once per (q, g, cosine) object triple:
    the operands must not be changed in place between calls."""
    for cq, cg, cc, res in _REFS:
        if cq is q and cg is g and cc == cosine:
            return res
    res = _reference(q, g, cosine)
    _REFS.append((q, g, cosine, res))
    del _REFS[:-4]
    return res


def _reference(q, g, cosine):
    q64, g64 = bf16r(q.cpu()), g.cpu().double()
    D = q64.shape[1]
    dot = q64 @ g64.t()
    mag = q64.abs() @ g64.abs().t()
    if not cosine:
        return dot, D * EPS_SUM * mag
    rq, rg = inv_norm64(q64)[:, None], inv_norm64(g64)[None, :]
    return dot * rq * rg, (2 * D + 8) * EPS_SUM * mag * rq * rg


def stable_topk(ref, k):
    """The float64 ranking: descending scores, equal scores by ascending index."""
    order = torch.sort(ref, dim=-1, descending=True, stable=True).indices[:, :k]
    return order, ref.gather(1, order)


def check_topk(idx, score, q, g, k, q_scale=None, g_scale=None):
    """None when (idx, score) meets (a)-(e), else the first failed condition as a string.

    q_scale / g_scale: None for the dot metric; anything else (the scales the kernel was given) says that the
    kernel multiplied by the rows' inverse L2 norms, which the reference takes in float64."""
    cosine = q_scale is not None or g_scale is not None
    ref, bar = reference(q, g, cosine)
    B, N = ref.shape
    idx, score = idx.cpu().long(), score.cpu().double()
    if tuple(idx.shape) != (B, k) or tuple(score.shape) != (B, k):
        return f"shape {tuple(idx.shape)} / {tuple(score.shape)}, expected {(B, k)}"
    if not bool(torch.isfinite(score).all()):
        return "a score is not finite"
    # (a)
    if bool((idx < 0).any()) or bool((idx >= N).any()):
        return f"(a) an index outside 0..{N - 1}: {idx[(idx < 0) | (idx >= N)][:4].tolist()}"
    if bool((idx.sort(-1).values.diff(dim=-1) == 0).any()):
        return "(a) an index twice in one row"
    # (b)
    ds, di = score.diff(dim=-1), idx.diff(dim=-1)
    if bool((ds > 0).any()):
        return "(b) scores increase along a row"
    if bool(((ds == 0) & (di < 0)).any()):
        return "(b) equal scores by descending index"
    # (c)
    r_at, b_at = ref.gather(1, idx), bar.gather(1, idx)
    err = (score - r_at).abs()
    if bool((err > b_at).any()):
        w = (err / b_at.clamp_min(1e-300)).max().item()
        return f"(c) a score misses the bar of its index's float64 score: worst |err| / bar = {w:.3g}"
    # (d)
    left = torch.ones_like(ref, dtype=torch.bool).scatter_(1, idx, False)
    over = ref - r_at[:, k - 1:k] - (bar + b_at[:, k - 1:k])
    if bool(((over > 0) & left).any()):
        b = int(((over > 0) & left).any(-1).nonzero()[0])
        return f"(d) query {b}: a row left out scores above the k-th returned one by more than both bars"
    # (e)
    want, r_want = stable_topk(ref, k)
    diff = idx != want
    n_diff = int(diff.sum())
    if n_diff > MAX_MISMATCH * B * k:
        return f"(e) {n_diff} of {B * k} positions differ from the float64 stable ranking"
    gap = (r_at - r_want).abs() - (b_at + bar.gather(1, want))
    if bool(((gap > 0) & diff).any()):
        return "(e) a differing position is not a near tie"
    return None


def assert_topk(idx, score, q, g, k, q_scale=None, g_scale=None):
    """(idx, score) [B, k] against float64 on the bf16-rounded operands: conditions (a)-(e) of the module text."""
    ref, bar = reference(q, g, q_scale is not None or g_scale is not None)
    r_at = ref.gather(1, idx.cpu().long().clamp(0, ref.shape[1] - 1))
    b_at = bar.gather(1, idx.cpu().long().clamp(0, ref.shape[1] - 1))
    worst = ((score.cpu().double() - r_at).abs() / b_at.clamp_min(1e-300)).max().item()
    n_diff = int((idx.cpu().long() != stable_topk(ref, k)[0]).sum())
    print(f"topk B={ref.shape[0]} N={ref.shape[1]} D={q.shape[1]} k={k}: worst |err| / bar = {worst:.4f}, "
          f"{n_diff} positions off the float64 ranking")
    why = check_topk(idx, score, q, g, k, q_scale, g_scale)
    assert why is None, why


def assert_rejects(idx, score, q, g, k, q_scale=None, g_scale=None, what=""):
    """The negative control: the same comparison must refuse this answer."""
    why = check_topk(idx, score, q, g, k, q_scale, g_scale)
    print(f"control {what}: {why}")
    assert why is not None, f"{what}: the checker does not see this fault"
    return why


def exact_topk(q, g, k):
    """Small-integer operands (every fp32 sum exact): the answer bit for bit, (idx int32, score float32)."""
    ref = q.cpu().double() @ g.cpu().double().t()
    assert float(ref.abs().max()) < 2 ** 24
    order, vals = stable_topk(ref, k)
    return order.to(torch.int32), vals.to(torch.float32)

"""The reference e4m3 quantiser of the search tests (test_search_e4m3_cpu.py,
test_search_e4m3_gpu.py): csrc/kernels/sim_topk.hip's gallery_pack8 rule on
the CPU, bit for bit, and the planted-neighbour data both files use.

For a finite row v (bf16 widened first): amax = max |v_d| = m 2^x with
1 <= m < 2; e = 8 - x if m <= 1.75 else 7 - x (the largest integer with
amax 2^e <= 448), clamped to [-126, 126], 0 for a zero row; codes =
e4m3fn(v 2^e), nearest even, subnormals kept. The multiply by a power of two
is exact, so torch's own fp32 -> float8_e4m3fn conversion reproduces the
codes. Scale: 2^-e (dot), or 1 / max(sqrt(sum codes^2), 1e-12) (cosine; in
float64 here).
"""
import torch


def exponents(rows):
    """e [M] (int32) of float32 / bfloat16 rows [M, D]."""
    amax = rows.to(torch.float32).abs().amax(-1)
    m, x1 = torch.frexp(amax)  # amax = m 2^x1, 0.5 <= m < 1: the text's m is 2 m, its x is x1 - 1
    e = torch.where(m <= 0.875, 9 - x1, 8 - x1).clamp(-126, 126)
    return torch.where(amax == 0, torch.zeros_like(e), e).to(torch.int32)


def quantise(rows, metric="dot"):
    """(codes float8_e4m3fn [M, D], scale [M], e int32 [M]); scale is float32 2^-e (dot) or the float64 inverse norm
    of the codes (cosine)."""
    e = exponents(rows)
    scaled = torch.ldexp(rows.to(torch.float64), e[:, None]).to(torch.float32)  # (exact)
    assert float(scaled.abs().max()) <= 448 if scaled.numel() else True
    codes = scaled.to(torch.float8_e4m3fn)
    if metric == "dot":
        scale = torch.ldexp(torch.ones(len(e), dtype=torch.float64), -e).to(torch.float32)
    else:
        scale = 1.0 / codes.to(torch.float64).pow(2).sum(-1).sqrt().clamp_min(1e-12)
    return codes, scale, e


def round_bytes(v):
    """e4m3fn(v) as uint8 bytes, by the same conversion as `quantise` (nearest even, subnormals kept); v finite,
    |v| <= 448 and exact in float32."""
    v32 = v.to(torch.float32)
    assert torch.equal(v32.to(torch.float64), v.to(torch.float64)) and float(v32.abs().max()) <= 448
    return v32.to(torch.float8_e4m3fn).view(torch.uint8)


def dequantise(codes, e):
    """codes 2^-e as float32: exact, and a bf16 value (4 significant bits)."""
    return torch.ldexp(codes.to(torch.float64), -e[:, None]).to(torch.float32)


def planted(B=64, N=5003, D=512, seed=5):
    """(q [B, D], g [N, D]) float32: row 16 b + j has cosine 0.9 - 0.04 j to query b (j < 16), every other row is
    random; all row norms are scaled by random factors in [0.01, 50]."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, D, generator=gen, dtype=torch.float64)
    g = torch.randn(N, D, generator=gen, dtype=torch.float64)
    qu = q / q.norm(dim=-1, keepdim=True)
    for b in range(B):
        for j in range(16):
            u = g[16 * b + j] - (g[16 * b + j] @ qu[b]) * qu[b]
            u = u / u.norm()
            c = 0.9 - 0.04 * j
            g[16 * b + j] = c * qu[b] + (1 - c * c) ** 0.5 * u
    lo, hi = torch.tensor(0.01).log(), torch.tensor(50.0).log()
    g = g * (lo + (hi - lo) * torch.rand(N, 1, generator=gen, dtype=torch.float64)).exp()
    q = q * (lo + (hi - lo) * torch.rand(B, 1, generator=gen, dtype=torch.float64)).exp()
    return q.to(torch.float32), g.to(torch.float32)

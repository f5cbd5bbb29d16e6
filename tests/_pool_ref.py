"""The global average pool's reference, shared by test_embed_gpu.py and
test_kernels_pool_gpu.py: the test inputs, and avgpool_global's stated
summation order performed literally in torch fp32 on the CPU."""
import torch

from dmlc import ops


def _input(B, HW, C, scale, seed, cancelling=False):
    """CPU input of a case: bf16 randn, or random e4m3 bytes without the two NaN encodings.

    fp32 sums of 49 bf16 randn values (8 significant bits within a few binades) are exact, and so are sums of
    e4m3 values: every summation order gives the same bits. cancelling: pixel 0 scaled by 2^20 and pixel 9 its
    negative, so the small pixels added in between lose low bits to the large one before it cancels, and the
    result depends on the order well above a bf16 ulp."""
    g = torch.Generator().manual_seed(seed)
    if scale is None:
        x = torch.randn(B, HW, C, generator=g).bfloat16()
        if cancelling:
            x[:, 0] *= 2.0 ** 20
            x[:, 9] = -x[:, 0]
        return x[:, 0].contiguous() if HW == 1 else x
    b = torch.randint(0, 256, (B, HW, C), dtype=torch.uint8, generator=g)
    b[(b & 0x7F) == 0x7F] = 0x38  # 0x7f / 0xff are NaN: 1.0 instead
    return b


def _widen(x_cpu):
    return x_cpu.view(ops.FP8).float() if x_cpu.dtype == torch.uint8 else x_cpu.float()


def _pool_emulated(xf, scale, sequential=False):
    """avgpool_global's order in torch fp32 on the CPU. xf: fp32 [B, HW, C]. sequential: plain pixel order instead."""
    B, HW, C = xf.shape
    parts = []
    for p in range(1 if sequential else 8):
        s = torch.zeros(B, C, dtype=torch.float32)
        for i in range(p, HW, 1 if sequential else 8):
            s = s + xf[:, i]
        parts.append(s)
    tot = parts[0] if sequential else \
        ((parts[0] + parts[1]) + (parts[2] + parts[3])) + ((parts[4] + parts[5]) + (parts[6] + parts[7]))
    inv = torch.tensor(1.0 if scale is None else scale, dtype=torch.float32) / torch.tensor(float(HW))
    return (tot * inv).bfloat16().float()

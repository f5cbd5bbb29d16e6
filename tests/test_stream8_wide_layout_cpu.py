"""conv3x3_stream8's WIDE form (14x14x256 -> 7x7x512 at stride 2, IMG = 2
whole images per workgroup, conv3x3_stream8_block.hip): the staging and read
offsets of conv3x3_stream8_kernel.h modelled as in test_layouts_cpu.py's
stride-2 case, with the second image's rows and its key offset H * W = 49.
Every lane must read the 32 channels of input pixel (2r + kh - 1, 2c + kw - 1)
of its image (odd fq: second 16 first), border lanes the zero pixel, and both
16-B reads of every X fragment must be bank-conflict free, the downsample
phase's centre tap (tap 4) included."""
import torch

from test_layouts_cpu import _B128_GROUPS

H = W = 7
CI, IMG = 256, 2
HI, WI, CPX = 2 * H, 2 * W, CI // 16


def test_stream8_wide_lds_layout():
    torch.manual_seed(2)
    img = torch.randint(0, 256, (IMG * HI, WI, CI), dtype=torch.uint8)  # the images' rows, one after the other
    ZB = IMG * HI * WI * CI
    lds = torch.zeros(ZB + CI, dtype=torch.uint8)  # + the zero pixel
    for i in range(IMG * HI):
        ii, y = divmod(i, HI)
        for q in range(WI):
            x = 2 * q if q < WI // 2 else 2 * (q - WI // 2) + 1
            K = ii * H * W + ((y + 1) >> 1) * W + ((x + 1) >> 1)
            for pc in range(CPX):
                lc = (((pc >> 1) ^ (K & 7)) << 1) | (pc & 1)
                o = (i * WI + q) * CI + 16 * pc
                lds[o:o + 16] = img[i, x, 16 * lc:16 * lc + 16]
    npix = IMG * H * W
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        dq = WI // 2 - 1 if kw == 0 else (0 if kw == 1 else WI // 2)
        toff = ((kh - 1) * WI + dq) * CI
        ktap = (W if kh == 2 else 0) + (1 if kw == 2 else 0)
        for cc in range(CI // 128):
            for f in range((npix + 15) // 16):
                a0, a1 = [], []
                for lane in range(64):
                    fr, fq = lane & 15, lane >> 4
                    p = min(16 * f + fr, npix - 1)
                    ii, pi = divmod(p, H * W)
                    r, pcol = divmod(pi, W)
                    inside = not ((r == 0 and kh == 0) or (pcol == 0 and kw == 0))
                    xa = ((ii * HI + 2 * r) * WI + pcol) * CI + toff if inside else ZB
                    t0 = ((fq ^ ((fr + ktap) & 7)) << 5) | ((fq & 1) << 4)
                    a0.append(xa + (t0 ^ (cc << 7)))
                    a1.append(xa + ((t0 ^ 16) ^ (cc << 7)))
                    got = torch.cat([lds[a0[-1]:a0[-1] + 16], lds[a1[-1]:a1[-1] + 16]])
                    if inside and 16 * f + fr < npix:
                        ch = 128 * cc + 32 * fq
                        exp = img[ii * HI + 2 * r + kh - 1, 2 * pcol + kw - 1, ch:ch + 32]
                        if fq & 1:
                            exp = torch.cat([exp[16:], exp[:16]])
                        assert torch.equal(got, exp), (tap, cc, f, lane)
                    elif not inside:
                        assert not got.any()
                live = [l for l in range(64) if 16 * f + (l & 15) < npix]  # border lanes included
                for addr in (a0, a1):
                    for grp in _B128_GROUPS:
                        slots = {}
                        for l in grp:
                            if l in live:
                                slots.setdefault((addr[l] // 16) % 16, set()).add(addr[l])
                        assert all(len(v) == 1 for v in slots.values()), (tap, cc, f)

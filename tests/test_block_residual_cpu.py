"""CPU checks of conv3x3_block.hip's residual read from the x ring (no GPU
needed): the read's LDS addresses (bank conflicts, which channels they
fetch), a replay of the ring's slots over the kernel's 16 steps (every row is
in the ring when a producer or a consumer reads it, and no DMA of a step
lands on a row read in that step), and the GPU test's negative control.
"""
import pytest
import torch

import _kernel_bar as kb
from test_layouts_cpu import _b128_ways

RING = kb.kernel_const("conv3x3_block.hip", "kRing")
H = W = 56  # the only shape the kernel accepts
R = kb.kernel_const("conv3x3_block.hip", "kR")
STEPS = H // R + 2
Q = W + 2
HALF = Q * 64
SLOT = 2 * HALF


def test_residual_read_addresses():
    """Lane (fr, g) of fragment f reads, from the slot of its pixel's row,
    K half wn, column q = col + 1, chunk g ^ ((q >> 1) & 3): conflict free,
    and by the staging rule (chunk c of (h, q) holds channels
    8 (4h + (c ^ ((q >> 1) & 3)))) exactly channels 32 wn + 8 g .. + 7."""
    for nr in range(0, H, R):  # the consumer step's first row
        for wm in range(2):
            for wn in range(2):
                for f in range(R * W // 32):
                    addr = []
                    for lane in range(64):
                        fr, g = lane & 15, lane >> 4
                        p = wm * (R * W // 2) + 16 * f + fr
                        row, q = nr + p // W, p % W + 1
                        a = (row % RING) * SLOT + wn * HALF + q * 64 + ((g ^ ((q >> 1) & 3)) << 4)
                        addr.append(a)
                        h, rest = (a % SLOT) // HALF, (a % SLOT) % HALF
                        c = (rest % 64) // 16
                        assert rest // 64 == q and 1 <= q <= W
                        assert 8 * (4 * h + (c ^ ((q >> 1) & 3))) == 32 * wn + 8 * g
                    assert _b128_ways(addr) == 1, (nr, wm, wn, f)
                    assert max(addr) + 16 <= RING * SLOT


def _dma_rows(step):
    """x rows whose DMA (or zero fill, rows >= 56) the producers issue at the
    top of `step`: issue_dma of the kernel."""
    if step + 1 > H // R:
        return []
    base = -3 if step == 0 else R * (step - 1) + 1
    nb = 1 if step == 0 else base + R
    return [r for r in range(nb + 1, nb + R + 1) if r >= 6]


def test_x_ring_replay():
    ring = {r % RING: r for r in range(0, 6)}
    ring[(-1) % RING] = -1  # the zeroed slot
    residual_of = {}
    for step in range(STEPS):
        landing = _dma_rows(step)
        targets = {r % RING for r in landing}
        reads = []
        if step <= H // R:  # producers: t rows base .. base + 3 read x rows base - 1 .. base + 4
            base = -3 if step == 0 else R * (step - 1) + 1
            first = base + 1 if step == 0 else base - 1  # step 0: pixel half 1 only (tile rows 2, 3)
            reads += [r for r in range(first, base + R + 1)]
        if 1 <= step < STEPS - 1:  # consumers: the next step's residual rows, before the barrier
            nb = R * (step - 1)
            residual_of[step + 1] = list(range(nb, nb + R))
            reads += residual_of[step + 1]
        for r in reads:
            if r >= H or r < -1:  # zero-filled slots past the image; row -2 feeds only t row -1, stored as zeros
                continue
            assert ring.get(r % RING) == r, f"step {step}: x row {r} is not in the ring"
            assert r % RING not in targets, f"step {step}: x row {r} is read while this step's DMA lands on its slot"
        for r in landing:  # landed by the step's closing barrier
            ring[r % RING] = r
    # every consumer step got the rows it stores: C_{s-2} = y rows 4 (s - 2) .. + 3
    assert residual_of == {s: list(range(R * (s - 2), R * (s - 2) + R)) for s in range(2, STEPS)}
    # and the read cannot move past the barrier: the next step's DMA lands on exactly those rows' slots
    for s in range(2, H // R):
        assert {r % RING for r in _dma_rows(s)} == {r % RING for r in residual_of[s]}


@pytest.mark.parametrize("B", [1, 3])
def test_stale_residual_control_is_rejected(B):
    """The float64 reference itself, rounded to bf16, passes the chained bar
    on the GPU test's operands, and misses it against the stale-residual
    reference: the bar sees that fault."""
    import test_block_memwait_gpu as m
    name = f"random B={B}"
    ref, bnd = m.reference(name)
    y = kb.bf16r(torch.relu(ref))
    kb.assert_close(y, torch.relu(ref), bnd, name)
    kb.assert_rejects(y, torch.relu(m.stale_residual(*m._case(name))), bnd, name + " [stale residual]")


def test_edge_case_reference_passes_its_own_bar():
    import test_block_memwait_gpu as m
    ref, bnd = m.reference("edges")
    kb.assert_close(kb.bf16r(torch.relu(ref)), torch.relu(ref), bnd, "edges")

"""The e4m3 gallery without a GPU (csrc/kernels/sim_topk.hip's FP8 form):
the reference quantiser the GPU tests compare gallery_pack8 with, the native
sizing functions and refusals, the kernel's LDS layout, and the
planted-neighbour data of the GPU test."""
import pytest
import torch

import dmlc
from _e4m3_ref import dequantise, exponents, planted, quantise
from _search_bar import EPS_SUM, reference, stable_topk

C = dmlc.native()


# ---------------------------------------------------------------- the reference quantiser
def test_quantiser_range():
    gen = torch.Generator().manual_seed(3)
    rows = torch.randn(200, 256, generator=gen) * torch.logspace(-20, 20, 200, base=2.0)[:, None]
    rows[7] = 0
    for src in (rows, rows.bfloat16()):
        codes, scale, e = quantise(src, "dot")
        c = codes.float()
        assert bool(torch.isfinite(c).all()) and float(c.abs().max()) <= 448
        top = torch.ldexp(src.float().abs().amax(-1).double(), e)
        live = torch.arange(200) != 7
        assert bool((top[live] > 224).all()) and bool((top[live] <= 448).all())  # one more doubling would pass 448
        assert int(e[7]) == 0 and float(scale[7]) == 1 and not bool(c[7].any())
        assert torch.equal(scale.double(), torch.ldexp(torch.ones(200, dtype=torch.float64), -e))
        # the largest element of a row is rounded at 3 mantissa bits: within 2^-4 relative
        back = dequantise(codes, e)
        big = src.float().abs().argmax(-1, keepdim=True)
        rel = (back.gather(1, big) - src.float().gather(1, big)).abs() / src.float().gather(1, big).abs().clamp_min(1e-30)
        assert float(rel[live].max()) <= 2.0 ** -4


def test_quantiser_edges():
    def e_of(amax):
        row = torch.zeros(1, 128)
        row[0, 5] = -amax
        return int(exponents(row)[0])
    assert e_of(56.0) == 3 and e_of(57.0) == 2           # 56 * 8 = 448; 57 * 8 = 456 > 448
    assert e_of(448.0) == 0 and e_of(449.0) == -1 and e_of(1.0) == 8 and e_of(1.75) == 8 and e_of(1.7500001) == 7
    assert e_of(448 * 2.0 ** -3) == 3 and e_of(2.0 ** -140) == 126 and e_of(3e38) == -120
    # subnormal codes are kept: 2^-9 is e4m3's smallest
    row = torch.zeros(1, 128)
    row[0, 0], row[0, 1], row[0, 2] = 256.0, 2.0 ** -9, 2.0 ** -11
    codes, _, e = quantise(row)
    assert int(e[0]) == 0 and codes.float()[0, :3].tolist() == [256.0, 2.0 ** -9, 0.0]


def test_small_integers_are_exact():
    gen = torch.Generator().manual_seed(9)
    for D in (128, 4096):
        q = torch.randint(-3, 4, (9, D), generator=gen).float()
        g = torch.randint(-3, 4, (33, D), generator=gen).float()
        g[4] = 0
        g[5] = g[5].clamp(-1, 1)
        (cq, sq, eq), (cg, sg, eg) = quantise(q), quantise(g)
        assert torch.equal(dequantise(cq, eq), q) and torch.equal(dequantise(cg, eg), g)
        # products are multiples of 2^14 (of 2^12 where a row's amax is below 3) and |sum| <= 448^2 4096 < 2^30:
        # the fp32 matmul of the codes is exact in any order
        f32 = cq.float() @ cg.float().t()
        assert torch.equal(f32.double(), cq.double() @ cg.double().t())
        score = (f32 * sq[:, None]) * sg[None, :]
        assert torch.equal(score.double(), q.double() @ g.double().t())
    # dequantised codes and raw codes are bf16 values
    rows = torch.randn(50, 128, generator=gen) * 37
    codes, _, e = quantise(rows)
    for t in (codes.float(), dequantise(codes, e)):
        assert torch.equal(t.bfloat16().float(), t)


# ---------------------------------------------------------------- native sizing and refusals, no device
@pytest.mark.parametrize("D,ok", [(0, False), (64, False), (96, False), (128, True), (192, False), (512, True),
                                  (2048, True), (4096, True), (4224, False)])
def test_supported(D, ok):
    assert C.sim_topk8_supported(D) is ok


def test_workspace():
    for B in (1, 17, 256, 300):
        for k in (1, 5, 16):
            for s in (1, 7, 256, 512):
                n = C.sim_topk8_ws_bytes(B, k, s)
                assert n >= s * B * k * 8 + B * 4096 + B * 4  # candidates, the queries' codes, their scales
    for bad in ((-1, 1, 1), (1, -1, 1), (1, 1, -1)):
        with pytest.raises(ValueError):
            C.sim_topk8_ws_bytes(*bad)


def test_native_refusals_before_any_launch():
    """Every refusal comes before the first launch: these run without a device, on pointers never read."""
    F32, F16 = C.TensorDType.F32, C.TensorDType.F16
    P = 4096  # (16-B aligned, never dereferenced)

    def search(q=P, dt=F32, g=P, gs=P, B=2, N=40, D=128, k=16, ws=P, ws_bytes=None, slices=0, g_label=0, q_want=0):
        n = C.sim_topk8_ws_bytes(max(B, 0), 16, 1) if ws_bytes is None else ws_bytes
        C.sim_topk8(q, dt, g, gs, True, B, N, D, k, P, P, ws, n, 256, 0, slices=slices, g_label=g_label, q_want=q_want)
    for kw in (dict(D=96), dict(D=64), dict(D=4224), dict(k=0), dict(k=17), dict(k=10, N=9), dict(N=0), dict(B=-1),
               dict(dt=F16), dict(slices=2), dict(slices=-1), dict(ws_bytes=C.sim_topk8_ws_bytes(2, 16, 1) - 1),
               dict(q=0), dict(g=0), dict(gs=0), dict(ws=0), dict(q=P + 8), dict(g=P + 4), dict(q_want=P)):
        with pytest.raises(ValueError):
            search(**kw)
    search(B=0)  # nothing to do, nothing launched

    def pack(rows=P, dt=F32, codes=P, scale=P, M=3, D=128):
        C.gallery_pack8(rows, dt, codes, scale, True, M, D, 0)
    for kw in (dict(D=96), dict(D=8192), dict(M=-1), dict(dt=F16), dict(rows=0), dict(codes=0), dict(scale=0),
               dict(rows=P + 4), dict(codes=P + 8)):
        with pytest.raises(ValueError):
            pack(**kw)
    pack(M=0)


# ---------------------------------------------------------------- the LDS layout
# ds_read_b128 is serviced in four 16-lane groups; a group is conflict-free
# when its distinct 16-B addresses hit distinct banks (test_layouts_cpu.py).
_B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
                list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
_B128_GROUPS += [[l + 32 for l in g] for g in _B128_GROUPS]


def _b128_ways(addr):
    worst = 1
    for grp in _B128_GROUPS:
        banks = {}
        for l in grp:
            for b in range(addr[l] // 4, addr[l] // 4 + 4):
                banks.setdefault(b % 64, set()).add(addr[l])
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


GB = 128 * 128  # the gallery region of a stage; the 256 query rows follow


def _st_off(r, c):
    return r * 128 + ((c ^ (r & 7)) << 4)


def _reads(region, row0, pairing):
    """The two ds_read_b128 of one fragment: per read the 64 lanes' addresses."""
    out = []
    for half in range(2):
        addr = []
        for lane in range(64):
            fr, fq = lane & 15, lane >> 4
            c = (fq, fq + 4)[half] if pairing == "fq,fq+4" else 2 * fq + half
            addr.append(region + _st_off(row0 + fr, c))
        out.append(addr)
    return out


def test_lds_fragment_reads_conflict_free():
    for gf in range(8):
        for addr in _reads(0, 16 * gf, "fq,fq+4"):
            assert _b128_ways(addr) == 1, gf
    for wave in range(8):
        for qf in range(2):
            for addr in _reads(GB, 32 * wave + 16 * qf, "fq,fq+4"):
                assert _b128_ways(addr) == 1, (wave, qf)
    # the control: chunks 2 fq, 2 fq + 1 under the same swizzle would be 2-way
    assert _b128_ways(_reads(0, 0, "2fq,2fq+1")[0]) == 2


def test_lds_dma_places_chunks_where_reads_expect():
    """LDS-DMA instruction i of a region: lane l's 16 bytes land at 1024 i + 16 l, position p = 64 i + l is row
    p >> 3, and the lane fetches logical chunk (p & 7) ^ (row & 7) (K bytes 16 c .. 16 c + 15 of the block)."""
    for rows, n_instr in ((128, 16), (256, 32)):
        placed = {}
        for i in range(n_instr):
            for lane in range(64):
                p = 64 * i + lane
                r = p >> 3
                placed[(r, (p & 7) ^ (r & 7))] = 1024 * i + 16 * lane
        assert placed == {(r, c): _st_off(r, c) for r in range(rows) for c in range(8)}
    # a lane's two chunks cover the same K bytes for both operands, and the four fq cover the block once
    assert sorted(c for fq in range(4) for c in (fq, fq + 4)) == list(range(8))


# ---------------------------------------------------------------- the planted neighbours of the GPU test
def test_planted_neighbours_rank_first():
    q, g = planted()
    B, D = q.shape
    (cq, _, _), (cg, _, _) = quantise(q), quantise(g)
    ref, bar = reference(cq.to(torch.bfloat16), cg.to(torch.bfloat16), True)  # float64 cosine of the codes
    order, vals = stable_topk(ref, 17)
    want = 16 * torch.arange(B)[:, None] + torch.arange(16)[None, :]
    assert torch.equal(order[:, :16], want)
    gap = vals[:, :-1] - vals[:, 1:]
    bars = bar.gather(1, order)
    assert bool((gap > bars[:, :-1] + bars[:, 1:]).all())
    assert float(bar.max()) <= (2 * D + 8) * EPS_SUM
    # against the unquantised cosine: the codes move a score by about 0.002, far inside the 0.04 steps
    exact = (q.double() / q.double().norm(dim=-1, keepdim=True)) @ (g.double() / g.double().norm(dim=-1, keepdim=True)).t()
    assert float((ref - exact).abs().max()) < 0.01

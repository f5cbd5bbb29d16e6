"""Host-side launch parameters of the nearest-neighbour search
(csrc/kernels/sim_topk.hip), no GPU needed: the gallery is cut into slices of
whole 128-row tiles that cover it exactly once and are never empty, there are
never more slices than tiles (or than the merge's 512), and the workspace
holds every slice's k candidates per query."""
import pytest

import dmlc

C = dmlc.native()
TILE = 128
NS = [1, 2, 127, 128, 129, 1000, 5003, 20011, 100_000, 1_000_000, 10_000_000]


@pytest.mark.parametrize("cus", [1, 8, 104, 256, 304, 1024])
@pytest.mark.parametrize("B", [1, 16, 17, 256, 300])
def test_slices(B, cus):
    for N in NS:
        tiles = (N + TILE - 1) // TILE
        s = C.sim_topk_slices(B, N, cus)
        assert 1 <= s <= min(tiles, cus, 512), (N, s)
        assert s <= C.sim_topk_max_slices(N) == min(tiles, 512)
        if tiles >= cus and cus <= 512:
            assert s == cus  # one workgroup per CU
        for n_slices in {s, 1, C.sim_topk_max_slices(N)}:
            end = 0
            for i in range(n_slices):
                first, last = C.sim_topk_slice_rows(N, n_slices, i)
                assert first == end and first % TILE == 0 and last > first, (N, n_slices, i)
                assert last % TILE == 0 or last == N
                end = last
            assert end == N
        for k in (1, 5, 16):
            assert C.sim_topk_ws_bytes(B, k, s) >= s * B * k * 8  # a score and a row each


def test_slice_rows_rejects():
    for bad in [(1000, 0, 0), (1000, 9, 0), (1000, 4, 4), (1000, 4, -1), (0, 1, 0)]:
        with pytest.raises(ValueError):
            C.sim_topk_slice_rows(*bad)
    assert C.sim_topk_slices(1, 0, 256) == 0 and C.sim_topk_max_slices(0) == 0


@pytest.mark.parametrize("D,ok", [(0, False), (16, False), (32, True), (48, False), (4096, True), (4128, False)])
def test_supported(D, ok):
    assert C.sim_topk_supported(D) is ok

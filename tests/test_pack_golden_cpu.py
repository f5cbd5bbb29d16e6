"""The packed weight arena against recorded digests, no GPU needed.

tests/golden/pack_digests.json holds, for every case of test_pack_cpu.py
packed from _golden_weights.golden_weights: the arena's size, a 64-bit FNV-1a
digest of the whole arena, one chained digest per region kind, and the region
table (layer, kind, off, bytes, digest of the region's bytes) with a sha256 of
its layout. It was recorded with Engine::pack_digest from the packer as it was
before layout_weights / pack_host moved to csrc/runtime/engine_pack.cpp and
were rewritten around FragOrder, so a change to the packer that alters one
byte or one offset of the arena fails here and names the first region that
differs.

Record again (PYTHONPATH=. python tests/test_pack_golden_cpu.py) only with a change that
means to alter the arena.
"""
import hashlib
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pack_digests.json")
ORDERS = {"None", "Stream", "Stream8", "StemDense", "AlexStem"}  # FragOrder's enumerators


def _cases():
    from test_pack_cpu import CASES
    from _golden_weights import case_id
    return [(case_id(a, o), a, o) for a, o in CASES]


def _pack(arch, opts):
    from dmlc import native
    from _golden_weights import golden_weights
    return native().pack_digest(arch, golden_weights(arch), opts)


def _record(packed):
    """pack_digest's result as the golden file stores it."""
    total, arena, kinds, regions = packed[:4]
    table = [[layer, kind, off, n] for layer, kind, off, n, _ in regions]
    return {
        "total": total,
        "arena": f"{arena:016x}",
        "kinds": {k: f"{v:016x}" for k, v in sorted(kinds.items())},
        "table_sha256": hashlib.sha256(json.dumps(table).encode()).hexdigest(),
        "regions": [[layer, kind, off, n, f"{d:016x}"] for layer, kind, off, n, d in regions],
    }


@pytest.fixture(scope="module")
def packed():
    """case id -> pack_digest's result for the golden weights, each case packed once."""
    cache = {}

    def get(cid, arch, opts):
        if cid not in cache:
            cache[cid] = _pack(arch, opts)
        return cache[cid]
    return get


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _first_difference(got, want):
    for g, w in zip(got["regions"], want["regions"]):
        if g != w:
            return f"first differing region: {g[0]} {g[1]} (off, bytes, digest) {g[2:]}, recorded {w[0]} {w[1]} {w[2:]}"
    n, m = len(got["regions"]), len(want["regions"])
    if n != m:
        extra = (got if n > m else want)["regions"][min(n, m)]
        return f"{n} regions, recorded {m}: first unmatched {extra[0]} {extra[1]}"
    return "every region matches its record: the difference is in the padding between regions"


@pytest.mark.parametrize("cid,arch,opts", _cases(), ids=[c[0] for c in _cases()])
def test_pack_matches_golden(packed, golden, cid, arch, opts):
    got, want = _record(packed(cid, arch, opts)), golden[cid]
    why = "" if got == want else _first_difference(got, want)
    if why:
        print(why)
    assert got["total"] == want["total"], why
    assert [r[:4] for r in got["regions"]] == [r[:4] for r in want["regions"]], why
    assert got["table_sha256"] == want["table_sha256"], why
    assert got["kinds"] == want["kinds"], why
    assert got["arena"] == want["arena"], why


def test_one_fragment_order_per_layer(packed):
    """Engine's frag_order gives every layer exactly one FragOrder, and the
    layers with a wf region are exactly those whose order is not None."""
    for cid, arch, opts in _cases():
        regions, orders = packed(cid, arch, opts)[3:5]
        layers = [layer for layer, _ in orders]
        assert sorted(layers) == sorted(r[0] for r in regions if r[1] == "w"), cid
        assert {o for _, o in orders} <= ORDERS, cid
        assert {layer for layer, o in orders if o != "None"} == {r[0] for r in regions if r[1] == "wf"}, cid


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump({cid: _record(_pack(arch, opts)) for cid, arch, opts in _cases()}, f, indent=0)
        f.write("\n")

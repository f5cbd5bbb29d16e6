"""What tells one captured hipGraph from another (Engine::key_of), no GPU needed.

A forward replays the graph captured for its key, so two requests whose
launches differ in any argument must never share one: every pointer and size
of the request is in the key, the input kind tells a u8 forward from each kind
of tensor forward on the same pointer, and the normalise flag counts only next
to a features buffer (without one it changes nothing). ``graph_key`` takes
integers for pointers and touches no device.
"""
import itertools

from dmlc import native

# graph_key's arguments; arbitrary, pairwise different, non-zero "pointers"
BASE = dict(images=0x7000_1000, B=4, Hin=224, Win=224, k=1, idx=0x7000_2000, prob=0x7000_3000, logits=0x7000_4000,
            features=0x7000_5000, l2norm=False)
CHANGED = dict(images=0x7100_1000, B=5, Hin=200, Win=300, k=5, idx=0x7100_2000, prob=0x7100_3000, logits=0x7100_4000,
               features=0x7100_5000)


def key(**changes):
    return native().graph_key(**{**BASE, **changes})


def test_every_field_is_keyed():
    base = key()
    for name, value in CHANGED.items():
        assert value != BASE[name]
        assert key(**{name: value}) != base, name
    # a buffer that comes or goes is a change of that field too
    for name in ("logits", "features"):
        assert key(**{name: 0}) != base, name


def test_l2norm_counts_only_next_to_a_features_buffer():
    assert key(features=0, l2norm=True) == key(features=0, l2norm=False)
    assert key(l2norm=True) != key(l2norm=False)


def test_input_kinds_never_share_a_key():
    T = native().TensorDType
    kinds = [None] + [(dt, cl) for dt in (T.F32, T.F16, T.BF16) for cl in (False, True)]
    keys = [key(tensor=t) for t in kinds]
    assert len(keys) == 7
    for (i, a), (j, b) in itertools.combinations(enumerate(keys), 2):
        assert a != b, (kinds[i], kinds[j])


def test_same_arguments_same_key():
    T = native().TensorDType
    for changes in ({}, dict(l2norm=True), dict(features=0), dict(tensor=(T.BF16, True))):
        assert key(**changes) == key(**changes)
    assert all(isinstance(v, int) for v in key())

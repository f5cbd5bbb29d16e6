"""Weights for the pack / plan goldens (tests/golden/pack_digests.json,
plan_digests.json): the zoo's parameter names and shapes, values that depend
on neither torch's RNG nor its initialisers, so a recorded digest stays valid
across torch versions.
"""
import numpy as np

from dmlc.models import build, state_dict_f32

_cache = {}


def golden_weights(arch):
    """{name: float32 array}: numpy.random.RandomState(0) standard normals,
    keys visited in sorted order; running_var = |.| + 0.5."""
    base = arch.replace("_fp8", "")
    if base not in _cache:
        shapes = {k: tuple(v.shape) for k, v in state_dict_f32(build(base, seed=0)).items()}
        rng = np.random.RandomState(0)
        w = {}
        for k in sorted(shapes):
            v = rng.standard_normal(shapes[k]).astype(np.float32)
            w[k] = np.abs(v) + np.float32(0.5) if k.endswith("running_var") else v
        _cache[base] = w
    return _cache[base]


def case_id(arch, opts):
    return f"{arch}-{'-'.join(opts) or 'default'}"

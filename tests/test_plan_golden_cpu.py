"""The engine's launch plans against recorded digests, no GPU needed.

tests/golden/plan_digests.json holds a sha256 of the JSON of plan_audit's
plan lines (kernel, first op, n_ops, detail) on a 256-CU device for every case
of test_pack_cpu.py at B in {1, 4, 32, 200, 256}, native and resized images
(B = 200 is on the wrong side of the planner's 70 %-of-a-round rule), and at
B = 256 once each with topk=5, a tensor input and features. It was recorded
from the planner as it was before it moved to csrc/runtime/engine_plan.cpp and
its predicates changed from "the layer has a wf_off" to "the layer's FragOrder
is the one my kernel reads", so a predicate that stops matching fails here
where test_plan_cpu.py has no sequence for the case.

Record again (PYTHONPATH=. python tests/test_plan_golden_cpu.py) only with a change that
means to alter a plan.
"""
import hashlib
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "plan_digests.json")
CUS = 256
SPECS = ([(f"b{B}{'' if nat else '-resized'}", dict(B=B, native=nat)) for B in (1, 4, 32, 200, 256)
          for nat in (True, False)] +
         [(f"b256-{k}", dict(B=256, native=True, **{k: v}))
          for k, v in (("topk", 5), ("tensor_in", True), ("features", True))])


def _cases():
    from test_pack_cpu import CASES
    from _golden_weights import case_id
    return [(case_id(a, o), a, o) for a, o in CASES]


def _plan(arch, opts, spec):
    from dmlc import native
    from _golden_weights import golden_weights
    lines, _ = native().plan_audit(arch, golden_weights(arch), opts, num_cus=CUS, **spec)
    return [list(line) for line in lines]


def _sha(lines):
    return hashlib.sha256(json.dumps(lines).encode()).hexdigest()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("cid,arch,opts", _cases(), ids=[c[0] for c in _cases()])
def test_plans_match_golden(golden, cid, arch, opts):
    assert sorted(golden[cid]) == sorted(s for s, _ in SPECS)
    for sid, spec in SPECS:
        lines = _plan(arch, opts, spec)
        if _sha(lines) != golden[cid][sid]:
            print(f"{cid} {sid}: current plan")
            for line in lines:
                print("  ", line)
        assert _sha(lines) == golden[cid][sid], f"{cid} {sid}: the plan differs from the recorded one"


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump({cid: {sid: _sha(_plan(arch, opts, spec)) for sid, spec in SPECS} for cid, arch, opts in _cases()},
                  f, indent=0)
        f.write("\n")

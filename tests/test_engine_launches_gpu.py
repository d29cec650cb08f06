"""The launches of the engine, pinned: every case of launch_trace.CASES issues the launches recorded in
tests/golden/engine_attn_launches.json — the same entry points in the same order with the same canonical arguments (owner and byte
offset of every buffer, shapes, strides, scalars, descriptor tables field by field, the reduce table entry by entry).

The golden was recorded by tools/record_engine_launches.py on the commit BEFORE the engine's attention host code was folded into one
operand record and one argument builder; a refactor of engine.py that is meant to change no launch must leave this test passing with
the file untouched.  A change that is meant to alter launches records a new file on purpose and says so.

The inference cases compare the whole generate() call: its three decode steps end at the length cap (max_len = 3), not at a value
computed on the device."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_trace as lt  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    made = {}
    yield made
    made.clear()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "engine_attn_launches.json")) as f:
        return json.load(f)


def test_golden_holds_every_case(golden):
    assert sorted(golden) == sorted(lt.CASES)


@pytest.mark.parametrize("case", lt.CASES)
def test_launches_match_the_recorded_trace(engines, golden, case):
    rec = lt.record_case(case, engines)
    lt.check_routes(case, rec)
    assert rec.unowned == lt.UNOWNED.get(case, 0), f"case {case}: {rec.unowned} arguments that no owner contains"
    got, want = rec.digest(), golden[case]
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print(f"case {case}: launch {i} differs: recorded {w}, now {g}")
            print(json.dumps(rec.launches[i], indent=1))
            pytest.fail(f"case {case}: launch {i} ({g[0]}, recorded as {w[0]}) differs from the recorded trace")
    assert len(got) == len(want), f"case {case}: {len(got)} launches, {len(want)} recorded; first extra: {max(got, want, key=len)[min(len(got), len(want))]}"

#!/usr/bin/env python3
"""Record tests/golden/tail_parent_digests.json: a SHA-256 (with shape and dtype) of every output of the forward sub-layer tail launches
of tests/test_tail_kernels_gpu.py (tail_forward_digests: kk_sublayer_out_fwd and kk_linear_tail_fwd), on an MI355X.  Run it on the tree
BEFORE a change to csrc/kk_tail.h or its callers that is meant to keep the bits; a change that moves them on purpose records again and
says so.  The encoder stack's use of the same arithmetic is pinned by tools/record_encstack_golden.py.
    python tools/record_tail_golden.py COMMIT [output.json]        (COMMIT: the name of the commit the tree is at, kept in the file)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_tail_kernels_gpu as t  # noqa: E402
from kokoro_ruslan_amd import lib  # noqa: E402

commit, path = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else t.GOLDEN
lib.load()
cases = t.tail_forward_digests(lib)
with open(path, "w") as f:
    json.dump({"commit": commit, "cases": cases}, f, indent=0, sort_keys=True)
    f.write("\n")
print(f"recorded at {commit}: {len(cases)} launches, {sum(len(c) for c in cases.values())} tensors -> {path} ({os.path.getsize(path)} bytes)")

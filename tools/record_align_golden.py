#!/usr/bin/env python3
"""Record tests/golden/align_parent_mix_outputs.npz: every result of tests/test_align_unified_gpu.py's outputs() (public methods of
PhoneAligner only) on an MI355X.  Run it on the tree BEFORE a change to csrc/kk_align.hip or align.py that is meant to keep the bits; a
change that moves them on purpose records again and says so.
    python tools/record_align_golden.py COMMIT [output.npz]        (COMMIT: the name of the commit the tree is at, kept in the file)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import test_align_unified_gpu as t  # noqa: E402

commit, path = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else t.PARENT
fx = t.fixture_of(t.outputs(), commit)
np.savez_compressed(path, **fx)
print(f"{len(fx['names'])} results ({len(fx) - 3} also raw), recorded at {commit} -> {path} ({os.path.getsize(path)} bytes)")

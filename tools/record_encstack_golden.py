#!/usr/bin/env python3
"""Record tests/golden/encstack_parent_digests.json: a SHA-256 (with shape and dtype) of every tensor the fused text-encoder forward
leaves behind, for the cases of tests/test_encstack_gpu.py (DIGEST_CASES), on an MI355X.  Run it on the tree BEFORE a change to
csrc/kk_encstack.hip or to the code it shares with the library that is meant to keep the bits; a change that moves them on purpose
records again and says so.  Both workgroup placements must give the same bits.  For the dropout cases the seed is the first one
from 77 up at which a sub-layer tail past the first layer drops one sample of the batch and keeps another (DropPath's row / S).
    python tools/record_encstack_golden.py COMMIT [output.json]        (COMMIT: the name of the commit the tree is at, kept in the file)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_encstack_gpu as t  # noqa: E402
from kokoro_ruslan_amd import engine, spec, synthetic  # noqa: E402

commit, path = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else t.GOLDEN
mods, engines, cases = (engine, spec, synthetic), {}, {}
for case, (kw, B, T, P, ragged, dropout) in t.DIGEST_CASES.items():
    layers = spec.ModelDims(**kw).enc_layers
    for seed in range(77, 177):
        got = t.fused_encoder_tensors(mods, engines, case, 0, seed)
        if not dropout or t.droppath_is_exercised(got, layers, B):
            break
    else:
        raise SystemExit(f"{case}: no seed in [77, 177) drops one sample and keeps another")
    tensors = {k: t._digest(v) for k, v in got.items()}
    other = {k: t._digest(v) for k, v in t.fused_encoder_tensors(mods, engines, case, 1, seed).items()}
    assert tensors == other, f"{case}: the two placements differ in {[k for k in tensors if tensors[k] != other[k]]}"
    cases[case] = {"seed": seed, "tensors": tensors}
    print(f"{case}: seed {seed}, {len(tensors)} tensors")
with open(path, "w") as f:
    json.dump({"commit": commit, "cases": cases}, f, indent=0, sort_keys=True)
    f.write("\n")
print(f"recorded at {commit} -> {path} ({os.path.getsize(path)} bytes)")

#!/usr/bin/env python3
"""Record tests/golden/gemm_routes.json: the kernel each bf16 GEMM entry point launches, and the SHA-256 of what it leaves where the
launch has no k-slices, for every case of tests/test_gemm_routes_gpu.py (public entry points only).  Run it on the tree BEFORE a
change to the host dispatch of kk_gemm16.hip that is meant to keep the routes; a change that moves a route on purpose records again
and says so.
    python tools/record_gemm_routes.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_gemm_routes_gpu as t  # noqa: E402
from kokoro_ruslan_amd import lib as kk  # noqa: E402

routes = {t.case_id(c): t.run_case(kk, c) for c in t.CASES}
with open(t.GOLDEN_FILE, "w") as f:
    json.dump(routes, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(routes)} cases -> {t.GOLDEN_FILE}")

#!/usr/bin/env python
"""Record the launch-trace golden of the engine (tests/golden/engine_attn_launches.json) on an MI355X.

    python tools/record_engine_launches.py [--out PATH] [--full PATH.json.gz] [--cases a,b,...]

Run it on the commit whose launches are to be pinned — the PARENT of a refactor of engine.py, never the refactored tree: the test
(tests/test_engine_launches_gpu.py) replays the same cases and compares.  Per case the file holds [entry point, first 16 hex digits
of the SHA-256 of the canonical arguments] of every launch of the call (tests/launch_trace.py says what is canonical).  Each case is
checked to take the route it is there for (launch_trace.ROUTES) before anything is written.  --full also keeps the canonical
arguments themselves (gzip), for reading a difference without a GPU."""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import launch_trace as lt  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "engine_attn_launches.json"))
    ap.add_argument("--full", default=None)
    ap.add_argument("--cases", default=None)
    a = ap.parse_args()
    cases = a.cases.split(",") if a.cases else lt.CASES
    engines, golden, full, bad = {}, {}, {}, []
    for case in cases:
        t0 = time.time()
        rec = lt.record_case(case, engines)
        try:
            lt.check_routes(case, rec)
        except AssertionError as e:
            bad.append(str(e))
        if rec.unowned != lt.UNOWNED.get(case, 0):
            bad.append(f"case {case}: {rec.unowned} arguments that no owner contains, launch_trace.UNOWNED says {lt.UNOWNED.get(case, 0)}")
        golden[case], full[case] = rec.digest(), rec.launches
        print(f"{case}: {len(rec.launches)} launches, {rec.unowned} unowned addresses, {time.time() - t0:.1f} s", flush=True)
    if a.full:
        with gzip.open(a.full, "wt") as f:
            json.dump(full, f)
    for msg in bad:
        print("ROUTE:", msg)
    if bad:
        return 1
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(c)}: {json.dumps(golden[c], separators=(',', ':'))}" for c in golden) + "\n}\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

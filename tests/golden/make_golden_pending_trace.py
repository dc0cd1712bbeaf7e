#!/usr/bin/env python3
"""Record tests/golden/pending_trace.json: for every scripted call sequence of tests/pending_trace.py the state of the four
unstored-row records (mgrit_hip_deferred, mgrit_hip_twin, mgrit_hip_lagged, mgrit_hip_up2_pending) behind every library call, and
a SHA-256 digest of the u, v and g slabs of every level behind a settle of every level (pending_trace.pack says how the file is laid out). Needs a GPU and the built library.
tests/test_hip_pending_trace.py replays every script and compares with equality.

The file is the record of the host-side decisions of the commit it was made on: record it BEFORE a change that is meant to keep them
(a refactor of the bookkeeping), commit it unchanged with the change. It names the hipcc it was made with: the slab digests are
device arithmetic, which a new compiler may move without any change to the sources.

Usage:  python tests/golden/make_golden_pending_trace.py [output file]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    sys.path.insert(0, p)

import pending_trace as pt  # noqa: E402
from periodic2d_bits import hipcc_version  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else pt.GOLDEN_FILE
    results = {}
    for case in pt.CASES:
        got = results[pt.case_id(case)] = pt.run_case(case)
        print(f"{pt.case_id(case)}: {got['calls']} calls, {len(got['changes'])} changes", flush=True)
    pt.dump(pt.pack(hipcc_version(), results), out)


if __name__ == "__main__":
    main()

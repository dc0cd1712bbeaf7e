#!/usr/bin/env python3
"""Record tests/golden/periodic2d_bits.json: SHA-256 digests of what the periodic 2-D device paths (Allen-Cahn IMEX and Newton-PCG,
Gray-Scott IMEX and Newton-BiCGStab, Cahn-Hilliard, Burgers, Navier-Stokes and Ginzburg-Landau IMEX) leave in the u, v and g slabs after every sweep of the fixed cases of tests/periodic2d_bits.py, on seeded inputs.
Needs a GPU and the built library. tests/test_hip_periodic2d_bits.py recomputes every digest and compares with equality.

The file is the record of the device arithmetic of the commit it was made on: record it BEFORE a change that is meant to keep the bits
(a refactor of the kernels, a compiler flag), commit it unchanged with the change. It names the hipcc it was made with; a new compiler
may move the bits without any change to the sources, and the test says so when it fails.

Usage:  python tests/golden/make_golden_periodic2d_bits.py [output file]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    sys.path.insert(0, p)

import periodic2d_bits as bits  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else bits.GOLDEN_FILE
    rec = {"hipcc": bits.hipcc_version(), "cases": {}}
    for name in bits.CASES:
        rec["cases"][name] = bits.run_case(name)
        print(f"{name}: {len(rec['cases'][name]['digests'])} digests", flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

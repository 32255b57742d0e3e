#!/usr/bin/env python3
"""Generates tests/golden/route_b_reference_declarations.json: every `void XxxCUDA(...);` declaration of the reference's
B/kernels.h as tests/test_cpu_route_b.py parses it -- the sha256 of its normalised parameter list (types, names, order, default
values) and the line range it occupies.  The header is read where it lies in the reference tree; only the digests and line
numbers are committed, so tests/test_cpu_route_b.py::test_signatures_follow_the_reference_header runs without that tree.

Run:  python scripts/make_golden_route_b.py <root of the reference tree>
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_cpu_route_b import _declarations   # noqa: E402  (the parser the test uses)

HEADER = "applications/badslam/src/badslam/kernels.h"
OUT = os.path.join(ROOT, "tests", "golden", "route_b_reference_declarations.json")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    text = open(os.path.join(sys.argv[1], HEADER)).read()
    table = {name: {"params_sha256": hashlib.sha256(params.encode()).hexdigest(), "lines": [first, last]}
             for name, (params, first, last) in sorted(_declarations(text).items())}
    with open(OUT, "w") as f:
        json.dump({"header": "B/kernels.h", "declarations": table}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} declarations -> {os.path.relpath(OUT, ROOT)}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Record tests/golden/temporal_abi_status.json from the library built in the tree: the answers of the flagged C ABI's host side to
the cases of tests/test_temporal_abi_status.py.  Run it on a build whose answers are the ones to keep (no GPU needed)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "activesparseshifts-pytorch_amd"), os.path.dirname(HERE)):
    sys.path.insert(0, p)

import test_temporal_abi_status as T  # noqa: E402

listed = T.cases()
rows = [T.answers(c) for c in listed]
with open(T.GOLDEN, "w") as f:
    f.write('{"cases_sha256": "%s",\n "rows": [\n' % T.digest(listed))
    f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
    f.write("\n]}\n")
print(len(rows), "rows ->", T.GOLDEN)

#!/usr/bin/env python3
"""Generate tests/golden/reference_citations.json: what tests/test_citations.py needs to know about the reference tree.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_citations_golden.py <reference checkout>

For every file of the reference whose name a boundary document cites (include/quest_hip.h, INTEGRATION.md,
examples/pybind_binding.cpp): its path in the tree, its number of lines, and for each identifier the documents pin to
a citation of that file, the numbers of the lines it occurs on.  Names and numbers only -- no text of the reference.
Rerun it after adding or changing a citation.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import test_citations as tc  # noqa: E402  (the citation parser the test uses)


def main(ref):
    ref = os.path.abspath(ref)
    cited = {}  # path as cited -> identifiers pinned to it
    for doc in tc.DOCS:
        text = open(os.path.join(ROOT, doc)).read()
        for path, _a, _b, symbol, _off in tc._citations(text):
            syms = cited.setdefault(path, set())
            if symbol and ("_" in symbol or re.search(r"[a-z][A-Z]", symbol)) and not symbol.isupper():
                syms.add(symbol.split("::")[-1])
    by_name = {}
    for d, _, names in os.walk(ref):
        if "/.git" in d:
            continue
        for n in names:
            by_name.setdefault(n, []).append(os.path.relpath(os.path.join(d, n), ref))
    files = {}
    for path, syms in sorted(cited.items()):
        for rel in by_name.get(os.path.basename(path), []):
            with open(os.path.join(ref, rel), errors="replace") as f:
                lines = f.read().splitlines()
            rec = files.setdefault(rel, {"lines": len(lines), "symbols": {}})
            for s in sorted(syms):
                rec["symbols"][s] = [i + 1 for i, l in enumerate(lines) if s in l]
    out = os.path.join(HERE, "reference_citations.json")
    with open(out, "w") as f:
        json.dump({"files": dict(sorted(files.items()))}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, len(files), "files")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])

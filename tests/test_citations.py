"""Every `file:line` citation of the boundary documents resolves against the reference tree.

`include/quest_hip.h` and `INTEGRATION.md` tell a maintainer which reference declaration each C-ABI entry replaces.  A
citation that points at the wrong lines is worse than none, and nobody re-reads them by hand: this test does, against
tests/golden/reference_citations.json -- the cited reference files' paths, line counts and the lines each pinned identifier
occurs on, recorded from a reference checkout by tests/golden/make_citations_golden.py (rerun it after changing a citation).

Checked for every citation `path/file.ext:A` or `:A-B` (and the `:C-D` continuations that follow it):
  * the file exists in the reference tree (by its path suffix; a bare basename must be unique or one candidate must fit),
  * the line range lies inside the file,
and, where the text names the symbol the citation is about -- `symbol (file:A-B`, `-> Symbol, file:A-B` --
  * that symbol occurs inside the cited lines.
"""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_citations.json")
DOCS = ["include/quest_hip.h", "INTEGRATION.md", "examples/pybind_binding.cpp"]

CITE = re.compile(r"(?P<path>(?:[\w.-]+/)*[\w-]+\.(?:cuh|cu|h|py|sh|md|cmake|txt)):(?P<a>\d+)(?:-(?P<b>\d+))?")
CONT = re.compile(r"\s*(?:,|/|and|kernel|launch|math|planner|aux|dispatch)?\s*:(\d+)(?:-(\d+))?")
# the symbol a citation is about: `symbol (file:..`  |  `-> Symbol, file:..`  |  `Symbol, file:..` after an arrow
SYMBOL_BEFORE = re.compile(r"(?:->\s*)?([A-Za-z_][\w:]*)\s*(?:\(|,)\s*$")
DEFINITION_AFTER = re.compile(r"(?://[^\n]*\n)*(?:torch::Tensor|void|class|static \w+)\s+(\w+)")
# per document: at least this many citations / symbol-pinned citations must be found (the parser still works)
EXPECT = {"include/quest_hip.h": (20, 8), "INTEGRATION.md": (12, 0), "examples/pybind_binding.cpp": (8, 7)}
OWN_FILES = {"quest_hip.h", "INTEGRATION.md", "DESIGN.md", "SURVEY.md", "BASELINE.md", "VERDICT.md", "bench.py"}


def _index():
    """basename -> [(path in the reference tree, its record: line count + the lines each pinned identifier occurs on)]"""
    with open(FIXTURE) as f:
        recorded = json.load(f)["files"]
    files = {}
    for rel, rec in recorded.items():
        files.setdefault(os.path.basename(rel), []).append(("/" + rel, rec))
    return files


def _candidates(index, path):
    base = os.path.basename(path)
    return [f for f in index.get(base, []) if f[0].endswith("/" + path) or "/" not in path]


def _n_lines(cand):
    return cand[1]["lines"]


def _occurs(cand, symbol, a=1, b=None):
    """Does `symbol` occur on a line of the range a..b of the file (whole file: b None)?  An identifier the fixture does
    not record for the file fails the test: rerun tests/golden/make_citations_golden.py."""
    lines = cand[1]["symbols"].get(symbol)
    assert lines is not None, f"{cand[0]}: `{symbol}` not recorded in {os.path.relpath(FIXTURE, ROOT)}"
    return any(a <= n <= (b if b is not None else n) for n in lines)


def _citations(text):
    """(path, first line, last line, symbol or None, offset) for every citation of `text`, continuations included."""
    for m in CITE.finditer(text):
        path = m.group("path")
        if os.path.basename(path) in OWN_FILES or os.path.exists(os.path.join(ROOT, path)):
            continue  # a file of this repo, not of the reference
        before = text[max(0, m.start() - 80):m.start()].replace("\n * ", " ").replace("\n", " ")
        sym = SYMBOL_BEFORE.search(before)
        symbol = sym.group(1) if sym else None
        if symbol is None and before.rstrip().endswith("//"):
            # examples/pybind_binding.cpp: `// bsk_ops.h:A-B` on the line above the definition it mirrors
            nxt = DEFINITION_AFTER.match(text, text.find("\n", m.end()) + 1)
            symbol = nxt.group(1) if nxt else None
        a, b = int(m.group("a")), int(m.group("b") or m.group("a"))
        yield path, a, b, symbol, m.start()
        pos = m.end()
        while True:  # `, kernel :398-449` / `, :136` style continuations refer to the same file
            c = CONT.match(text, pos)
            if not c or text[pos:c.end()].count("\n") > 1:
                break
            yield path, int(c.group(1)), int(c.group(2) or c.group(1)), None, c.start()
            pos = c.end()


@pytest.mark.parametrize("doc", DOCS)
def test_every_citation_resolves_and_names_its_symbol(doc):
    index = _index()
    text = open(os.path.join(ROOT, doc)).read()
    problems, n_checked, n_symbols = [], 0, 0
    for path, a, b, symbol, off in _citations(text):
        line_no = text.count("\n", 0, off) + 1
        cands = _candidates(index, path)
        if not cands:
            problems.append(f"{doc}:{line_no}: {path}:{a}-{b}: no such file in the reference")
            continue
        fits = [c for c in cands if 1 <= a <= b <= _n_lines(c)]
        if not fits:
            problems.append(f"{doc}:{line_no}: {path}:{a}-{b}: outside the file ({[_n_lines(c) for c in cands]} lines)")
            continue
        n_checked += 1
        # a code identifier (snake_case or CamelCase), not the English word that happens to precede a parenthesis
        if symbol and ("_" in symbol or re.search(r"[a-z][A-Z]", symbol)) and not symbol.isupper():
            plain = symbol.split("::")[-1]
            hit = any(_occurs(c, plain, a, b) for c in fits)
            # only symbols the reference file knows at all are pinned to the range (the sentence may name one of OUR
            # functions in front of a citation that explains it)
            known = any(_occurs(c, plain) for c in fits)
            if known:
                n_symbols += 1
                if not hit:
                    where = [n for c in fits for n in c[1]["symbols"][plain]][:6]
                    problems.append(f"{doc}:{line_no}: `{plain}` is not inside {path}:{a}-{b} (it occurs at lines {where})")
    assert not problems, "\n".join(problems)
    assert n_checked >= EXPECT[doc][0] and n_symbols >= EXPECT[doc][1], (n_checked, n_symbols)

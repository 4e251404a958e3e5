"""Every `path:line[-line]` citation of a reference file in the sources, headers and documents names an existing file of the
reference checkout and a line range inside it.  The reference's file list and line counts are a committed fixture
(tests/golden/reference_line_counts.json, written by tests/golden/make_golden.py): nothing else of it is read."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LINES = os.path.join(ROOT, "tests", "golden", "reference_line_counts.json")
PAT = re.compile(r"([A-Za-z_][\w/\.]*\.(?:py|yaml|sh)):(\d+)(?:-:?(\d+))?")
OURS = ("tests/", "scripts/", "cotnet_amd/", "oracle/", "profiles/", "bench", "__graft")
NOT_OURS = ("SURVEY", "VERDICT", "ADVICE", "PAPERS", "SNIPPETS", "BASELINE")


def test_reference_citations_resolve():
    with open(REF_LINES) as fh:
        lines = json.load(fh)  # {path inside the reference: number of lines}
    by_name = {}
    for p in lines:
        by_name.setdefault(os.path.basename(p), []).append("/" + p)

    def nlines(p):
        return lines[p[1:]]

    tracked = subprocess.run(["git", "ls-files", "*.py", "*.md", "*.h", "*.hip", "*.c", "*.sh"], cwd=ROOT, capture_output=True,
                             text=True).stdout.split()
    if not tracked:  # (a copy of the tree without git: the project's own directories and top-level files)
        exts = (".py", ".md", ".h", ".hip", ".c", ".sh")
        tracked = [f for f in os.listdir(ROOT) if f.endswith(exts)]
        for top in ("cotnet_amd", "include", "oracle", "profiles", "scripts", "tests"):
            for d, dirs, fs in os.walk(os.path.join(ROOT, top)):
                dirs[:] = [x for x in dirs if not x.startswith((".", "_")) and x != "build"]
                tracked += [os.path.relpath(os.path.join(d, f), ROOT) for f in fs if f.endswith(exts)]
    checked, bad = 0, []
    for s in tracked:
        if s.startswith(NOT_OURS):
            continue
        with open(os.path.join(ROOT, s), errors="replace") as fh:
            txt = fh.read()
        for m in PAT.finditer(txt):
            path, last = m.group(1), int(m.group(3) or m.group(2))
            base = os.path.basename(path)
            if os.path.exists(os.path.join(ROOT, path)) or path.startswith(OURS):
                continue
            cands = [p for p in by_name.get(base, []) if p.endswith("/" + path)] or ([] if "/" in path else by_name.get(base, []))
            if not cands:
                continue  # (our own files cited by base name, abbreviations like `mix.py`)
            checked += 1
            if not any(last <= nlines(c) for c in cands):
                bad.append((s, m.group(0)))
    assert checked > 200 and not bad, (checked, bad[:10])

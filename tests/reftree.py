"""Stand-ins for the three reference files the Haskell patches edit (app/Main.hs, src/Scene/World.hs, tracer.cabal), so the patch
tests run from this repository alone.  tests/golden/reference_lines.json holds one fingerprint per line of each file (the first 16 hex
digits of the SHA-256 of the line without its newline), never the text.  A stand-in has the original's line count; a line whose text
occurs somewhere in the repository's own diffs (context, removed or added) is that text, every other line is an opaque token made
from its fingerprint.  Equal lines stay equal and different lines stay different, so patch(1) accepts, fuzzes or offsets a hunk on
a stand-in exactly as it would on the original.

Regenerate the fixture from a checkout of the reference:  python tests/reftree.py <reference tree> > tests/golden/reference_lines.json
"""
import glob
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_lines.json")
HASKELL = os.path.join(ROOT, "haskell-path-tracer_amd", "haskell")
FILES = ("app/Main.hs", "src/Scene/World.hs", "tracer.cabal")


def fingerprint(line):
    return hashlib.sha256(line.encode("utf-8")).hexdigest()[:16]


def known_lines():
    """Every line of a hunk body of every diff under haskell/ (what the repository already holds)."""
    lines = set()
    for diff in glob.glob(os.path.join(HASKELL, "**", "*.diff"), recursive=True):
        for line in open(diff, encoding="utf-8").read().split("\n"):
            if line[:1] in (" ", "-", "+") and not line.startswith(("--- ", "+++ ")):
                lines.add(line[1:])
            elif line == "":
                lines.add("")
    return {fingerprint(line): line for line in lines}


def stand_in(rel):
    """The text of the stand-in for reference file `rel`."""
    prints = json.load(open(FIXTURE))["files"][rel]
    known = known_lines()
    return "".join(known.get(p, "<reference line %s>" % p) + "\n" for p in prints)


def write_tree(dest, files=FILES):
    for rel in files:
        path = os.path.join(str(dest), rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w", encoding="utf-8") as f:
            f.write(stand_in(rel))


if __name__ == "__main__":
    tree = sys.argv[1]
    out = {"format": "sha256(line without newline)[:16], one per line; every file ends in a newline", "files": {}}
    for rel in FILES:
        text = open(os.path.join(tree, rel), encoding="utf-8").read()
        assert text.endswith("\n") and "\r" not in text, rel
        out["files"][rel] = [fingerprint(line) for line in text[:-1].split("\n")]
    json.dump(out, sys.stdout, indent=0)
    sys.stdout.write("\n")

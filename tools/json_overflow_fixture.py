"""Builds tests/golden/json_overflow_v135.json.gz (tooling): yjs's answer (tools/json_corpus.js --states: the image's
yjs 13.5.16 bundle, y-prosemirror restated) for every by-construction document of tests/json_overflow_docs.py -- its
root and the absent name -- and for the tool's own boundary sessions, which carry their states.

    python tools/json_overflow_fixture.py OUT.json.gz"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "tests/json_overflow_docs.py unique() through tools/json_corpus.js --states (yjs 13.5.16 bundle) via tools/json_overflow_fixture.py"


def build(out):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import json_overflow_docs
    states = []
    for d in json_overflow_docs.unique():      # (a document asked twice, by its root and by an absent name, is one state)
        if d.u.hex() not in states:
            states.append(d.u.hex())
    with tempfile.TemporaryDirectory() as t:
        a = os.path.join(t, "in.json")
        with open(a, "w") as f:
            json.dump({"source": SOURCE, "states": states}, f)
        subprocess.run(["node", os.path.join(ROOT, "tools", "json_corpus.js"), "--states", a, out], check=True, stdout=subprocess.DEVNULL)


def text(path):
    """The fixture's JSON text (what regenerating must reproduce byte for byte)."""
    return gzip.open(path, "rb").read()


if __name__ == "__main__":
    build(sys.argv[1])
    doc = json.loads(text(sys.argv[1]))
    print(len(doc["states"]), "states", len(doc["sessions"]), "sessions", os.path.getsize(sys.argv[1]), "bytes")

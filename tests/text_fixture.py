"""The plain-text fixture (tests/golden/text_v135.json.gz, tools/text_corpus.js) for the text tests.

A set's row i holds the roots of row i of its input fixture -- the states are read from there, not stored twice --
as [name, flat, deep] hex triples; the edge sessions carry their own states.  expectations() flattens everything
into (label, state, name, flat, deep) rows, every one of which yjs answered (no row is a refusal)."""
import gzip
import hashlib
import json
import os
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = os.path.join(GOLDEN, "text_v135.json.gz")
SETS = ("snapshot_v135", "snapshot_text_v135", "snapshot_pending_v135", "snapshot_subdoc_v135")

_cache = {}


def load():
    if "fix" not in _cache:
        _cache["fix"] = json.load(gzip.open(FIX, "rt"))
    return _cache["fix"]


def input_sha256(name):
    return hashlib.sha256(open(os.path.join(GOLDEN, name), "rb").read()).hexdigest()


def set_states(name):
    """The states (the `u` of every row) of an input fixture."""
    if name not in _cache:
        rows = json.load(gzip.open(os.path.join(GOLDEN, name + ".json.gz"), "rt"))["rows"]
        _cache[name] = [bytes.fromhex(r[0]) for r in rows]
    return _cache[name]


def expectations(sets=SETS, edges=True):
    """[(label, state, name, flat, deep)] over the given sets and the edge sessions."""
    fix = load()
    out = []
    for s in sets:
        states = set_states(s)
        for i, roots in enumerate(fix["sets"][s]):
            for nm, flat, deep in roots:
                out.append((f"{s}[{i}]", states[i], bytes.fromhex(nm), bytes.fromhex(flat), bytes.fromhex(deep)))
    if edges:
        for e in fix["edges"]:
            st = bytes.fromhex(e["state"])
            for nm, flat, deep in e["roots"]:
                out.append((e["note"], st, bytes.fromhex(nm), bytes.fromhex(flat), bytes.fromhex(deep)))
    return out


def write_asks(path, asks):
    """tools/snapdev/textdev.cpp's input: asks = [(state, name, mode)]."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(asks)))
        for st, nm, mode in asks:
            f.write(struct.pack("<I", len(st)) + st + struct.pack("<I", len(nm)) + nm + struct.pack("<I", mode))


def read_textdev(path):
    """textdev's output: [(flat tier, flat bytes, general status, general bytes)]."""
    b = open(path, "rb").read()
    i, out = 0, []
    while i < len(b):
        tier, fl = struct.unpack_from("<iI", b, i)
        i += 8
        fb = b[i:i + fl]
        i += fl
        gs, gl = struct.unpack_from("<iI", b, i)
        i += 8
        out.append((tier, fb, gs, b[i:i + gl]))
        i += gl
    return out

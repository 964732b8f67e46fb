"""The toJSON fixture (tests/golden/tojson_v135.json.gz, tools/tojson_corpus.js) for the ygm_tojson_v1 tests.

A set's row i holds the asks of row i of its input fixture -- the states are read from there, not stored twice -- as
[name hex, kind, status, json hex] for the first fix["full"] states and [name hex, kind, status, sha256(json), length]
after them; the edge sessions and the seeded random sessions carry their own states and full bytes.  expectations()
flattens everything into (label, state, name, kind, status, json bytes or None, sha256, length) rows: serialized roots
(status 0) and refusals."""
import gzip
import hashlib
import json
import os
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = os.path.join(GOLDEN, "tojson_v135.json.gz")
SETS = ("snapshot_v135", "snapshot_text_v135", "snapshot_pending_v135", "snapshot_subdoc_v135", "snapshot_nogc_v135")
MAP, ARRAY, TEXT = 0, 1, 2
ST_MORE = 65   # ygm_json.hpp's internal ST_JSON_MORE: never a result

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


def _row(label, state, r):
    if len(r) == 4:
        b = bytes.fromhex(r[3])
        return (label, state, bytes.fromhex(r[0]), r[1], r[2], b, hashlib.sha256(b).hexdigest(), len(b))
    return (label, state, bytes.fromhex(r[0]), r[1], r[2], None, r[3], r[4])


def expectations(sets=SETS, edges=True, random=True):
    key = ("exp", tuple(sets), edges, random)
    if key not in _cache:
        fix = load()
        out = []
        for s in sets:
            states = set_states(s)
            for i, asks in enumerate(fix["sets"][s]):
                out.extend(_row(f"{s}[{i}]", states[i], r) for r in asks)
        if random:
            for e in fix["random"]:
                st = bytes.fromhex(e["state"])
                out.extend(_row(f"random {e['seed']}", st, r) for r in e["asks"])
        if edges:
            for e in fix["edges"]:
                st = bytes.fromhex(e["state"])
                out.extend(_row(e["note"], st, r) for r in e["asks"])
        _cache[key] = out
    return _cache[key]


def edge(note, i=0):
    """(state, name, kind, json bytes, status) of ask i of a named edge session."""
    for e in load()["edges"]:
        if e["note"] == note:
            r = e["asks"][i]
            return bytes.fromhex(e["state"]), bytes.fromhex(r[0]), r[1], bytes.fromhex(r[3]), r[2]
    raise KeyError(note)


def matches(row, status, data):
    """Does (status, bytes) equal the row's expectation?  Refusals give no bytes."""
    st, b, sha, ln = row[4:8]
    if status != st:
        return False
    if st != 0:
        return len(data) == 0
    return len(data) == ln and (data == b if b is not None else hashlib.sha256(data).hexdigest() == sha)


def write_asks(path, asks):
    """tools/snapdev/tojsondev.cpp's input: asks = [(state, name, kind)]."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(asks)))
        for st, nm, kind in asks:
            f.write(struct.pack("<I", len(st)) + st + struct.pack("<I", len(nm)) + nm + struct.pack("<I", kind))


def read_tojsondev(path):
    """tojsondev's output: [(status, reran, bytes)]."""
    b = open(path, "rb").read()
    i, out = 0, []
    while i < len(b):
        st, re, ln = struct.unpack_from("<iII", b, i)
        i += 12
        out.append((st, re, b[i:i + ln]))
        i += ln
    return out

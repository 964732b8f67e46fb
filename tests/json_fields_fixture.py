"""The keyed-object fixture (tests/golden/json_fields_v135.json.gz, tools/json_fields_corpus.js) for the tests of
ygm_json_fields_v1.

A set's row i holds the asks of row i of its input fixture -- the states are read from there, not stored twice -- as
[fields, status, json hex] for the first fix["full"] rows and [fields, status, sha256(json), length] after them, where
fields is None (every key of doc.share) or the listed names (hex) in list order; `keys` are the state's share keys in
the order its all-fields object has them.  The edge sessions carry their own states and full bytes.  rows() flattens
everything into Row tuples; matches() is json_fixture's."""
import collections
import gzip
import hashlib
import json
import os

import json_fixture as jf

FIX = os.path.join(jf.GOLDEN, "json_fields_v135.json.gz")
SETS = jf.SETS
EMPTY_DOC = b'{"type":"doc","content":[]}'

# label, state, fields (None or [bytes]), status, json (bytes or None), sha256, length -- json_fixture.matches' layout --
# then the state's keys ([bytes], output order)
Row = collections.namedtuple("Row", "label state fields status json sha length keys")

_cache = {}


def load():
    if "fix" not in _cache:
        _cache["fix"] = json.load(gzip.open(FIX, "rt"))
    return _cache["fix"]


def _row(label, state, keys, r):
    fields = None if r[0] is None else [bytes.fromhex(h) for h in r[0]]
    if len(r) == 3:
        b = bytes.fromhex(r[2])
        return Row(label, state, fields, r[1], b, hashlib.sha256(b).hexdigest(), len(b), keys)
    return Row(label, state, fields, r[1], None, r[2], r[3], keys)


def rows(sets=SETS, edges=True):
    key = ("rows", tuple(sets), edges)
    if key not in _cache:
        fix = load()
        out = []
        for s in sets:
            states = jf.set_states(s)
            for i, e in enumerate(fix["sets"][s]):
                keys = [bytes.fromhex(h) for h in e["keys"]]
                out.extend(_row(f"{s}[{i}]", states[i], keys, r) for r in e["asks"])
        if edges:
            for e in fix["edges"]:
                st = bytes.fromhex(e["state"])
                keys = [bytes.fromhex(h) for h in e["keys"]]
                out.extend(_row(e["note"], st, keys, r) for r in e["asks"])
        _cache[key] = out
    return _cache[key]


def edge(note):
    """The Rows of a named edge session, in the order of its asks."""
    got = [r for r in rows(sets=(), edges=True) if r.label == note]
    if not got:
        raise KeyError(note)
    return got


def matches(row, status, data):
    return jf.matches(tuple(row[:7]), status, data)


def field_lists(rs):
    """The encoded field lists of Rows (hocuspocus_amd.engine.encode_fields: importable without the library)."""
    from hocuspocus_amd.engine import encode_fields
    return [encode_fields(r.fields) for r in rs]

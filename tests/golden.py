"""Loader for the committed golden fixtures (tests/golden/*).

yjs13516_vectors.jsonl.gz -- made by tests/golden/gen/gen_fixtures.js from
yjs 13.5.16 (the copy JupyterLab bundles in the build image); see SURVEY.md §8c.
Each case: op in {merge, diff, sv}, hex inputs, hex `out` (None when yjs threw)
and `err` (yjs's exception text).
"""
import functools
import gzip
import json
import os

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# yjs throws on these; any engine error status is an acceptable equivalent.
THROW_STATUSES = {1, 2, 4, 5}  # EMALFORMED, ERANGE, ESURROGATE, EDEPTH
# Edge-family notes whose content yjs re-encodes; the
# engine may refuse them with ENONCANON instead of normalising.
NONCANON_NOTES = ("any ", "json ", "embed non-canonical", "format non-canonical", "doc {gc:true}")


def load_yjs_vectors():
    with gzip.open(os.path.join(HERE, "yjs13516_vectors.jsonl.gz")) as f:
        lines = f.read().decode().splitlines()
    header = json.loads(lines[0])
    cases = [json.loads(l) for l in lines[1:]]
    assert header["count"] == len(cases)
    return header, cases


def load_v8_sort_vectors():
    with gzip.open(os.path.join(HERE, "v8_timsort_vectors.json.gz")) as f:
        return json.loads(f.read())


def case_inputs(c):
    if c["op"] == "merge":
        return [bytes.fromhex(x) for x in c["in"]]
    if c["op"] == "diff":
        return bytes.fromhex(c["update"]), bytes.fromhex(c["sv"])
    return bytes.fromhex(c["update"])


def check_result(c, status, out):
    """Returns None if (status, out) is an acceptable answer for golden case c, else a reason."""
    exp = c["out"]
    if exp is None:
        return None if status in THROW_STATUSES else f"yjs threw ({c['err']}) but got status {status}"
    if status == 0:
        return None if out.hex() == exp else f"bytes differ:\n exp {exp}\n got {out.hex()}"
    if status == 3 and c["family"] == "edge" and (c.get("note") or "").startswith(NONCANON_NOTES):
        return None
    return f"status {status} but yjs returned {exp}"


def ds_to_desc(update_hex):
    """Rewrites an output's delete set into client-descending order (yjs 13.6.x writeDeleteSet)."""
    from v1util import ds_offset, encode_ds, read_ds
    b = bytes.fromhex(update_hex)
    p = ds_offset(b)
    ds, _ = read_ds(b, p)
    return (b[:p] + encode_ds(sorted(ds, key=lambda e: -e[0]))).hex()


# ---------------------------------------------------------------------------------------- stored documents
# (what each file holds and how it was made is told in the CPU test file that pins it: test_snapshot.py,
# test_snapshot_nogc.py, test_version.py, test_version_shared.py)
def path(name):
    return os.path.join(HERE, name)


FIX, TFIX, PFIX, SFIX = (path("snapshot%s_v135.json.gz" % s) for s in ("", "_text", "_pending", "_subdoc"))
CFIX, PCFIX = path("contains_v135.json.gz"), path("contains_pending_v135.json.gz")
NFIX, S2FIX = path("snapshot_nogc_v135.json.gz"), path("step2_nogc_v135.json.gz")
VFIX, HFIX = path("version_v135.json.gz"), path("version_history_v135.json.gz")


def _pairs(fix):
    """-> (update, yjs's snapshot of it) per row"""
    d = json.load(gzip.open(fix, "rt"))
    return [(bytes.fromhex(u), bytes.fromhex(e)) for u, e in d["rows"]]


def fixtures():
    return _pairs(FIX)


def text_fixtures():
    return _pairs(TFIX)


def pending_fixtures():
    return _pairs(PFIX)


def subdoc_fixtures():
    return _pairs(SFIX)


def nogc_fixtures():
    return _pairs(NFIX)


def _contains(fix):
    """-> (state, update, Y.snapshotContainsUpdate's answer) per row"""
    d = json.load(gzip.open(fix, "rt"))
    states = [bytes.fromhex(s) for s in d["states"]]
    return [(states[i], bytes.fromhex(u), bool(e)) for i, u, e in d["rows"]]


def contains_fixtures():
    return _contains(CFIX)


def contains_pending_fixtures():
    return _contains(PCFIX)


def step2_nogc_rows():
    d = json.load(gzip.open(S2FIX, "rt"))
    return [(bytes.fromhex(u), bytes.fromhex(sv), None if e is None else bytes.fromhex(e), eq) for u, sv, e, eq in d["rows"]]


def version_rows():
    """-> dicts: family, state, version, take (bytes), restored / restored_nogc (bytes, or None where yjs throws)"""
    d = json.load(gzip.open(VFIX, "rt"))
    out = []
    for r in d["rows"]:
        o = {"family": r["family"], "note": r.get("note", "")}
        for k in ("state", "version", "take"):
            o[k] = bytes.fromhex(r[k])
        for k in ("restored", "restored_nogc"):
            o[k] = None if r[k] == "throws" else bytes.fromhex(r[k])
        out.append(o)
    return out


@functools.lru_cache(maxsize=None)
def history_docs():
    """-> dicts: family, state (bytes), versions: dicts of note, version (bytes), restored / restored_nogc (bytes, or
    None where yjs throws)"""
    d = json.load(gzip.open(HFIX, "rt"))
    out = []
    for doc in d["docs"]:
        vs = []
        for v in doc["versions"]:
            o = {"note": v.get("note", ""), "version": bytes.fromhex(v["version"])}
            for k in ("restored", "restored_nogc"):
                o[k] = None if v[k] == "throws" else bytes.fromhex(v[k])
            vs.append(o)
        out.append({"family": doc["family"], "state": bytes.fromhex(doc["state"]), "versions": vs})
    return tuple(out)


def version_to_desc(v):
    """An encoded Snapshot V1 as yjs 13.6 writes it: delete-set clients and state-vector clients descending."""
    from v1util import encode_ds, rd_vu, read_ds, vu
    ds, p = read_ds(v, 0)
    n, p = rd_vu(v, p)
    sv = []
    for _ in range(n):
        c, p = rd_vu(v, p)
        k, p = rd_vu(v, p)
        sv.append((c, k))
    o = bytearray(encode_ds(sorted(ds, key=lambda e: -e[0]))) + vu(len(sv))
    for c, k in sorted(sv, key=lambda e: -e[0]):
        o += vu(c) + vu(k)
    return bytes(o)


def update_to_desc(u):
    return bytes.fromhex(ds_to_desc(u.hex()))


def expected(row, key, compat135):
    """A version row's take / restored / restored_nogc as the engine answers it: yjs's bytes in 13.5 mode, their
    client-descending rewrite in the default mode, None where yjs throws."""
    e = row[key]
    if e is None or compat135:
        return e
    return version_to_desc(e) if key == "take" else update_to_desc(e)


def _sv(pairs, ds=b"\x00"):
    """An encoded version: a delete set, then the state vector's (client, clock) pairs."""
    from v1util import vu
    o = bytearray(ds) + vu(len(pairs))
    for c, k in pairs:
        o += vu(c) + vu(k)
    return bytes(o)


UNSUP_STATE = bytes([2, 1, 5, 0, 0, 1, 1, 5, 1, 0, 1, 0])   # client 5's block twice: outside the snapshot envelope

# versions ygm_version_restore_v1 refuses: (what, its bytes, the status) -- the header's refusal table
REFUSALS = (
    ("truncated state vector", lambda: _sv([(7, 3)])[:-1], 1),
    ("truncated delete set", lambda: bytes([1, 7, 1, 0]), 1),
    ("empty version", lambda: b"", 1),
    ("varuint above 2^53", lambda: b"\x00\x01\x07" + b"\xff" * 8 + b"\x7f", 2),
    ("non-minimal varuint", lambda: b"\x00\x01\x87\x00\x03", 3),
    ("client repeated in the state vector", lambda: _sv([(7, 3), (7, 2)]), 3),
    ("client repeated in the delete set", lambda: _sv([(7, 3)], ds=bytes([2, 7, 1, 0, 1, 7, 1, 2, 1])), 3),
    ("clock above the state's", lambda: _sv([(7, 6)]), 8),
    ("client the state does not have", lambda: _sv([(7, 3), (8, 1)]), 8),
    ("4097 state-vector entries", lambda: _sv([(7, 3)] + [(1000 + i, 0) for i in range(4096)]), 9),
)

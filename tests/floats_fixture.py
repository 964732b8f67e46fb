"""Shared pieces of the YGM_F_FLOATS tests: the two fixtures (tests/golden/dtoa_v8.json.gz: V8's Number.prototype.toString
for edge and random doubles; tests/golden/floats_v135.json.gz: states that hold floats, with yjs's JSON and the status a
context without the flag gives), an independent Number::toString built on Python's repr, and hand-written documents
whose Array root holds one ContentAny of numbers, each encoded as lib0's writeAny encodes it."""
import gzip
import json
import os
import struct

from v1util import vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DTOA_FIX = os.path.join(GOLDEN, "dtoa_v8.json.gz")
FLOATS_FIX = os.path.join(GOLDEN, "floats_v135.json.gz")
MAP, ARRAY, TEXT = 0, 1, 2
LONGEST = -1.7976931348623157e+308     # 24 bytes of JSON for 9 of state

_cache = {}


def load(path):
    if path not in _cache:
        _cache[path] = json.load(gzip.open(path, "rt"))
    return _cache[path]


def v8_doubles():
    """[(double, String(x))] of the fixture."""
    if "doubles" not in _cache:
        _cache["doubles"] = [(struct.unpack(">d", bytes.fromhex(h))[0], s) for h, s in load(DTOA_FIX)["doubles"]]
    return _cache["doubles"]


def v8_floats():
    """[(float32 bits, String(value))] of the fixture."""
    return [(int(h, 16), s) for h, s in load(DTOA_FIX)["floats"]]


def js_number(x):
    """Number::toString(x) of a finite double (ECMA-262): repr's digits -- the shortest that read back, correctly
    rounded -- laid out by JavaScript's rule."""
    if x == 0:
        return "0"
    mant, _, ex = repr(abs(x)).partition("e")
    ip, _, fp = mant.partition(".")
    digits = ip + fp
    n = len(ip) + (int(ex) if ex else 0)            # the value is 0.digits * 10^n
    lead = len(digits) - len(digits.lstrip("0"))
    digits, n = digits.lstrip("0").rstrip("0"), n - lead
    k = len(digits)
    if k <= n <= 21:
        s = digits + "0" * (n - k)
    elif 0 < n <= 21:
        s = digits[:n] + "." + digits[n:]
    elif -6 < n <= 0:
        s = "0." + "0" * -n + digits
    else:
        s = digits[0] + ("." + digits[1:] if k > 1 else "") + "e" + ("+" if n > 0 else "-") + str(abs(n - 1))
    return ("-" if x < 0 else "") + s


def any_number(x):
    """lib0 0.2.104 writeAny of a number: a varInt when it is an integer of magnitude <= 2^31 - 1, a float32 when that
    holds it exactly, else a float64 (so the state's parse finds it canonical)."""
    if x == int(x) and abs(x) <= 2147483647:
        n, neg = abs(int(x)), struct.pack(">d", x)[0] >= 0x80      # (negative zero keeps its sign bit, as lib0 writes it)
        o = bytearray([(0x80 if n > 63 else 0) | (0x40 if neg else 0) | (n & 63)])
        n >>= 6
        while n:
            o.append((0x80 if n > 127 else 0) | (n & 127))
            n >>= 7
        return b"\x7d" + bytes(o)
    try:
        f = struct.pack(">f", x)
        if struct.unpack(">f", f)[0] == x:
            return b"\x7c" + f
    except OverflowError:
        pass
    return b"\x7b" + struct.pack(">d", x)


def array_doc(values, client=7):
    """One client, one Item: a ContentAny of `values` in the list of root "a" -> (state, its toJSON as an Array)."""
    body = b"".join(any_number(x) for x in values)
    state = b"\x01\x01" + vu(client) + b"\x00" + b"\x08\x01\x01a" + vu(len(values)) + body + b"\x00"
    return state, ("[" + ",".join(js_number(x) for x in values) + "]").encode()


def tojson_rows():
    """(note, state, name, kind, status with the flag, bytes, status without it) of every toJSON ask."""
    return [(e["note"], bytes.fromhex(e["state"]), bytes.fromhex(r[0]), r[1], r[2], bytes.fromhex(r[3]), r[4])
            for e in load(FLOATS_FIX)["tojson"] for r in e["asks"]]


def json_rows():
    """(note, state, name, status with the flag, bytes, status without it) of every ProseMirror ask."""
    return [(e["note"], bytes.fromhex(e["state"]), bytes.fromhex(r[0]), r[1], bytes.fromhex(r[2]), r[3])
            for e in load(FLOATS_FIX)["json"] for r in e["asks"]]


def fields_rows():
    """(note, state, fields (None: all, or names), status with the flag, bytes, status without it) of every fields ask."""
    return [(e["note"], bytes.fromhex(e["state"]), None if r[0] is None else [bytes.fromhex(n) for n in r[0]], r[1], bytes.fromhex(r[2]), r[3])
            for e in load(FLOATS_FIX)["fields"] for r in e["asks"]]


def want(rows, floats):
    """[(status, bytes)] a context opened with / without the flag must give: without it a row that was refused keeps its
    refusal, every other row its bytes."""
    return [(r[-3], r[-2]) if floats else (r[-1], r[-2] if r[-1] == 0 else b"") for r in rows]

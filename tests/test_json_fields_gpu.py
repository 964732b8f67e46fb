"""Every field of a stored document as one JSON object on the GPU (ygm_json_fields_v1 / ygm_json_fields_v1_device:
k_json's fields instantiation over the workspace batch, with its second launch for the objects that outgrow their
workspace's output region).

Every row of tests/golden/json_fields_v135.json.gz through the host and the device form under both flag values; each
document's all-fields object against its roots' ygm_json_v1 outputs joined in the fixture's key order; objects that
overflow by their fields alone (an empty state under 12 absent names; six roots that fit one by one); all-fields,
listed, malformed-list, refused and __proto__ asks side by side in one wave at 1, 16 and 64 documents per wave; a host
batch over several chunks; a fields call between two single-field calls on one context; field lists that start 1 and
15 bytes into their arena.  Every comparison is exact."""
import collections
import re

import numpy as np
import pytest

import json_fields_fixture as ff
import json_fixture as jf
from devrun import engine_fixture, read_results, upload

pytestmark = pytest.mark.gpu

JSON_LINE = re.compile(r"^ygm json tiers: docs (\d+) general (\d+) overflow (\d+) overflow_bytes (\d+)$", re.M)
KNOBS = ("YGM_SNAP_NOLDS", "YGM_SNAP_DPW", "YGM_CHUNK_MB")
APIS = ("batch", "device")
EMPTY_STATE = b"\x00\x00"      # Y.encodeStateAsUpdate(new Y.Doc()): caps_of(0, 0, 0, 2).out = 2 + 48 * 4 + 16 + 64 = 274
CAP_EMPTY = 274
SIX = "overflow: six roots that fit one by one, an object that does not"
EINVAL, EMALFORMED, EUNSUPPORTED = 8, 1, 9

Out = collections.namedtuple("Out", "res lines")


def al16(n):
    return (n + 15) // 16 * 16


def enc(fields):
    from hocuspocus_amd.engine import encode_fields
    return encode_fields(fields)


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


eng = engine_fixture(compat135=True)


def tier_lines(capfd):
    return [dict(zip(("docs", "general", "overflow", "overflow_bytes"), map(int, ln))) for ln in JSON_LINE.findall(capfd.readouterr().err)]


def call(eng, capfd, states, lists, api, lead=0):
    """One fields call over (state, encoded field list) pairs; the device form's first list starts `lead` bytes into
    its arena.  Asserted for every call: the internal status 65 never comes out, a refused document has no bytes, the
    payload is the sum of the status-0 lengths."""
    n = len(states)
    out0 = eng.stats().bytes_out
    capfd.readouterr()
    if api == "batch":
        # (the raw lists go through the ABI as they are: Engine.json_fields_batch takes names, not bytes)
        import ctypes
        from hocuspocus_amd.engine import _Result, _pack, _ptr, lib
        sa, so = _pack([bytes(s) for s in states])
        fa, fo = _pack([bytes(f) for f in lists])
        r = _Result()
        rc = lib().ygm_json_fields_v1(eng._ctx, sa or None, _ptr(so), fa or None, _ptr(fo), 0, n, ctypes.byref(r))
        assert rc == 0
        got = eng._unpack(r)
        assert all(s == 0 or not b for s, b in got)
        res = [(s, b if s == 0 else b"") for s, b in got]
    else:
        ta, to, nbytes = upload(states)
        tf, tfo, _ = upload(lists, lead=lead)
        r = eng.json_fields_device(ta, nbytes, to, tf, tfo, n)
        res, offs, lens = read_results(r, n, every=True, places=True)
        assert all(offs[d] + lens[d] <= int(r.data_bytes) for d in range(n))
        assert int(r.payload_bytes) == sum(len(b) for st, b in res if st == 0)
    lines = tier_lines(capfd)
    assert jf.ST_MORE not in {st for st, _ in res}
    assert all(st == 0 or b == b"" for st, b in res)
    assert eng.stats().bytes_out - out0 == sum(len(b) for st, b in res if st == 0)
    assert sum(ln["docs"] for ln in lines) == n
    return Out(res, lines)


def check(rows, res, what):
    assert len(res) == len(rows)
    bad = [k for k in range(len(rows)) if not ff.matches(rows[k], *res[k])]
    assert not bad, (what, len(bad), [(rows[k].label, rows[k].fields, rows[k].status, res[k][0], res[k][1][:60]) for k in bad[:4]])


@pytest.mark.parametrize("compat", [True, False])
def test_whole_fixture_in_one_call(capfd, compat):
    from hocuspocus_amd import Engine
    rows = ff.rows()
    states, lists = [r.state for r in rows], ff.field_lists(rows)
    e = Engine(0, compat135=compat)
    try:
        for api in APIS:
            o = call(e, capfd, states, lists, api)
            check(rows, o.res, (api, compat))
            assert sum(ln["overflow"] for ln in o.lines) == 1      # (the six-root session's all-fields object)
        names = e.json_fields_batch([r.state for r in rows[:64]], [r.fields for r in rows[:64]])      # the names form of the binding
        check(rows[:64], [(0, x) if isinstance(x, bytes) else (x.code, b"") for x in names], "json_fields_batch")
    finally:
        e.close()


def test_all_fields_object_is_the_single_field_jsons_joined(eng, capfd):
    """Ties the two forms together on the GPU: per document, '{' + "key":ygm_json_v1(key), ... + '}' in the fixture's
    key order, or the first refusing key's status (a __proto__ key counting as YGM_EUNSUPPORTED where it stands)."""
    seen, docs = set(), []
    for r in ff.rows():
        if r.fields is None and (r.label, r.state) not in seen:
            seen.add((r.label, r.state))
            docs.append(r)
    pairs = [(k, d.state, key) for k, d in enumerate(docs) for key in d.keys]
    single = eng.json_batch([p[1] for p in pairs], [p[2] for p in pairs])
    capfd.readouterr()
    by = collections.defaultdict(list)
    for (k, _, key), x in zip(pairs, single):
        by[k].append((key, x))
    got = call(eng, capfd, [d.state for d in docs], [b""] * len(docs), "batch").res
    import json
    objects = 0
    for k, d in enumerate(docs):
        want_st, parts = 0, []
        for key, x in by[k]:
            st = EUNSUPPORTED if key == b"__proto__" else 0 if isinstance(x, bytes) else x.code
            if st:
                want_st = st
                break
            parts.append(json.dumps(key.decode(), ensure_ascii=False).encode() + b":" + x)
        want = (0, b"{" + b",".join(parts) + b"}") if want_st == 0 else (want_st, b"")
        assert got[k] == want, (d.label, want_st, got[k][0])
        assert got[k][0] == d.status
        objects += want_st == 0
    assert objects >= 40 and len(docs) > 1700


@pytest.mark.parametrize("api", APIS)
def test_overflow_by_fields_alone(eng, capfd, api):
    names12 = [b"absent%02d" % i for i in range(12)]
    want12 = b"{" + b",".join(b'"%s":%s' % (n, ff.EMPTY_DOC) for n in names12) + b"}"
    want2 = b"{" + b",".join(b'"%s":%s' % (n, ff.EMPTY_DOC) for n in names12[:2]) + b"}"
    assert all(len(n) == 8 for n in names12) and len(want2) <= CAP_EMPTY < len(want12)
    o = call(eng, capfd, [EMPTY_STATE], [enc(names12)], api)
    assert o.res == [(0, want12)]
    assert o.lines == [{"docs": 1, "general": 1, "overflow": 1, "overflow_bytes": al16(len(want12))}]
    o = call(eng, capfd, [EMPTY_STATE], [enc(names12[:2])], api)
    assert o.res == [(0, want2)] and o.lines == [{"docs": 1, "general": 1, "overflow": 0, "overflow_bytes": 0}]
    # the exact edge: an object of exactly the region's bytes fits, one byte more runs again
    fit = [b"k" * (CAP_EMPTY - 2 - 3 - len(ff.EMPTY_DOC))]
    for names, rerun in ((fit, 0), ([fit[0] + b"k"], 1)):
        want = b'{"%s":%s}' % (names[0], ff.EMPTY_DOC)
        assert len(want) == CAP_EMPTY + rerun
        o = call(eng, capfd, [EMPTY_STATE], [enc(names)], api)
        assert o.res == [(0, want)] and o.lines[0]["overflow"] == rerun and o.lines[0]["overflow_bytes"] == rerun * al16(len(want))
    # six roots: each root's JSON fits its workspace (the single-field calls do not rerun), the object does not
    six = ff.edge(SIX)
    capfd.readouterr()
    singles = eng.json_batch([six[0].state] * 6, six[0].keys)
    assert [ln["overflow"] for ln in tier_lines(capfd)] == [0] and all(isinstance(x, bytes) for x in singles)
    o = call(eng, capfd, [six[0].state, EMPTY_STATE, six[1].state], [b"", b"", enc(six[1].fields)], api)
    check([six[0]], o.res[:1], api)
    check([six[1]], o.res[2:], api)
    assert o.res[1] == (0, b"{}")
    assert o.res[0][1] == b"{" + b",".join(b'"%s":%s' % (k, x) for k, x in zip(six[0].keys, singles)) + b"}"
    assert o.lines == [{"docs": 3, "general": 3, "overflow": 1, "overflow_bytes": al16(six[0].length)}]      # (two roots fit)


def mixed(eng):
    """(state, encoded list, status, bytes or None: see the fixture row) for one wave and a half of unlike asks."""
    odd = ff.edge("roots named 2, 10, b, 01, the empty name, 4294967295 and a name to escape")
    proto = ff.edge("a __proto__ root")
    two3 = ff.edge("two roots, the first in output order refuses with 3, the other with 9")
    pend = ff.edge("a root named only by pending structs")
    one = ff.edge("one root")
    six = ff.edge(SIX)
    cut = one[0].state[:-3]
    snap = eng.snapshot_batch([cut])[0][0]
    assert snap not in (0, EINVAL)

    def row(r):
        return (r.state, enc(r.fields), r)

    def raw(state, fl, st, b=b""):
        return (state, fl, ff.Row("raw", state, None, st, b, "", len(b), []))
    docs = [row(odd[0]), row(odd[1]), raw(one[0].state, b"\x05abcd", EINVAL), row(proto[0]), raw(EMPTY_STATE, b"", 0, b"{}"),
            raw(cut, b"", snap), row(six[0]), raw(one[0].state, b"\x81\x00a", EINVAL), row(proto[3]), raw(b"", b"", EMALFORMED),
            row(two3[0]), row(two3[3]), raw(EMPTY_STATE, b"\x02\xc0\xaf", EINVAL), row(pend[0]), row(proto[1]), row(one[3]),
            raw(cut, b"\x81\x00a", snap), row(odd[2]), row(six[1]), raw(odd[0].state, b"\x01a" * 1025, EINVAL), row(odd[3]),
            raw(one[0].state, b"\x01a" * 1024, 0, b'{"a":%s}' % ff.EMPTY_DOC), row(pend[2]), row(two3[4])]
    return docs


@pytest.mark.parametrize("dpw", [None, "1", "64"])
def test_mixed_lanes(eng, capfd, monkeypatch, dpw):
    if dpw:
        monkeypatch.setenv("YGM_SNAP_DPW", dpw)
    docs = mixed(eng)
    assert 16 < len(docs) < 32
    rows = [d[2] for d in docs]
    assert {r.status for r in rows} >= {0, 3, 9, EINVAL, EMALFORMED}
    for api in APIS:
        o = call(eng, capfd, [d[0] for d in docs], [d[1] for d in docs], api)
        check(rows, o.res, (api, dpw))
        assert [st for st, _ in o.res] == [r.status for r in rows]
        assert [ln["overflow"] for ln in o.lines] == [1]      # (the six-root object; its two-root ask fits)


def test_chunks_equal_one_call(eng, capfd, monkeypatch):
    rows = ff.rows()
    take, total = 0, 0
    while total <= (5 << 19):      # 2.5 MB of states: three chunks of 1 MB
        total += len(rows[take].state)
        take += 1
    rows = rows[:take] + ff.edge(SIX)      # (a rerun in the last chunk)
    assert all(len(r.state) < (1 << 20) for r in rows)
    states, lists = [r.state for r in rows], ff.field_lists(rows)
    one = call(eng, capfd, states, lists, "batch")
    check(rows, one.res, "one chunk")
    assert len(one.lines) == 1
    monkeypatch.setenv("YGM_CHUNK_MB", "1")
    many = call(eng, capfd, states, lists, "batch")
    assert len(many.lines) >= 2
    assert many.res == one.res
    assert sum(ln["overflow"] for ln in many.lines) == one.lines[0]["overflow"] >= 1
    assert sum(ln["overflow_bytes"] for ln in many.lines) == one.lines[0]["overflow_bytes"]
    # asks of both kinds on both sides of the first cut
    first = many.lines[0]["docs"]
    assert {r.fields is None for r in rows[:first]} == {r.fields is None for r in rows[first:]} == {True, False}


def test_between_two_single_field_calls(eng, capfd):
    """A fields call (with a rerun) between two ygm_json_v1 calls on one context leaves their results and their
    host_syncs deltas as they are."""
    single = [r for r in jf.expectations(sets=(), edges=True) if r[3] == 0 and not r[0].startswith("overflow")][:20]
    six = ff.edge(SIX)
    odd = ff.edge("roots named 2, 10, b, 01, the empty name, 4294967295 and a name to escape")
    frows = [odd[0], six[0], odd[1]]

    def plain():
        capfd.readouterr()
        res = eng.json_batch([r[1] for r in single], [r[2] for r in single])
        return res, tier_lines(capfd)
    s0 = eng.stats().host_syncs
    a, la = plain()
    s1 = eng.stats().host_syncs
    f1 = call(eng, capfd, [r.state for r in frows], ff.field_lists(frows), "batch")
    s2 = eng.stats().host_syncs
    b, lb = plain()
    s3 = eng.stats().host_syncs
    f2 = call(eng, capfd, [r.state for r in frows], ff.field_lists(frows), "batch")
    check(frows, f1.res, "fields")
    assert a == b == [r[4] for r in single] and la == lb and [ln["overflow"] for ln in la] == [0]
    assert f1.res == f2.res and f1.lines == f2.lines and [ln["overflow"] for ln in f1.lines] == [1]
    assert s3 - s2 == s1 - s0 and (s2 - s1) - (s1 - s0) == 1, (s0, s1, s2, s3)      # (the rerun's one more wait)


@pytest.mark.parametrize("lead", [1, 15])
def test_field_lists_anywhere_in_their_arena(eng, capfd, lead):
    rows = [r for r in ff.rows(sets=(), edges=True)]
    o = call(eng, capfd, [r.state for r in rows], ff.field_lists(rows), "device", lead)
    check(rows, o.res, lead)
    assert sum(ln["overflow"] for ln in o.lines) == 1


def test_empty_batch_and_bad_kind(eng):
    import ctypes
    from hocuspocus_amd.engine import YjsError, _Result, lib
    assert eng.json_fields_batch([], []) == []
    assert eng.json_fields_device(0, 0, 0, 0, 0, 0).payload_bytes == 0
    assert eng.json_fields_batch([EMPTY_STATE], [None]) == [b"{}"]      # every list empty: no fields arena
    assert eng.json_fields_batch([EMPTY_STATE, EMPTY_STATE], [[], ["x"]]) == [b"{}", b'{"x":%s}' % ff.EMPTY_DOC]
    off = np.array([0, 2], np.uint64)
    foff = np.array([0, 0], np.uint64)
    res = _Result()
    for kind in (1, 0xFFFFFFFF):
        rc = lib().ygm_json_fields_v1(eng._ctx, ctypes.c_char_p(EMPTY_STATE), off.ctypes.data_as(ctypes.c_void_p), None,
                                      foff.ctypes.data_as(ctypes.c_void_p), kind, 1, ctypes.byref(res))
        assert rc == EINVAL
        with pytest.raises(YjsError) as e:
            eng.json_fields_device(0, 0, 0, 0, 0, 0, kind=kind)
        assert e.value.code == EINVAL

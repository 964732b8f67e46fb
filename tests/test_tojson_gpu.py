"""toJSON of stored Map, Array and Text roots on the GPU (ygm_tojson_v1 / ygm_tojson_v1_device: the snapshot's count /
scan launches, k_tojson, and k_tojson's second launch for the documents whose JSON did not fit their workspace).

Every row of tests/golden/tojson_v135.json.gz (yjs 13.5.16's own toJSON: serialized roots and refusals) through the
host and the device form, one batch per kind; batches of one document fewer than, exactly and one more than a wave
takes; a wave whose documents end one byte under, at and over the staged size; refusals between good neighbours; the
4 KB string of 0x01 bytes, whose 24 KB JSON takes the second run at the cost of exactly one more host wait; a host
batch over two chunks; docs_snapshot; and ygm_json_v1, which still refuses kinds 1 and 2."""
import ctypes
import re

import numpy as np
import pytest

import tojson_fixture as tf
from devrun import engine_fixture, read_results, upload
from v1util import vu

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^ygm tojson tiers: docs (\d+) general (\d+) overflow (\d+) overflow_bytes (\d+)$", re.M)
KNOBS = ("YGM_SNAP_NOLDS", "YGM_SNAP_DPW", "YGM_CHUNK_MB")
DPW = 16             # docstage::DPW
STAGE = 40960        # docstage::STAGE
BIG = "a 4 KB string of 0x01 bytes in a Map"
APIS = ("batch", "device")


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


eng = engine_fixture(compat135=True)


def device_tojson(eng, states, names, kind, lead=0):
    """ygm_tojson_v1_device over arenas from torch (the first state `lead` bytes into its arena) -> (status, bytes)."""
    ta, to, nbytes = upload(states, lead=lead)
    tn, tno, _ = upload(names)
    assert ta.data_ptr() % 16 == 0
    n = len(states)
    r = eng.tojson_device(ta, nbytes, to, tn, tno, n, kind)
    res, offs, lens = read_results(r, n, every=True, places=True)
    assert int(r.payload_bytes) == sum(lens[d] for d in range(n) if res[d][0] == 0)
    for d in range(n):
        assert offs[d] + lens[d] <= int(r.data_bytes) and (res[d][0] == 0 or lens[d] == 0)
    return res


def run(eng, capfd, states, names, kind, api="batch", lead=0):
    """One call of one kind -> [(status, bytes)], the call's tier lines."""
    capfd.readouterr()
    if api == "batch":
        res = [(0, r) if isinstance(r, bytes) else (r.code, b"") for r in eng.tojson_batch(states, names, kind)]
    else:
        res = device_tojson(eng, states, names, kind, lead)
    lines = [dict(zip(("docs", "general", "overflow", "overflow_bytes"), map(int, ln))) for ln in LINE.findall(capfd.readouterr().err)]
    assert tf.ST_MORE not in {s for s, _ in res}
    return res, lines


def run_rows(eng, capfd, rows, api="batch"):
    """Rows of any kinds, one call per kind, results back in the rows' order; the tier lines of all the calls."""
    res, lines = [None] * len(rows), []
    for kind in (tf.MAP, tf.ARRAY, tf.TEXT):
        idx = [k for k, r in enumerate(rows) if r[3] == kind]
        if idx:
            got, ln = run(eng, capfd, [rows[k][1] for k in idx], [rows[k][2] for k in idx], kind, api)
            lines += ln
            for k, g in zip(idx, got):
                res[k] = g
    return res, lines


def check(rows, res, what):
    assert len(res) == len(rows)
    bad = [k for k in range(len(rows)) if not tf.matches(rows[k], *res[k])]
    assert not bad, (what, len(bad), [(rows[k][0], rows[k][2], rows[k][3], rows[k][4], res[k][0], res[k][1][:60], (rows[k][5] or b"")[:60]) for k in bad[:4]])


def test_whole_fixture_host_and_device_forms_agree(eng, capfd):
    rows = tf.expectations()
    host, l1 = run_rows(eng, capfd, rows, "batch")
    check(rows, host, "batch")
    dev, l2 = run_rows(eng, capfd, rows, "device")
    assert dev == host                      # equal bytes, equal statuses
    for lines in (l1, l2):
        assert sum(ln["docs"] for ln in lines) == len(rows) and sum(ln["overflow"] for ln in lines) == 1
    print("whole fixture", l2)


def test_default_flags_give_the_same(capfd):
    from hocuspocus_amd import Engine
    rows = tf.expectations(sets=(), edges=True, random=True)
    e136 = Engine(0, compat135=False)   # the JSON does not depend on YGM_F_COMPAT_135
    try:
        res, _ = run_rows(e136, capfd, rows)
        check(rows, res, "default flags")
    finally:
        e136.close()


@pytest.mark.parametrize("n", [DPW - 1, DPW, DPW + 1])
def test_batches_around_a_wave(eng, capfd, n):
    rows = [r for r in tf.expectations(sets=(), edges=False) if r[3] == tf.MAP][:n]
    assert len(rows) == n
    for api in APIS:
        res, lines = run(eng, capfd, [r[1] for r in rows], [r[2] for r in rows], tf.MAP, api)
        check(rows, res, (api, n))
        assert [ln["docs"] for ln in lines] == [n]


def map_doc(n, salt=0):
    """Written out by hand: one client, one Item -- a ContentAny holding a string of n letters under key "k" of root
    "m"; its toJSON as a Map is {"k":"<the letters>"}."""
    s = bytes(97 + (i * 7 + salt) % 26 for i in range(n))
    return b"\x01\x01" + vu(7) + b"\x00" + b"\x28\x01\x01m\x01k" + b"\x01\x77" + vu(n) + s + b"\x00", b'{"k":"' + s + b'"}'


def fitted(count, total):
    """`count` documents of `total` bytes together: equal lengths, the last adjusted (a document is its n letters, the
    varuint of n and 13 bytes around them)."""
    size = lambda n: len(map_doc(0)[0]) - 1 + len(vu(n)) + n
    ns = [total // count - size(0) - 2] * count
    rest = total - sum(size(n) for n in ns[:-1])
    for last in range(max(rest - size(0) - 4, 0), rest):
        if size(last) == rest:
            return ns[:-1] + [last]
    raise AssertionError("no fit")


@pytest.mark.parametrize("dpw,count", [(None, DPW), ("1", 1)])
@pytest.mark.parametrize("extent", [STAGE - 1, STAGE, STAGE + 1])
def test_staged_size_boundary(eng, capfd, monkeypatch, dpw, count, extent):
    """The first wave's documents end exactly `extent` bytes after its 16-aligned start: one byte under and at the
    staged size they are parsed from LDS, one byte over from memory; a second wave follows."""
    if dpw:
        monkeypatch.setenv("YGM_SNAP_DPW", dpw)
    docs = [map_doc(n, k) for k, n in enumerate(fitted(count, extent))] + [map_doc(33, 5), map_doc(0, 1)]
    assert sum(len(d[0]) for d in docs[:count]) == extent
    res, lines = run(eng, capfd, [d[0] for d in docs], [b"m"] * len(docs), tf.MAP, "device")
    assert res == [(0, d[1]) for d in docs]
    assert [ln["overflow"] for ln in lines] == [0]


def test_every_second_document_refused(eng, capfd):
    edges = [r for r in tf.expectations(sets=(), edges=True, random=False) if r[3] == tf.MAP]
    good = [r for r in edges if r[4] == 0 and r[0] != BIG]
    refused = [r for r in edges if r[4] != 0]
    assert {r[4] for r in refused} == {9, 3, 1} and len(refused) == 8
    cut = good[3][1][:-3]
    snap = eng.snapshot_batch([cut])[0][0]
    assert snap != 0
    refused.append(("truncated", cut, b"m", tf.MAP, snap, b"", "", 0))
    rows = []
    for k, r in enumerate(refused):
        rows += [good[k % len(good)], r]
    rows.append(good[0])
    for api in APIS:
        res, _ = run(eng, capfd, [r[1] for r in rows], [r[2] for r in rows], tf.MAP, api)
        check(rows, res, api)


def test_overflow_runs_again_with_one_more_host_wait(eng, capfd):
    edges = tf.expectations(sets=(), edges=True, random=False)
    big = [r for r in edges if r[0] == BIG][0]
    small = [r for r in edges if r[0] == "a key set twice"][0]
    assert len(big[1]) < 4200 and big[7] == 6 * 4096 + len('{"ctl":""}') and big[5].count(b"\\u0001") == 4096
    notes = []
    for api in APIS:
        s0 = eng.stats().host_syncs
        res2, l2 = run(eng, capfd, [small[1], small[1]], [b"m", b"m"], tf.MAP, api)
        s1 = eng.stats().host_syncs
        res3, l3 = run(eng, capfd, [small[1], big[1], small[1]], [b"m", b"m", b"m"], tf.MAP, api)
        s2 = eng.stats().host_syncs
        check([small, small], res2, api)
        check([small, big, small], res3, api)
        notes.append((api, "without", l2, "host_syncs", s1 - s0, "with", l3, "host_syncs", s2 - s1))
        assert res3[0] == res2[0] and res3[2] == res2[1]
        assert [ln["overflow"] for ln in l2] == [0] and [ln["overflow"] for ln in l3] == [1]
        assert l3[0]["overflow_bytes"] == (big[7] + 15) // 16 * 16
        assert (s2 - s1) - (s1 - s0) == 1, (s0, s1, s2)
    for n in notes:
        print(*n)


def test_two_chunks_equal_one(eng, capfd, monkeypatch):
    rows = [r for r in tf.expectations() if r[3] == tf.MAP]
    states, names = [r[1] for r in rows], [r[2] for r in rows]
    assert (5 << 20) < sum(map(len, states)) < (10 << 20)      # (8.1 MB of states: two chunks of 5 MB)
    one, l1 = run(eng, capfd, states, names, tf.MAP)
    monkeypatch.setenv("YGM_CHUNK_MB", "5")
    two, l2 = run(eng, capfd, states, names, tf.MAP)
    assert len(l1) == 1 and len(l2) == 2
    assert one == two
    check(rows, two, "two chunks")


def test_docs_snapshot_grows_by_n_docs(eng, capfd):
    rows = [r for r in tf.expectations(sets=(), edges=False) if r[3] == tf.ARRAY][:37]
    for api in APIS:
        s0 = eng.stats()
        d0 = s0.docs_snapshot
        res, _ = run(eng, capfd, [r[1] for r in rows], [r[2] for r in rows], tf.ARRAY, api)
        check(rows, res, api)
        s1 = eng.stats()
        assert s1.docs_snapshot - d0 == len(rows)


def test_empty_batch_and_bad_kind(eng):
    from hocuspocus_amd.engine import EINVAL, YjsError, _Result, lib
    st, name, kind, js, status = tf.edge("a key set twice")
    assert (kind, status, js) == (tf.MAP, 0, b'{"a":"three","b":"two"}')
    for k in (tf.MAP, tf.ARRAY, tf.TEXT):
        assert eng.tojson_batch([], [], k) == []
        assert eng.tojson_device(0, 0, 0, 0, 0, 0, k).payload_bytes == 0
    assert eng.tojson_batch([st], ["m"], tf.MAP) == [js]
    assert eng.tojson_batch([st, st, st], ["", "", ""], tf.MAP) == [b"{}"] * 3      # every name empty: no names arena
    assert eng.tojson_batch([st], [""], tf.ARRAY) == [b"[]"] and eng.tojson_batch([st], [""], tf.TEXT) == [b'""']
    off = np.array([0, len(st)], np.uint64)
    noff = np.array([0, 1], np.uint64)
    res = _Result()
    for bad in (3, 0xFFFFFFFF):
        rc = lib().ygm_tojson_v1(eng._ctx, ctypes.c_char_p(st), off.ctypes.data_as(ctypes.c_void_p), ctypes.c_char_p(b"m"),
                                 noff.ctypes.data_as(ctypes.c_void_p), bad, 1, ctypes.byref(res))
        assert rc == EINVAL
        with pytest.raises(YjsError) as e:
            eng.tojson_device(0, 0, 0, 0, 0, 0, bad)
        assert e.value.code == EINVAL
        with pytest.raises(YjsError):
            eng.tojson_batch([st], ["m"], bad)


def test_json_v1_still_refuses_kinds_1_and_2(eng):
    from hocuspocus_amd.engine import EINVAL, YjsError
    st = tf.edge("a key set twice")[0]
    for kind in (1, 2):
        with pytest.raises(YjsError) as e:
            eng.json_batch([st], ["m"], kind=kind)
        assert e.value.code == EINVAL
        with pytest.raises(YjsError) as e:
            eng.json_fields_batch([st], [None], kind=kind)
        assert e.value.code == EINVAL

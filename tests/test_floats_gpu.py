"""Non-integer numbers in stored-document JSON on the GPU (YGM_F_FLOATS given to ygm_open): the FLOATS instantiations of
k_tojson and k_json, beside a context opened without the flag.

Every row of tests/golden/floats_v135.json.gz (yjs 13.5.16's JSON of states that hold floats) through ygm_tojson_v1,
ygm_json_v1, ygm_json_fields_v1 and their _device forms on both contexts: with the flag strings and statuses are yjs's,
without it every row that holds a float is YGM_ENONCANON and every other row is unchanged.  A batch of 64 hand-written
Array documents of 512 numbers each from tests/golden/dtoa_v8.json.gz (the device's 128-bit product against V8's
strings); the same batch of -1.7976931348623157e+308 alone, whose JSON outgrows every workspace and takes the second
launch at the cost of exactly one more host wait; and a float document between an integer-only, a malformed and a
BigInt one."""
import re

import pytest

import floats_fixture as ff
from devrun import read_results, upload
from hocuspocus_amd.engine import encode_fields

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^ygm (tojson|json) tiers: docs (\d+) general (\d+) overflow (\d+) overflow_bytes (\d+)$", re.M)
KNOBS = ("YGM_SNAP_NOLDS", "YGM_SNAP_DPW", "YGM_CHUNK_MB")
APIS = ("batch", "device")


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def engines():
    """(a context opened with YGM_F_FLOATS, one opened without)"""
    from hocuspocus_amd import Engine
    on, off = Engine(0, floats=True), Engine(0)
    yield on, off
    on.close()
    off.close()


def device_call(eng, fn, states, seconds, kind=None):
    """One of the _device forms over arenas from torch -> [(status, bytes)]."""
    ta, to, nbytes = upload(states)
    tn, tno, _ = upload(seconds)
    n = len(states)
    r = getattr(eng, fn)(ta, nbytes, to, tn, tno, n, *(() if kind is None else (kind,)))
    res, offs, lens = read_results(r, n, every=True, places=True)
    for d in range(n):
        assert offs[d] + lens[d] <= int(r.data_bytes) and (res[d][0] == 0 or lens[d] == 0)
    return res


def plain(res):
    return [(0, r) if isinstance(r, bytes) else (r.code, b"") for r in res]


def tojson(eng, states, names, kind, api):
    if api == "batch":
        return plain(eng.tojson_batch(states, names, kind))
    return device_call(eng, "tojson_device", states, names, kind)


def tojson_rows(eng, rows, api):
    res = [None] * len(rows)
    for kind in (ff.MAP, ff.ARRAY, ff.TEXT):
        idx = [k for k, r in enumerate(rows) if r[3] == kind]
        for k, g in zip(idx, tojson(eng, [rows[k][1] for k in idx], [rows[k][2] for k in idx], kind, api)):
            res[k] = g
    return res


def same(rows, got, floats, what):
    want = ff.want(rows, floats)
    bad = [(r[0], r[2], w[0], g[0], w[1][:80], g[1][:80]) for r, w, g in zip(rows, want, got) if g != w]
    assert len(got) == len(rows) and not bad, (what, floats, len(bad), bad[:4])


@pytest.mark.parametrize("api", APIS)
def test_tojson_fixture_on_both_contexts(engines, api):
    rows = ff.tojson_rows()
    for eng, floats in zip(engines, (True, False)):
        same(rows, tojson_rows(eng, rows, api), floats, "tojson " + api)
    assert sum(r[4] == 0 and r[6] == 3 for r in rows) >= 180


@pytest.mark.parametrize("api", APIS)
def test_json_and_json_fields_fixture_on_both_contexts(engines, api):
    pj, fj = ff.json_rows(), ff.fields_rows()
    for eng, floats in zip(engines, (True, False)):
        if api == "batch":
            got = plain(eng.json_batch([r[1] for r in pj], [r[2] for r in pj]))
            gotf = plain(eng.json_fields_batch([r[1] for r in fj], [r[2] for r in fj]))
        else:
            got = device_call(eng, "json_device", [r[1] for r in pj], [r[2] for r in pj])
            gotf = device_call(eng, "json_fields_device", [r[1] for r in fj], [encode_fields(r[2]) for r in fj])
        same(pj, got, floats, "json " + api)
        same(fj, gotf, floats, "json_fields " + api)


def v8_batch():
    """64 documents of 512 numbers each, taken in turn from the V8 fixture (wrapping around), with V8's own strings."""
    v8 = ff.v8_doubles()
    docs = []
    for d in range(64):
        part = [v8[(d * 512 + i) % len(v8)] for i in range(512)]
        state, js = ff.array_doc([x for x, _ in part], 100 + d)
        assert js == ("[" + ",".join(s for _, s in part) + "]").encode()      # the test's reference is V8's strings
        docs.append((state, js))
    return docs


@pytest.mark.parametrize("api", APIS)
def test_64_array_documents_of_512_numbers_equal_v8(engines, api):
    on, off = engines
    docs = v8_batch()
    got = tojson(on, [d[0] for d in docs], [b"a"] * 64, ff.ARRAY, api)
    bad = [d for d in range(64) if got[d] != (0, docs[d][1])]
    if bad:
        g, w = got[bad[0]][1].split(b","), docs[bad[0]][1].split(b",")
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(g, w)) if a != b][:5]
        raise AssertionError((api, len(bad), bad[:4], got[bad[0]][0], diff))
    assert tojson(off, [d[0] for d in docs], [b"a"] * 64, ff.ARRAY, api) == [(3, b"")] * 64


def test_longest_numbers_take_the_second_launch_with_one_more_host_wait(engines, capfd):
    """Every value -1.7976931348623157e+308: 24 bytes (and a comma) for 9 bytes of state.  All 64 documents outgrow
    their workspace's output region, are listed, run again and come out whole; host_syncs grows by the one extra wait."""
    on, _ = engines
    state, js = ff.array_doc([ff.LONGEST] * 512)
    small = ff.array_doc([1.5, 0.25, -3.75])
    assert len(js) == 512 * 25 + 1
    for api in APIS:
        capfd.readouterr()
        s0 = on.stats().host_syncs
        r2 = tojson(on, [small[0]] * 64, [b"a"] * 64, ff.ARRAY, api)
        s1 = on.stats().host_syncs
        l2 = LINE.findall(capfd.readouterr().err)
        r3 = tojson(on, [state] * 64, [b"a"] * 64, ff.ARRAY, api)
        s2 = on.stats().host_syncs
        l3 = LINE.findall(capfd.readouterr().err)
        assert r2 == [(0, small[1])] * 64
        assert r3 == [(0, js)] * 64
        print(api, "without", l2, "host_syncs", s1 - s0, "with", l3, "host_syncs", s2 - s1)
        assert [(ln[0], int(ln[1]), int(ln[3])) for ln in l2] == [("tojson", 64, 0)]
        assert [(ln[0], int(ln[1]), int(ln[3])) for ln in l3] == [("tojson", 64, 64)]
        assert int(l3[0][4]) == 64 * ((len(js) + 15) // 16 * 16)
        assert (s2 - s1) - (s1 - s0) == 1, (s0, s1, s2)


@pytest.mark.parametrize("api", APIS)
def test_mixed_batch_each_status_its_own(engines, api):
    """A float document, an integer-only one, a malformed one and a BigInt one, twice over: each status is its own."""
    on, off = engines
    rows = {r[0]: r for r in ff.tojson_rows() if r[3] == ff.MAP}
    fl, ints, big = rows["refused: a finite non-integer number"], rows["integers only (the flag changes nothing)"], \
        rows["a float before a BigInt, and a float after a Uint8Array"]
    cut = ints[1][:-3]
    bad = plain(off.tojson_batch([cut], [b"m"], ff.MAP))[0]
    assert bad[0] not in (0, 3) and bad[1] == b""
    states = [fl[1], ints[1], cut, big[1]] * 2 + [fl[1]]
    got_on = tojson(on, states, [b"m"] * len(states), ff.MAP, api)
    got_off = tojson(off, states, [b"m"] * len(states), ff.MAP, api)
    assert got_on == [(0, b'{"w":1.5}'), (0, ints[5]), bad, (1, b"")] * 2 + [(0, b'{"w":1.5}')]
    assert got_off == [(3, b""), (0, ints[5]), bad, (3, b"")] * 2 + [(3, b"")]

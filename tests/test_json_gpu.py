"""Stored documents as ProseMirror JSON on the GPU (ygm_json_v1 / ygm_json_v1_device: the snapshot's count / scan
launches, k_json, and k_json's second launch for the documents whose JSON did not fit their workspace).

Every row of tests/golden/json_v135.json.gz (yjs 13.5.16 and the restated y-prosemirror serializer: serialized roots
and refusals) through the host and the device form; the edge sessions as a batch of their own; refusals and a
truncated state between good neighbours; the overflow session's second run and its one extra host wait; the call's
argument checks; a host batch over two chunks."""
import ctypes
import re

import numpy as np
import pytest

import json_fixture as jf
from devrun import engine_fixture, read_results, upload

pytestmark = pytest.mark.gpu

JSON_LINE = re.compile(r"^ygm json tiers: docs (\d+) general (\d+) overflow (\d+) overflow_bytes (\d+)$", re.M)
KNOBS = ("YGM_SNAP_NOLDS", "YGM_SNAP_DPW", "YGM_CHUNK_MB")
OVERFLOW = "overflow: 64 one-character strings, each under one more mark"
F = b"default"


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


eng = engine_fixture(compat135=True)


def host_json(eng, states, names):
    return [(0, r) if isinstance(r, bytes) else (r.code, b"") for r in eng.json_batch(states, names)]


def device_json(eng, states, names):
    """ygm_json_v1_device over arenas from torch -> (status, bytes) pairs."""
    ta, to, nbytes = upload(states)
    tn, tno, _ = upload(names)
    n = len(states)
    r = eng.json_device(ta, nbytes, to, tn, tno, n)
    res, offs, lens = read_results(r, n, every=True, places=True)
    assert int(r.payload_bytes) == sum(lens[d] for d in range(n) if res[d][0] == 0)
    for d in range(n):
        assert offs[d] + lens[d] <= int(r.data_bytes) and (res[d][0] == 0 or lens[d] == 0)
    return res


def run(eng, capfd, states, names, api="batch"):
    capfd.readouterr()
    res = host_json(eng, states, names) if api == "batch" else device_json(eng, states, names)
    lines = JSON_LINE.findall(capfd.readouterr().err)
    return res, [dict(zip(("docs", "general", "overflow", "overflow_bytes"), map(int, ln))) for ln in lines]


def check(rows, res, what):
    assert len(res) == len(rows)
    bad = [k for k in range(len(rows)) if not jf.matches(rows[k], *res[k])]
    assert not bad, (what, len(bad), [(rows[k][0], rows[k][2], rows[k][3], res[k][0], res[k][1][:60], (rows[k][4] or b"")[:60]) for k in bad[:4]])


@pytest.mark.parametrize("api", ["batch", "device"])
def test_whole_fixture_in_one_call(eng, capfd, api):
    rows = jf.expectations()
    res, lines = run(eng, capfd, [r[1] for r in rows], [r[2] for r in rows], api)
    check(rows, res, api)
    assert sum(ln["docs"] for ln in lines) == len(rows) and sum(ln["overflow"] for ln in lines) == 1
    assert jf.ST_MORE not in {s for s, _ in res}


@pytest.mark.parametrize("api", ["batch", "device"])
def test_edge_sessions_as_a_batch(eng, capfd, api):
    from hocuspocus_amd import Engine
    rows = jf.expectations(sets=(), edges=True)
    res, _ = run(eng, capfd, [r[1] for r in rows], [r[2] for r in rows], api)
    check(rows, res, api)
    e136 = Engine(0, compat135=False)   # the JSON does not depend on YGM_F_COMPAT_135
    try:
        res, _ = run(e136, capfd, [r[1] for r in rows], [r[2] for r in rows], api)
        check(rows, res, (api, "default flags"))
    finally:
        e136.close()


def test_refusals_and_a_truncated_state_touch_no_neighbour(eng, capfd):
    edges = [r for r in jf.expectations(sets=(), edges=True) if r[2] == F]
    good = [r for r in edges if r[3] == 0 and not r[0].startswith("overflow")]
    refused = [r for r in edges if r[3] != 0]
    assert {r[3] for r in refused} == {9, 3, 1} and len(refused) >= 10
    cut = good[5][1][:-3]
    snap = eng.snapshot_batch([cut])[0][0]
    assert snap != 0
    rows = []
    for k, r in enumerate(refused):
        rows += [good[k % len(good)], r]
    rows += [good[0], (("truncated", cut, F, snap, b"", "", 0)), good[1]]
    for api in ("batch", "device"):
        res, _ = run(eng, capfd, [r[1] for r in rows], [r[2] for r in rows], api)
        check(rows, res, api)


def test_overflow_runs_again_with_one_more_host_wait(eng, capfd):
    ovf = [r for r in jf.expectations(sets=(), edges=True) if r[0] == OVERFLOW and r[2] == F][0]
    small = [r for r in jf.expectations(sets=(), edges=True) if r[0] == "marks: on then off" and r[2] == F][0]
    for api in ("batch", "device"):
        s0 = eng.stats().host_syncs
        res2, l2 = run(eng, capfd, [small[1], small[1]], [F, F], api)
        s1 = eng.stats().host_syncs
        res3, l3 = run(eng, capfd, [small[1], ovf[1], small[1]], [F, F, F], api)
        s2 = eng.stats().host_syncs
        check([small, small], res2, api)
        check([small, ovf, small], res3, api)
        assert res3[0] == res2[0] and res3[2] == res2[1]
        assert [ln["overflow"] for ln in l2] == [0] and [ln["overflow"] for ln in l3] == [1]
        assert l3[0]["overflow_bytes"] == (ovf[6] + 15) // 16 * 16
        assert (s2 - s1) - (s1 - s0) == 1, (s0, s1, s2)


def test_empty_batch_and_bad_kind(eng):
    from hocuspocus_amd.engine import EINVAL, YjsError, _Result, lib
    st, js, _ = jf.edge("a paragraph without children")
    assert eng.json_batch([], []) == []
    assert eng.json_device(0, 0, 0, 0, 0, 0).payload_bytes == 0
    assert eng.json_batch([st], ["default"]) == [js]
    assert eng.json_batch([st], [""]) == [b'{"type":"doc","content":[]}']      # every name empty: no names arena
    off = np.array([0, len(st)], np.uint64)
    noff = np.array([0, 7], np.uint64)
    res = _Result()
    for kind in (1, 2, 0xFFFFFFFF):
        rc = lib().ygm_json_v1(eng._ctx, ctypes.c_char_p(st), off.ctypes.data_as(ctypes.c_void_p), ctypes.c_char_p(F),
                               noff.ctypes.data_as(ctypes.c_void_p), kind, 1, ctypes.byref(res))
        assert rc == EINVAL
        with pytest.raises(YjsError) as e:
            eng.json_device(0, 0, 0, 0, 0, 0, kind=kind)
        assert e.value.code == EINVAL
        with pytest.raises(YjsError):
            eng.json_batch([st], ["default"], kind=kind)


def test_two_chunks_equal_one(eng, capfd, monkeypatch):
    rows = jf.expectations()
    states, names = [r[1] for r in rows], [r[2] for r in rows]
    assert sum(map(len, states)) > (2 << 20)
    one, l1 = run(eng, capfd, states, names)
    monkeypatch.setenv("YGM_CHUNK_MB", "5")      # (8.4 MB of states: two chunks)
    two, l2 = run(eng, capfd, states, names)
    assert len(l1) == 1 and len(l2) == 2
    assert one == two
    check(rows, two, "two chunks")

"""The host API's chunk pipeline on the entry points no other test cuts into chunks: the V1 merge (the one path whose
lean launch is enqueued before the next chunk is staged), SV, diff, contains, the shared diff, the V2 SV, both
conversions, and text (flat and deep).  Each takes a batch whose primary arena is a little over 2 MB, runs it whole and
with YGM_CHUNK_MB=1 (read per call), and asserts: the chunked rows equal the unchunked ones (status, length, bytes),
the call really was chunked (stats().calls rose by at least 3), and the unchunked rows equal the CPU oracle or the
fixture's recorded expectation.  Then one zero-document call per entry point, and a merge batch holding a document
with no updates: both go through the same pipeline.

Snapshot and step2 with options, the shared step2, version take / restore, the shared restore and the V2 merge / diff
have chunked runs beside their own tests."""
import numpy as np
import pytest

import oracle
import text_fixture as tf
from devrun import engine_fixture
from golden import contains_fixtures, history_docs
from v1util import rd_vu, vu

pytestmark = pytest.mark.gpu

MB = 1 << 20
EMPTY = bytes.fromhex("0000")   # the update of a document with no structs and no deletions


eng = engine_fixture()


def _fill(rows, size):
    """`rows` repeated in order until their primary bytes pass 2 MB by a little; asserts 2 MB < bytes < 3 MB."""
    out, total = [], 0
    while total <= 2 * MB + 100000:
        out.append(rows[len(out) % len(rows)])
        total += size(out[-1])
    assert 2 * MB < total < 3 * MB, total
    return out


def _pin(eng, monkeypatch, call):
    """call() whole, then in 1 MB chunks: row for row the same, and really chunked.  -> the unchunked rows."""
    monkeypatch.delenv("YGM_CHUNK_MB", raising=False)
    ref = call()
    monkeypatch.setenv("YGM_CHUNK_MB", "1")
    s0 = eng.stats().calls
    got = call()
    assert eng.stats().calls - s0 >= 3, "the batch was not chunked"
    assert len(got) == len(ref)
    bad = [k for k in range(len(ref)) if got[k] != ref[k]]
    assert not bad, (len(bad), bad[:5])
    return ref


@pytest.fixture(scope="module")
def logs():
    """C2-shaped logs (tools/synth.text_updates), the leading documents whose updates are a little over 2 MB, with what
    the oracle makes of them: per document its updates, the merged state, the state vector of the merged first half of
    the log, and the merged state as update V2."""
    from tools import synth
    arena, upd_off, doc_upd = synth.text_updates(1400, 200, 1, 4, seed=5)
    n = int(np.searchsorted(upd_off[doc_upd], 2 * MB + 100000, side="right"))   # the first n documents end past it
    assert n < len(doc_upd) - 1
    n_upd = int(doc_upd[n])
    total = int(upd_off[n_upd])
    assert 2 * MB < total < 3 * MB, total
    ups = synth.split(arena[:total], upd_off[:n_upd + 1])
    docs = [ups[int(doc_upd[d]):int(doc_upd[d + 1])] for d in range(n)]
    merged, half, v2 = [], [], []
    for us in docs:
        st, m = oracle.merge_updates(us)
        assert st == 0
        merged.append(m)
        st, sv = oracle.encode_state_vector_from_update(oracle.merge_updates(us[:len(us) // 2])[1])
        assert st == 0
        half.append(sv)
        st, x = oracle.convert_update_format_v1_to_v2(m)
        assert st == 0
        v2.append(x)
    return {"arena": np.ascontiguousarray(arena[:total]), "upd_off": np.ascontiguousarray(upd_off[:n_upd + 1]),
            "upd_doc": np.repeat(np.arange(n, dtype=np.uint32), np.diff(doc_upd[:n + 1].astype(np.int64))),
            "docs": docs, "merged": merged, "half": half, "v2": v2}


# ---------------------------------------------------------------------------------------- update V1
def test_merge_v1_chunked(eng, monkeypatch, logs):
    """ygm_merge_v1: the chunks alternate between the two stage contexts, each chunk's lean launch enqueued before the
    next chunk is staged."""
    n = len(logs["docs"])
    ref = _pin(eng, monkeypatch, lambda: eng.merge_packed(logs["arena"], logs["upd_off"], logs["upd_doc"], n))
    assert ref == [(0, m) for m in logs["merged"]]


def test_merge_v1_chunked_with_an_empty_document(eng, monkeypatch, logs):
    """The same batch with a document of no updates before every 100th document and one at the end: each comes out as
    the empty update wherever the chunk edges fall."""
    n = len(logs["docs"])
    gaps = np.cumsum([1 if d and d % 100 == 0 else 0 for d in range(n)]).astype(np.uint32)   # empty documents before d
    ids = (np.arange(n, dtype=np.uint32) + gaps)
    upd_doc = np.repeat(ids, [len(us) for us in logs["docs"]]).astype(np.uint32)
    total = int(ids[-1]) + 2
    ref = _pin(eng, monkeypatch, lambda: eng.merge_packed(logs["arena"], logs["upd_off"], upd_doc, total))
    exp = [(0, EMPTY)] * total
    for d in range(n):
        exp[int(ids[d])] = (0, logs["merged"][d])
    assert sum(1 for e in exp if e == (0, EMPTY)) == int(gaps[-1]) + 1 >= 3
    assert ref == exp


def test_sv_v1_chunked(eng, monkeypatch, logs):
    base = [(m, oracle.encode_state_vector_from_update(m)) for m in logs["merged"]]
    rows = _fill(base, lambda r: len(r[0]))
    ref = _pin(eng, monkeypatch, lambda: eng.encode_state_vector_from_update_batch([r[0] for r in rows]))
    assert ref == [r[1] for r in rows]


def test_diff_v1_chunked(eng, monkeypatch, logs):
    base = [(m, sv, oracle.diff_update(m, sv)) for m, sv in zip(logs["merged"], logs["half"])]
    rows = _fill(base, lambda r: len(r[0]))
    ref = _pin(eng, monkeypatch, lambda: eng.diff_update_batch([r[0] for r in rows], [r[1] for r in rows]))
    assert ref == [r[2] for r in rows]
    assert all(st == 0 and len(b) > 2 for st, b in ref[:50])   # (the second half of the log: real diffs)


def test_contains_chunked(eng, monkeypatch):
    rows = _fill(contains_fixtures(), lambda r: len(r[0]))
    ref = _pin(eng, monkeypatch, lambda: eng.contains_batch([r[0] for r in rows], [r[1] for r in rows]))
    assert ref == [(0, r[2]) for r in rows]


def _scaled_sv(sv, num, den):
    """The state vector with every clock scaled by num / den."""
    n, p = rd_vu(sv, 0)
    o = bytearray(vu(n))
    for _ in range(n):
        c, p = rd_vu(sv, p)
        k, p = rd_vu(sv, p)
        o += vu(c) + vu(k * num // den)
    return bytes(o)


def test_diff_shared_chunked(eng, monkeypatch):
    """Three updates, the middle one about 300 KB with six asks: 2.1 MB of virtual bytes, so it is split over chunks
    that each stage it again; small ones before and after it."""
    docs = history_docs()
    big = [d for d in docs if d["family"] == "large"][0]["state"]
    small = [d["state"] for d in docs if d["family"] == "clients"][:2]
    assert 250000 < len(big) < 400000
    st, full = oracle.encode_state_vector_from_update(big)
    assert st == 0
    svs_big = [b"\x00", full, _scaled_sv(full, 1, 2), _scaled_sv(full, 1, 4), _scaled_sv(full, 3, 4), _scaled_sv(full, 9, 10)]
    updates = [small[0], big, small[1]]
    asks = [(0, b"\x00"), (0, oracle.encode_state_vector_from_update(small[0])[1])]
    asks += [(1, sv) for sv in svs_big]
    asks += [(2, b"\x00"), (2, _scaled_sv(oracle.encode_state_vector_from_update(small[1])[1], 1, 2))]
    virtual = sum(len(u) for u in updates) + sum(len(updates[a]) for a, _ in asks)
    assert 2 * MB < virtual < 3 * MB, virtual
    ref = _pin(eng, monkeypatch, lambda: eng.diff_update_shared_batch(updates, [a for a, _ in asks], [sv for _, sv in asks]))
    assert ref == [oracle.diff_update(updates[a], sv) for a, sv in asks]
    assert len({b for _, b in ref[2:8]}) == 6   # (six different answers from the one split update)


# ---------------------------------------------------------------------------------------- update V2
def test_sv_v2_chunked(eng, monkeypatch, logs):
    base = [(x, oracle.encode_state_vector_from_update_v2(x)) for x in logs["v2"]]
    rows = _fill(base, lambda r: len(r[0]))
    ref = _pin(eng, monkeypatch, lambda: eng.encode_state_vector_from_update_v2_batch([r[0] for r in rows]))
    assert ref == [r[1] for r in rows]
    assert all(st == 0 for st, _ in ref)


def test_convert_v1_to_v2_chunked(eng, monkeypatch, logs):
    base = [(m, oracle.convert_update_format_v1_to_v2(m)) for m in logs["merged"]]
    rows = _fill(base, lambda r: len(r[0]))
    ref = _pin(eng, monkeypatch, lambda: eng.convert_update_format_v1_to_v2_batch([r[0] for r in rows]))
    assert ref == [r[1] for r in rows]


def test_convert_v2_to_v1_chunked(eng, monkeypatch, logs):
    base = [(x, oracle.convert_update_format_v2_to_v1(x)) for x in logs["v2"]]
    rows = _fill(base, lambda r: len(r[0]))
    ref = _pin(eng, monkeypatch, lambda: eng.convert_update_format_v2_to_v1_batch([r[0] for r in rows]))
    assert ref == [r[1] for r in rows]
    assert all(st == 0 for st, _ in ref)


# ---------------------------------------------------------------------------------------- text
@pytest.mark.parametrize("deep", [False, True])
def test_text_chunked(eng, monkeypatch, deep):
    """Each chunk carries its slice of the root names (the second arena)."""
    rows = _fill(tf.expectations(), lambda r: len(r[1]))

    def call():
        return [(0, r) if isinstance(r, bytes) else (r.code, None) for r in eng.text_batch([r[1] for r in rows], [r[2] for r in rows], deep=deep)]
    ref = _pin(eng, monkeypatch, call)
    assert ref == [(0, r[4] if deep else r[3]) for r in rows]


# ---------------------------------------------------------------------------------------- nothing to do
@pytest.mark.parametrize("chunk_mb", [None, "1"])
def test_zero_documents(eng, monkeypatch, chunk_mb):
    """Every entry point of this file with an empty batch: YGM_OK and no rows."""
    if chunk_mb is None:
        monkeypatch.delenv("YGM_CHUNK_MB", raising=False)
    else:
        monkeypatch.setenv("YGM_CHUNK_MB", chunk_mb)
    assert eng.merge_updates_batch([]) == []
    assert eng.merge_packed(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), 0) == []
    assert eng.encode_state_vector_from_update_batch([]) == []
    assert eng.diff_update_batch([], []) == []
    assert eng.contains_batch([], []) == []
    assert eng.diff_update_shared_batch([], [], []) == []
    assert eng.diff_update_shared_batch([EMPTY], [], []) == []   # (a state nobody asks about)
    assert eng.encode_state_vector_from_update_v2_batch([]) == []
    assert eng.convert_update_format_v1_to_v2_batch([]) == []
    assert eng.convert_update_format_v2_to_v1_batch([]) == []
    assert eng.text_batch([], []) == [] and eng.text_batch([], [], deep=True) == []
    assert eng.merge_updates_batch([[]]) == [(0, EMPTY)]   # (and a batch of one document with no updates)

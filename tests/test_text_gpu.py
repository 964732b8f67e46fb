"""Plain text of stored documents on the GPU (ygm_text_v1 / ygm_text_v1_device: k_text_flat with 6 KiB, then 24 KiB of
LDS, then the snapshot's count / scan launches and k_text).

Fixture parity: every expectation of tests/golden/text_v135.json.gz (yjs 13.5.16: getText(name).toString() and the deep
walker) through the host and the device form, in a 13.5 and a default context -- the text depends on neither.  Then the
flat tier against the snapshot tiers (the same envelope and LDS sizes: the same counts on the call's tier line), the
flat tier's edges on hand-made updates whose text is known by construction (the emit's own-lane / whole-wave threshold
of 16 bytes, the 64-lane stride, the 16-client table, every arena residue with two tail paddings, the scanned
workspace offsets across block edges, buffers reused from call to call), and the statuses."""
import ctypes
import re

import numpy as np
import pytest

import snapshot_tier_docs as g
import text_fixture as tf
from devrun import engine_fixture, read_results, upload

pytestmark = pytest.mark.gpu

TEXT_LINE = re.compile(r"^ygm text tiers: docs (\d+) flat_first (\d+) flat_second (\d+) general (\d+)$", re.M)
SNAP_LINE = re.compile(r"^ygm snapshot tiers: docs (\d+) text_first (\d+) text_second (\d+) general (\d+) pending (\d+)$", re.M)
KNOBS = ("YGM_SNAP_NOLDS", "YGM_SNAP_TEXT", "YGM_SNAP_DPW", "YGM_CHUNK_MB")
T = b"t"      # the root name of the hand-made documents (snapshot_tier_docs.ROOT)


@pytest.fixture(autouse=True)
def tier_counts(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _engine(compat135):
    from hocuspocus_amd import Engine
    return Engine(0, compat135=compat135)


eng135 = engine_fixture(compat135=True)
eng136 = engine_fixture(compat135=False)


def host_text(eng, states, names, deep):
    """Engine.text_batch as (status, bytes | None) pairs."""
    return [(0, r) if isinstance(r, bytes) else (r.code, None) for r in eng.text_batch(states, names, deep=deep)]


def device_text(eng, states, names, deep, tail=0x00):
    """ygm_text_v1_device over arenas from torch, the 64 bytes after each set to `tail` -> (status, bytes | None)."""
    ta, to, nbytes = upload(states, tail=tail)
    tn, tno, _ = upload(names, tail=tail)
    assert ta.data_ptr() % 16 == 0
    n = len(states)
    r = eng.text_device(ta, nbytes, to, tn, tno, n, deep=deep)
    res, offs, lens = read_results(r, n, places=True)
    assert int(r.payload_bytes) == sum(lens[d] for d in range(n) if res[d][0] == 0)
    for d in range(n):
        assert res[d][0] != 0 or offs[d] + lens[d] <= int(r.data_bytes)
    return res


def run(eng, capfd, states, names, deep=False, api="batch", tail=0x00):
    """One call: its results and its tier line as a dict."""
    capfd.readouterr()
    res = host_text(eng, states, names, deep) if api == "batch" else device_text(eng, states, names, deep, tail)
    lines = TEXT_LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1, lines
    return res, dict(zip(("docs", "flat_first", "flat_second", "general"), map(int, lines[0])))


# ---------------------------------------------------------------- fixture parity
def _batches():
    """The fixture in a handful of batches: one per input set, one of the edge sessions."""
    out = [(s, tf.expectations(sets=(s,), edges=False)) for s in tf.SETS]
    out.append(("edges", tf.expectations(sets=(), edges=True)))
    return out


@pytest.mark.parametrize("api", ["batch", "device"])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("deep", [False, True])
def test_fixture_parity(eng135, eng136, capfd, deep, compat, api):
    """Bytes and statuses of every expectation; the pending set's rows (states that leave pending parts) are OK."""
    eng = eng135 if compat else eng136
    total = 0
    for what, rows in _batches():
        res, c = run(eng, capfd, [r[1] for r in rows], [r[2] for r in rows], deep, api)
        exp = [(0, r[4] if deep else r[3]) for r in rows]
        bad = [k for k in range(len(rows)) if res[k] != exp[k]]
        assert not bad, (what, len(bad), [(rows[k][0], rows[k][2], res[k][0], res[k][1] and res[k][1][:40], exp[k][1][:40]) for k in bad[:4]])
        assert c["docs"] == len(rows)
        total += len(rows)
    assert total == 1340 + 4269 + sum(len(e["roots"]) for e in tf.load()["edges"])


# ---------------------------------------------------------------- the flat tier against the snapshot tiers
@pytest.mark.parametrize("compat", [True, False])
def test_flat_tier_takes_what_the_snapshot_text_tier_takes(eng135, eng136, capfd, compat):
    """The whole snapshot_text_v135 batch asked by its root name: the flat tier's two launches take the documents
    k_snap_text's two launches take in a snapshot call of the same batch on the same context (the same envelope and LDS
    sizes).  One state of the batch is the struct-less update 00 00 (an empty document): it names no root, so no asked
    name can equal its root name and the flat tier leaves it to k_text whatever is asked, while the snapshot's first
    launch takes it.  It is counted apart, so that asked by another name the flat tier takes nothing at all."""
    eng = eng135 if compat else eng136
    states = tf.set_states("snapshot_text_v135")
    rootless = sum(s == b"\x00\x00" for s in states)
    assert rootless == 1 and all(b"\x01\x04text" in s for s in states if s != b"\x00\x00")
    exp = {r[0]: r for r in tf.expectations(sets=("snapshot_text_v135",), edges=False) if r[2] == b"text"}
    capfd.readouterr()
    eng.snapshot_batch(states)
    snap = SNAP_LINE.findall(capfd.readouterr().err)
    assert len(snap) == 1, snap
    text_first, text_second = int(snap[0][1]), int(snap[0][2])
    assert text_first + text_second > 0
    for deep in (False, True):      # both modes share the tier
        res, c = run(eng, capfd, states, [b"text"] * len(states), deep)
        assert (c["flat_first"] + rootless, c["flat_second"]) == (text_first, text_second), (c, snap)
        for k in range(len(states)):
            r = exp.get("snapshot_text_v135[%d]" % k)
            assert res[k] == (0, r[3] if r else b""), k
    # asked by another name: nothing for the flat tier, every text empty
    res, c = run(eng, capfd, states, [b"texu"] * len(states))
    assert (c["flat_first"], c["flat_second"], c["general"]) == (0, 0, len(states))
    assert res == [(0, b"")] * len(states)
    res, c = run(eng, capfd, states, [b"tex"] * len(states), api="device")
    assert (c["flat_first"], c["flat_second"]) == (0, 0) and res == [(0, b"")] * len(states)


# ---------------------------------------------------------------- flat-tier edges (texts known by construction)
def letters(n, seed=0):
    return bytes(97 + (seed + 7 * i + i // 26) % 26 for i in range(n))


def one_string(n):
    """Live text of n bytes in one part (n = 0: one deleted run)."""
    return (g.update([g.block(5, 0, [g.s(letters(n, n))])]), letters(n, n)) if n else (g.update([g.block(5, 0, [g.dl(3)])]), b"")


def chain(lens, client=7, deleted=()):
    """Strings of the given lengths by one client, each typed after the one before; `deleted`: indices of strings a
    delete range covers whole.  -> (update, text)"""
    out, ck, text, rs = [], 0, b"", []
    for i, L in enumerate(lens):
        txt = letters(L, i)
        out.append(g.s(txt, origin=(client, ck - 1)) if ck else g.s(txt))
        if i in deleted:
            rs.append((ck, L))
        else:
            text += txt
        ck += L
    return g.update([g.block(client, 0, out)], [(client, rs)] if rs else ()), text


LIVE = (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)
PARTS = (1, 63, 64, 65, 129)


def edge_docs():
    """[(what, update, text, tier)]: tier 'flat' (k_text_flat takes it) or 'general'."""
    D = []
    for n in LIVE:
        u, t = one_string(n)
        D.append(("live text of %d bytes" % n, u, t, "flat"))
    for k in PARTS:
        for what, lens in (("short", [6] * k), ("long", [17 + (i % 5) for i in range(k)]),
                           ("mixed", [(1, 16, 17, 40, 2, 64, 65, 3)[i % 8] for i in range(k)])):
            u, t = chain(lens)
            D.append(("%d %s parts" % (k, what), u, t, "flat"))
        u, t = chain([(5, 30)[i % 2] for i in range(k)], deleted=set(range(0, k, 3)))
        D.append(("%d parts, every third deleted" % k, u, t, "flat"))
    u, t = chain([6] * 70, deleted=set(range(70)))
    assert t == b""
    D.append(("every part deleted", u, t, "flat"))
    # 16 client blocks fill the flat tier's client table; a 17th (one deleted clock: the same text) goes to k_text.
    # Concurrent inserts at the list's start order by client id, ascending.
    ids = sorted(1000 + 37 * i for i in range(17))
    blocks = [g.block(c, 0, [g.s(bytes([97 + i]) * 2)]) for i, c in enumerate(ids[:16])]
    text16 = b"".join(bytes([97 + i]) * 2 for i in range(16))
    D.append(("16 clients", g.update(blocks[::-1]), text16, "flat"))
    D.append(("17 clients", g.update(([g.block(ids[16], 0, [g.dl(1)])] + blocks[::-1])), text16, "general"))
    D.append(("a two-byte letter", g.update([g.block(5, 0, [g.s("aé€b")])]), "aé€b".encode(), "general"))
    return D


def check(res, docs, what):
    bad = [k for k in range(len(docs)) if res[k] != (0, docs[k][2])]
    assert not bad, (what, [(docs[k][0], res[k][0], res[k][1] and res[k][1][:48], docs[k][2][:48]) for k in bad[:5]])


@pytest.mark.parametrize("api", ["batch", "device"])
@pytest.mark.parametrize("deep", [False, True])
def test_flat_tier_edges(eng135, eng136, capfd, deep, api):
    docs = edge_docs()
    for eng in (eng135, eng136):
        res, c = run(eng, capfd, [d[1] for d in docs], [T] * len(docs), deep, api)
        check(res, docs, (deep, api))
        flat = sum(d[3] == "flat" for d in docs)
        assert c["flat_first"] + c["flat_second"] == flat and c["general"] == len(docs) - flat, c
        assert c["flat_second"] == 0      # (129 parts and 1 025 bytes fit the first launch's 207 parts)


def test_flat_tier_second_launch(eng135, capfd):
    """Past the first launch's 207 parts: taken with 24 KiB; past 865: k_text.  The same text from all three."""
    docs = []
    for k in (g.CAP_FIRST, g.CAP_FIRST + 1, g.CAP_SECOND, g.CAP_SECOND + 1):
        u, t = chain([3 + i % 4 for i in range(k)])
        docs.append(("%d parts" % k, u, t, None))
    res, c = run(eng135, capfd, [d[1] for d in docs], [T] * len(docs), api="device")
    check(res, docs, "caps")
    assert (c["flat_first"], c["flat_second"], c["general"]) == (1, 2, 1), c


def test_every_arena_residue_and_both_tail_paddings(eng135, capfd):
    """A flat and a general document behind fillers, starting at every residue 0 .. 15 of the arena, the 64 bytes after
    both arenas 0xFF and then 0x00; then each as the last document of its arena."""
    targets = [chain([1, 16, 17, 40, 2, 64, 65, 3]), (g.update([g.block(5, 0, [g.s("aé€b" * 9)])]), ("aé€b" * 9).encode())]
    docs, at = [], 0
    for u, t in targets:
        for r in range(16):
            size = 11 + (r - at - 11) % 16
            docs += [("filler", g.filler(size), b"f" * (size - 10), None), ("target at residue %d" % r, u, t, None)]
            at += size + len(u)
            assert (at - len(u)) % 16 == r
    runs = []
    for tail in (0xFF, 0x00):
        res, c = run(eng135, capfd, [d[1] for d in docs], [T] * len(docs), api="device", tail=tail)
        check(res, docs, ("residues", tail))
        assert c["general"] == 16
        runs.append(res)
    assert runs[0] == runs[1]
    for k, (u, t) in enumerate(targets):
        last = [docs[2 * j] for j in range(3 + k)] + [("last", u, t, None)]
        for tail in (0xFF, 0x00):
            res, _ = run(eng135, capfd, [d[1] for d in last], [T] * len(last), api="device", tail=tail)
            check(res, last, ("last", k, tail))


def test_4097_one_struct_documents(eng136, capfd):
    """Scan block edges (256 documents a block): every third document has a two-byte letter and takes k_text, whose
    workspace lies at its scanned offset; the others are claimed by the flat tier and skipped there."""
    docs = []
    for k in range(4097):
        txt = (letters(1 + k % 23, k) + "é".encode()) if k % 3 == 0 else letters(1 + k % 29, k)
        docs.append(("doc %d" % k, g.update([g.block(1 + k % 100, 0, [g.s(txt)])]), txt, None))
    for api in ("device", "batch"):
        res, c = run(eng136, capfd, [d[1] for d in docs], [T] * len(docs), api=api)
        check(res, docs, ("4097", api))
        assert (c["flat_first"], c["flat_second"], c["general"]) == (4097 - 1366, 0, 1366), c


def test_large_then_small_batch_on_one_context(capfd):
    """Stale claim bytes, slots and workspaces of a large batch under a small one, and a snapshot call in between."""
    docs = edge_docs()
    big = docs * 6
    small = [docs[-1], docs[3], docs[-2]]
    eng = _engine(True)
    try:
        for what, batch, api in (("large", big, "device"), ("small", small, "device"), ("large", big, "batch"), ("small", small, "batch")):
            res, c = run(eng, capfd, [d[1] for d in batch], [T] * len(batch), True, api)
            check(res, batch, what)
            assert c["general"] == sum(d[3] == "general" for d in batch)
            eng.snapshot_batch([d[1] for d in small])
    finally:
        eng.close()


# ---------------------------------------------------------------- statuses
def test_statuses_are_the_snapshots_and_touch_no_neighbour(eng135, eng136, capfd):
    good = edge_docs()[:12]
    bad = [g.SMALL[:len(g.SMALL) - 3], g.SMALL[:5], g.get("B a client block twice").u, g.get("B client id 2^32").u,
           g.get("B delete range ending at 2^32").u, b""]
    states, names, exp = [], [], []
    for k, b in enumerate(bad):
        states += [good[2 * k][1], b, good[2 * k + 1][1]]
        names += [T] * 3
        exp += [good[2 * k][2], None, good[2 * k + 1][2]]
    for eng in (eng135, eng136):
        snap = eng.snapshot_batch(states)
        assert all(snap[3 * k + 1][0] != 0 for k in range(len(bad)))
        assert {snap[3 * k + 1][0] for k in range(len(bad))} >= {1, 9}      # EMALFORMED and EUNSUPPORTED are both met
        for api in ("batch", "device"):
            for deep in (False, True):
                res, _ = run(eng, capfd, states, names, deep, api)
                for k in range(len(states)):
                    if exp[k] is None:
                        assert res[k] == (snap[k][0], None), (k, res[k], snap[k][0])
                    else:
                        assert res[k] == (0, exp[k]), k
    # a state that leaves pending parts is read through its integrated part
    pend = [g.get("B first clock 3").u, g.get("B delete range past the state").u, g.get("B one Skip").u]
    res, _ = run(eng135, capfd, pend, [T] * 3)
    assert res == [(0, b""), (0, b"a"), (0, b"ab")]


def test_bad_mode_and_empty_batch(eng135):
    from hocuspocus_amd.engine import EINVAL, YjsError, _Result, lib
    u, _ = one_string(5)
    off = np.array([0, len(u)], np.uint64)
    noff = np.array([0, 1], np.uint64)
    res = _Result()
    for mode in (2, 7, 0xFFFFFFFF):
        st = lib().ygm_text_v1(eng135._ctx, ctypes.c_char_p(u), off.ctypes.data_as(ctypes.c_void_p), ctypes.c_char_p(T),
                               noff.ctypes.data_as(ctypes.c_void_p), mode, 1, ctypes.byref(res))
        assert st == EINVAL
        with pytest.raises(YjsError) as e:
            eng135.text_device(0, 0, 0, 0, 0, 0, mode=mode)
        assert e.value.code == EINVAL
    assert eng135.text_batch([], []) == []
    assert eng135.text_batch([], [], deep=True) == []
    r = eng135.text_device(0, 0, 0, 0, 0, 0)
    assert r.payload_bytes == 0
    assert eng135.text_batch([u], [""]) == [b""]      # every name empty: no names arena
    assert eng135.text_batch([u], ["t"]) == [letters(5, 5)]

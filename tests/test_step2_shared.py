"""Shared-state SyncStep2 / diffUpdate (ygm_sync_step2_shared_v1, ygm_diff_shared_v1): n_states states, n_asks state
vectors, ask a answered from states[ask_state[a]] -- a reconnect storm costs one upload and one snapshot per document,
not per client.  Every entry must be byte-identical to the per-pair reply, so every expected value here comes from the
yjs 13.5.16 fixtures (tests/golden/step2_v135.json.gz, step2_pending_v135.json.gz: one state x several state
vectors) or from the CPU oracle over yjs's own snapshot of the state -- never from the engine."""
import functools
import gzip
import json
import os

import pytest

import oracle
from devrun import engine_fixture
from v1util import rd_vu, vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EINVAL, EUNSUPPORTED = 8, 9

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def rows():
    d = json.load(gzip.open(os.path.join(GOLD, "step2_v135.json.gz"), "rt"))
    return tuple((bytes.fromhex(u), bytes.fromhex(sv), None if e is None else bytes.fromhex(e)) for u, sv, e, _eq in d["rows"])


@functools.lru_cache(maxsize=None)
def pending_rows():
    d = json.load(gzip.open(os.path.join(GOLD, "step2_pending_v135.json.gz"), "rt"))
    return tuple((bytes.fromhex(u), bytes.fromhex(sv), None if e is None else bytes.fromhex(e)) for u, sv, e, _eq in d["rows"])


@functools.lru_cache(maxsize=None)
def yjs_snapshots():
    """state -> yjs 13.5.16 encodeStateAsUpdate(applyUpdate(new Doc, state))"""
    out = {b"\x00\x00": b"\x00\x00"}   # (the empty document's state is its own snapshot)
    for f in ("snapshot_v135.json.gz", "snapshot_text_v135.json.gz"):
        for u, e in json.load(gzip.open(os.path.join(GOLD, f), "rt"))["rows"]:
            out[bytes.fromhex(u)] = bytes.fromhex(e)
    return out


def group(triples):
    """(state, sv, expected) rows -> states (distinct, first-seen order), ask_state (non-decreasing), svs, expected"""
    ix = {}
    for u, *_ in triples:
        ix.setdefault(u, len(ix))
    asks = sorted(triples, key=lambda t: ix[t[0]])   # (stable: a state's asks keep their order)
    return list(ix), [ix[u] for u, *_ in asks], [sv for _, sv, _ in asks], [e for *_, e in asks]


def differing(res, exp):
    """indices where a reply is not yjs's: bytes for a row yjs answered, the 13.5 surrogate refusal (4) for a null row"""
    return [k for k, (g, e) in enumerate(zip(res, exp)) if (g[0] != 4 if e is None else g != (0, e))]


eng135 = engine_fixture(compat135=True)


# ---------------------------------------------------------------------------------------- 1: the fixture, grouped
def test_step2_fixture_grouped_by_state(eng135):
    states, ask_state, svs, exp = group(rows())
    assert len(states) == 759 and len(svs) == 2280
    s0 = eng135.stats()
    res = eng135.sync_step2_shared_batch(states, ask_state, svs)
    s1 = eng135.stats()
    bad = differing(res, exp)
    assert not bad, f"{len(bad)} replies differ from yjs, first {bad[:5]}: {res[bad[0]]}"
    assert s1.docs_snapshot - s0.docs_snapshot == 759   # one snapshot per state, not per ask


# ---------------------------------------------------------------------------------------- 2: states with lost updates
def test_step2_pending_states_grouped_and_mixed(eng135):
    pstates, _, _, _ = group(pending_rows())
    assert len(pstates) == 580 and len(pending_rows()) == 2320
    pset = set(pstates)
    cstates = [u for u in group(rows())[0] if u not in pset][:100]   # (complete states the pending corpus does not hold)
    by_state = {}
    for u, sv, e in pending_rows() + tuple(r for r in rows() if r[0] not in pset):
        by_state.setdefault(u, []).append((u, sv, e))
    order, ci = [], 0
    for k, u in enumerate(pstates):   # a complete state after every sixth pending one (580 / 6 < 100: the rest follow)
        order.append(u)
        if k % 6 == 5 and ci < len(cstates):
            order.append(cstates[ci])
            ci += 1
    order += cstates[ci:]
    triples = [t for u in order for t in by_state[u]]
    states, ask_state, svs, exp = group(triples)
    assert states == order and len(svs) == 2320 + sum(len(by_state[u]) for u in cstates)
    s0 = eng135.stats()
    res = eng135.sync_step2_shared_batch(states, ask_state, svs)
    s1 = eng135.stats()
    bad = differing(res, exp)
    assert not bad, f"{len(bad)} replies differ from yjs, first {bad[:5]}: {res[bad[0]]}"
    assert s1.docs_pending > s0.docs_pending
    assert s1.docs_snapshot - s0.docs_snapshot == len(states)


# ---------------------------------------------------------------------------------------- 3: storm and gather shapes
def decode_sv(b):
    n, p = rd_vu(b, 0)
    out = []
    for _ in range(n):
        c, p = rd_vu(b, p)
        k, p = rd_vu(b, p)
        out.append((c, k))
    return out


def encode_sv(ents):
    return vu(len(ents)) + b"".join(vu(c) + vu(k) for c, k in ents)


def own_sv(snap):
    st, sv = oracle.encode_state_vector_from_update(snap, compat135=True)
    assert st == 0
    return decode_sv(sv)


def storm_svs(snap, n, truncated_at=None):
    """n state vectors for one state: cuts of its own vector at evenly spaced clocks, the empty vector first, every
    seventh with 17 extra unknown clients (over the walker's 16-entry table: the exact kernel), one truncated"""
    own = own_sv(snap)
    out = []
    for i in range(n):
        if i == 0:
            sv = b"\x00"
        else:
            cut = [(c, k * i // n) for c, k in own]
            if i % 7 == 6:
                cut += [(0x7F000000 + 3 * j, 5 + j) for j in range(17)]
            sv = encode_sv(cut)
        if i == truncated_at:
            sv = encode_sv([(c, k // 2) for c, k in own] + [(77, 300)])[:-1]   # (the last clock's final byte missing)
        out.append(sv)
    return out


# a client block repeated (yjs's writers never do): "a" by client 1, then a second block of client 1
REPEATED = bytes.fromhex("02" "010100" "040101610178" "010101" "8401000179" "00")


@functools.lru_cache(maxsize=None)
def storm():
    """states, ask_state, svs, expected (status, bytes) of the storm shape"""
    snaps = yjs_snapshots()
    uniq = group(rows())[0]
    big = max(uniq, key=len)
    assert len(big) == 14750 and len(own_sv(snaps[big])) == 1
    multi = [u for u in uniq if len(own_sv(snaps[u])) >= 3][:2]
    assert len(multi) == 2
    states = [big, multi[0], multi[1], b"\x00\x00", REPEATED]
    counts = [257, 0, 65, 1, 3]   # one over the walker's batch of 256; none; one over a wave; one; three
    ask_state, svs, exp = [], [], []
    for s, (u, n) in enumerate(zip(states, counts)):
        if u is REPEATED:
            v = [b"\x00", encode_sv([(1, 1)]), encode_sv([(1, 2)])]
            e = [(EUNSUPPORTED, None)] * n
        else:
            v = storm_svs(snaps[u], n, truncated_at=5 if s == 0 else None)
            e = [oracle.diff_update(snaps[u], sv, compat135=True, keep_sub=True) for sv in v]
        ask_state += [s] * n
        svs += v
        exp += e
    return states, ask_state, svs, exp


def test_storm_and_gather_shapes(eng135):
    states, ask_state, svs, exp = storm()
    assert len(svs) == 326 and ask_state != list(range(len(ask_state)))
    assert exp[5][0] != 0 and exp[4][0] == 0 and exp[6][0] == 0   # the truncated vector fails, its neighbours do not
    assert sum(1 for st, _ in exp[:257] if st == 0) >= 200
    s0 = eng135.stats()
    res = eng135.sync_step2_shared_batch(states, ask_state, svs)
    s1 = eng135.stats()
    bad = [k for k, (g, e) in enumerate(zip(res, exp)) if g != e]
    assert not bad, f"{len(bad)} of {len(exp)} differ, first {bad[:5]}: got {res[bad[0]]} expected {exp[bad[0]]}"
    assert [g[0] for g in res[-3:]] == [EUNSUPPORTED] * 3
    assert s1.docs_snapshot - s0.docs_snapshot == 5
    assert s1.docs_fast > s0.docs_fast   # the 17-client vectors went through the exact kernel


# ---------------------------------------------------------------------------------------- 4: the plain shared diff
def test_diff_update_shared_batch(eng135):
    snaps = yjs_snapshots()
    states, ask_state, svs, _ = group(rows())
    upd = [snaps[u] for u in states]
    exp = [oracle.diff_update(upd[s], sv, compat135=True) for s, sv in zip(ask_state, svs)]
    s0 = eng135.stats()
    res = eng135.diff_update_shared_batch(upd, ask_state, svs)
    s1 = eng135.stats()
    bad = [k for k, (g, e) in enumerate(zip(res, exp)) if g != (e if e[0] == 0 else (e[0], None))]
    assert not bad, f"{len(bad)} differ, first {bad[:5]}: got {res[bad[0]]} expected {exp[bad[0]]}"
    assert s1.docs_snapshot == s0.docs_snapshot   # no snapshot in a plain diff
    from hocuspocus_amd import Engine
    lo, hi = 600, 900   # (asks of whole states: the slice is cut at state boundaries)
    while ask_state[lo] == ask_state[lo - 1]:
        lo += 1
    while ask_state[hi] == ask_state[hi - 1]:
        hi += 1
    base = ask_state[lo]
    sl_states = upd[base:ask_state[hi - 1] + 1]
    with Engine(0) as e:
        res = e.diff_update_shared_batch(sl_states, [a - base for a in ask_state[lo:hi]], svs[lo:hi])
    exp = [oracle.diff_update(upd[s], sv) for s, sv in zip(ask_state[lo:hi], svs[lo:hi])]
    bad = [k for k, (g, x) in enumerate(zip(res, exp)) if g != (x if x[0] == 0 else (x[0], None))]
    assert not bad, f"default mode: {len(bad)} differ, first {bad[:5]}"


# ---------------------------------------------------------------------------------------- 5: edges
def test_edges(eng135):
    from hocuspocus_amd.engine import YjsError
    r = rows()
    three = group(r[:9])[0][:3]
    assert eng135.sync_step2_shared_batch(three, [], []) == []
    assert eng135.sync_step2_shared_batch([], [], []) == []
    assert eng135.diff_update_shared_batch([], [], []) == []
    k = next(i for i, (_, _, e) in enumerate(r) if e is not None)
    assert eng135.sync_step2_shared_batch([r[k][0]], [0], [r[k][1]]) == [(0, r[k][2])]
    calls = eng135.stats().calls
    for bad_ask in ([1, 0], [0, 3], [3], [0, 1, 0]):
        for fn in (eng135.sync_step2_shared_batch, eng135.diff_update_shared_batch):
            with pytest.raises(YjsError) as ei:
                fn(three, bad_ask, [b"\x00"] * len(bad_ask))
            assert ei.value.code == EINVAL
    assert eng135.stats().calls == calls   # refused before any device work


# ---------------------------------------------------------------------------------------- 6: one state over several chunks
def test_chunk_splitting(eng135, monkeypatch):
    monkeypatch.setenv("YGM_CHUNK_MB", "1")   # (read by the host API at each call)
    snaps = yjs_snapshots()
    uniq = group(rows())[0]
    big = max(uniq, key=len)
    small = [u for u in uniq if len(u) < 200][:20]
    assert len(big) == 14750 and len(small) == 20
    svs = storm_svs(snaps[big], 300, truncated_at=5)
    exp = [oracle.diff_update(snaps[big], sv, compat135=True, keep_sub=True) for sv in svs]
    ask_state = [0] * 300
    for s, u in enumerate(small):
        ask_state.append(1 + s)
        svs.append(b"\x00")
        exp.append(oracle.diff_update(snaps[u], b"\x00", compat135=True, keep_sub=True))
    s0 = eng135.stats()
    res = eng135.sync_step2_shared_batch([big] + small, ask_state, svs)
    s1 = eng135.stats()
    bad = [k for k, (g, e) in enumerate(zip(res, exp)) if g != e]
    assert not bad, f"{len(bad)} of {len(exp)} differ, first {bad[:5]}: got {res[bad[0]]} expected {exp[bad[0]]}"
    # about 4.4 MB of virtual bytes (300 asks x 14 750) against a 1 MB budget: the state is staged and snapshotted once
    # per chunk -- more than the 21 states, far fewer than the asks
    assert 21 < s1.docs_snapshot - s0.docs_snapshot < len(svs)

"""The kernel code around the two update-V2 fast transcoders (hocuspocus_amd/csrc/ygm_v2.hip: k_v12_fast's size tiers,
persistent loop, groups with holes, input-status loop and staging shift; k_v21f's per-wave staging decision), the
general kernels over fast-shaped inputs (YGM_V2_NOFAST / YGM_V21_NOFAST), the device-resident V2 entry points and
the V2 host API across chunk boundaries.

Every expected value is the CPU oracle's and is compared byte for byte (throws: any status of {1, 2, 4, 5} matches
any other).  Which path wrote a document shows in the device result: k_v12_fast writes document d
at align16(2 b0 + 64 d) (b0: its first V2 input byte), below slot_total = 2 arena_bytes + 64 n_docs; the general
pass packs its outputs from slot_total on.  The tests assert the exact set of documents below slot_total against a
flag fixed by construction in the corpus builders; the one CPU test pins that flag against the host build of the
fast encoder (tools/v2dev) and shows that the oracle alone gives every expected value."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from devrun import THROWS, engine_fixture, read_results, same, to_device
from lean_docs import CLIENTS, Log, item, text, upd
from v1util import vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
SV0 = b"\x00"            # the empty state vector: the diff is the whole state
F_IN = 7168              # v2f::F_IN, the large tier's cap; 3328: the small tier's
EXACT_L = [3327, 3328, 3329, 7167, 7168, 7169, 8000]


def v2(u):
    st, out = oracle.convert_update_format_v1_to_v2(u)
    assert st == 0, (st, u.hex())
    return out


# ---------------------------------------------------------------- corpus: documents with a claim flag by construction
class Doc:
    """A merge document: its V2 inputs, the V1 inputs they were converted from (None: an input is not a conversion),
    and whether k_v12_fast takes it (ASCII text log, >= 2 clean inputs, V1 result of 1..7168 bytes)."""

    def __init__(self, name, v1, claimed, v2s=None):
        self.name, self.v1, self.claimed = name, v1, claimed
        self.v2 = v2s if v2s is not None else [v2(u) for u in v1]

    @functools.cached_property
    def exp(self):
        return oracle.merge_updates_v2(self.v2)


class Ask:
    """A diff ask: a V2 state (converted from the V1 state), a state vector, and whether k_v12_fast takes it (diff:
    no input count rule -- ASCII text, V1 diff of 1..7168 bytes)."""

    def __init__(self, name, v1, sv, claimed):
        self.name, self.v1, self.sv, self.claimed = name, v1, sv, claimed
        self.v2 = v2(v1)

    @functools.cached_property
    def exp(self):
        return oracle.diff_update_v2(self.v2, self.sv)


def _exact_ups(k, m, clients, seed):
    """k one-character inserts round robin over `clients`, then one insert of m ASCII characters."""
    g = Log(clients, seed=seed)
    for i in range(k):
        g.plain(clients[i % len(clients)])
    if m:
        g.put(clients[k % len(clients)], [item(4, text("x" * m), origin=g.last)], m)
    return g.ups


def exact_log(L, clients=tuple(CLIENTS[:3]), seed=1):
    """A log whose oracle-merged V1 length is exactly L: the number of one-character updates and the length of the
    final insert are found by bisection (the merged length is monotone in both)."""
    def f(k, m):
        st, out = oracle.merge_updates(_exact_ups(k, m, clients, seed))
        assert st == 0
        return len(out)
    lo, hi = 1, 2
    assert f(lo, 1) <= L, (L, f(lo, 1))
    while f(hi, 1) <= L:
        lo, hi = hi, hi * 2
    while hi - lo > 1:          # the largest k whose log with a one-character final insert is <= L
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if f(mid, 1) <= L else (lo, mid)
    for k in range(lo, max(0, lo - 16), -1):   # (the final string's length prefix steps at 128: a few k)
        a, b = 1, L + 1
        while b - a > 1:        # the largest m with f(k, m) <= L
            mid = (a + b) // 2
            a, b = (mid, b) if f(k, mid) <= L else (a, mid)
        if f(k, a) == L:
            return _exact_ups(k, a, clients, seed)
    raise AssertionError(("no log of merged length", L))


# the empty update: two empty V2 inputs merge to the V1 bytes 00 00.  The fast encoder takes it (decided by
# test_corpus_flags_match_the_host_twin below, recorded here)
EMPTY_CLAIMED = True


@functools.lru_cache(None)
def exact_docs():
    """name -> (Doc, Ask) of the exact-length states: as merge_v2 of [the log's first half merged, the rest single],
    and as diff_v2 of the V2 state against the empty state vector (the internal V1 diff is the state, L bytes)."""
    out = {}
    for L in EXACT_L + [700, 20]:
        ups = exact_log(L) if L != 20 else exact_log(L, (5, 9, 7))
        h = (len(ups) + 1) // 2
        ins = [oracle.merge_updates(ups[:h])[1]] + ups[h:] if h > 1 else ups
        st, state = oracle.merge_updates(ins)
        assert st == 0 and len(state) == L and len(ins) >= 2, (L, len(state), len(ins))
        assert oracle.merge_updates(ups) == (0, state)
        assert oracle.diff_update(state, SV0) == (0, state)      # the V1 diff k_v12_fast sees: L bytes
        out[L] = (Doc("L%d" % L, ins, L <= F_IN), Ask("L%d" % L, state, SV0, L <= F_IN))
    e = bytes(2)
    out[0] = (Doc("empty", [e, e], EMPTY_CLAIMED), Ask("empty", e, SV0, EMPTY_CLAIMED))
    return out


def small_log(k, clients, seed, odd=None, at=None):
    """k one-character updates; update `at` is 'e' (the one character is 'é': not ASCII, one UTF-16 unit, the log stays
    contiguous) or 'type' (an Item with ContentType)."""
    g = Log(clients, seed=seed)
    for j in range(k):
        c = clients[j % len(clients)]
        if j == at and odd == "e":
            g.put(c, [item(4, text("é"), origin=g.last)], 1)
        elif j == at and odd == "type":
            g.put(c, [item(7, b"\x02", origin=g.last)], 1)
        else:
            g.plain(c)
    return g.ups


def truncated(doc_v1, i):
    v2s = [v2(u) for u in doc_v1]
    v2s[i] = v2s[i][:len(v2s[i]) // 2]
    return v2s


@functools.lru_cache(None)
def hole_docs():
    """One ineligible document of each kind."""
    t = small_log(3, CLIENTS[:2], 41)
    return [Doc("single", small_log(1, CLIENTS[:1], 40), False),                      # passthrough
            Doc("zero", [], False),                                                   # mergeUpdatesV2([])
            Doc("trunc", None, False, truncated(t, 1)),                               # a throw
            Doc("eacute", small_log(4, CLIENTS[:2], 42, "e", 2), False),              # the general path succeeds
            Doc("ctype", small_log(4, CLIENTS[:2], 43, "type", 3), False)]


@functools.lru_cache(None)
def group_batch():
    """Case 2: the exact-length sequence interleaved with the five ineligible kinds, repeated rotated by 0, 1, ...
    documents (at least 0..4) until every kind has stood at every j of a 5-group and of a 2-group, plus one document:
    n_docs is odd and no multiple of 5, the tail groups of both tiers are partial."""
    ex = exact_docs()
    E = [ex[L][0] for L in EXACT_L + [20, 0]]
    H = hole_docs()
    base = []
    for i, e in enumerate(E):
        base.append(e)
        if i < len(H):
            base.append(H[i])
    docs, r = [], 0
    while True:
        docs += base[r:] + base[:r]
        r += 1
        if r >= 5 and all({d % 5 for d, x in enumerate(docs) if x is h} == set(range(5)) and
                          {d % 2 for d, x in enumerate(docs) if x is h} == {0, 1} for h in H):
            break
        assert r < len(base)
    docs.append(pool()[0])
    while len(docs) % 5 == 0 or len(docs) % 2 == 0:
        docs.append(pool()[len(docs) % 97])
    return docs


@functools.lru_cache(None)
def pool():
    """97 distinct tiny text logs of two and three updates, one to three clients."""
    return [Doc("p%d" % i, small_log(2 + i % 2, CLIENTS[i % 5:i % 5 + 1 + i % 3], 100 + i), True) for i in range(97)]


REUSE_CYCLES = {6: [3328, 20, 700, 7168, 20, 3329],            # period coprime to 5: every slot of the small tier
                7: [7168, 20, 3329, 7167, 700, 3328, 20]}      # ... and to 2: both slots of the large tier


STRIDE_K = [2, 3, 63, 64, 65, 66, 128, 129, 130]


@functools.lru_cache(None)
def stride_docs():
    """Case 5: logs of k V2 updates, clean, and with update i a truncated one (a throw) or the 'é' one (status OK,
    the general path)."""
    docs = []
    for k in STRIDE_K:
        docs.append(Doc("k%d" % k, small_log(k, CLIENTS[:3], k), True))
        for i in sorted({0, 63, 64, k - 1}):
            if i < k:
                docs.append(Doc("k%d_t%d" % (k, i), None, False, truncated(small_log(k, CLIENTS[:3], k), i)))
                docs.append(Doc("k%d_e%d" % (k, i), small_log(k, CLIENTS[:3], k, "e", i), False))
    return docs


N_DEFER_SV = 17   # state-vector entries: one past the walker's table (DW_SVN = 16), the ask goes to the exact kernel


@functools.lru_cache(None)
def defer_asks():
    """Case 7: the pool's merged states asked for with a state vector of half of each client's clock; two of three
    asks carry unknown clients up to 17 entries, which the diff walker leaves to the exact kernel."""
    asks = []
    for i, p in enumerate(pool()):
        st, state = oracle.merge_updates(p.v1)
        clients = CLIENTS[i % 5:i % 5 + 1 + i % 3]
        n = len(p.v1)
        ent = [(c, len(range(j, n, len(clients))) // 2) for j, c in enumerate(clients)]
        deferred = i % 3 != 0
        if deferred:
            ent += [(1000 + j, 0) for j in range(N_DEFER_SV - len(ent))]
        sv = vu(len(ent)) + b"".join(vu(c) + vu(k) for c, k in ent)
        a = Ask("ask%d" % i, state, sv, True)
        a.deferred = deferred
        asks.append(a)
    return asks


# ---------------------------------------------------------------- the host twin pins the flags (no GPU)
@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """hv_v12f of tools/v2dev: (0, V2 bytes) where the fast encoder takes the V1 update, else (1 | 2, None)."""
    so = str(tmp_path_factory.mktemp("v2dev") / "libv2dev.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "v2dev", "v2dev.cpp")],
                   check=True, timeout=600)
    L = ctypes.CDLL(so)
    L.hv_v12f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]

    def run(v1):
        out = ctypes.create_string_buffer(8192)
        ln = ctypes.c_uint64()
        e = L.hv_v12f(v1, len(v1), out, ctypes.byref(ln))
        return e, out.raw[:ln.value] if e == 0 else None
    return run


def all_docs():
    ex = exact_docs()
    return [d for d, _ in ex.values()] + hole_docs() + pool() + stride_docs() + group_batch()


def all_asks():
    return [a for _, a in exact_docs().values()] + defer_asks()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ for the host build of the fast encoder")
def test_corpus_flags_match_the_host_twin(twin):
    """Every corpus document: the host build of k_v12_fast's per-lane code takes the oracle's V1 result exactly where
    the builder's flag says claimed, and its bytes are the oracle's V1 -> V2 conversion of that result -- which is
    also what the oracle's V2 operation gives, so the oracle alone supplies every expected value."""
    n = {True: 0, False: 0}
    for d in {id(x): x for x in all_docs()}.values():
        if d.v1 is None or len(d.v2) < 2:          # a truncated input / a passthrough / no input: never eligible
            assert not d.claimed, d.name
            if d.v1 is None:
                assert d.exp[0] in THROWS, (d.name, d.exp[0])
            n[False] += 1
            continue
        st, v1 = oracle.merge_updates(d.v1)
        assert st == 0, d.name
        assert d.exp == (0, v2(v1)), d.name
        e, out = twin(v1)
        assert (e == 0) == d.claimed, (d.name, e, len(v1))
        if e == 0:
            assert out == d.exp[1], d.name
        n[d.claimed] += 1
    for a in all_asks():
        st, v1 = oracle.diff_update(a.v1, a.sv)
        assert st == 0, a.name
        assert a.exp == (0, v2(v1)), a.name
        e, out = twin(v1)
        assert (e == 0) == a.claimed, (a.name, e, len(v1))
        if e == 0:
            assert out == a.exp[1], a.name
        n[a.claimed] += 1
    ex = exact_docs()
    assert [ex[L][0].claimed for L in EXACT_L] == [True] * 5 + [False] * 2
    assert min(n.values()) > 40, n


# ---------------------------------------------------------------- device runs
eng = engine_fixture()


def _fetch(r, n):
    res, off, ln = read_results(r, n, places=True)
    return res, off, ln, int(r.payload_bytes)


def _arena(blobs):
    a = np.frombuffer(b"".join(blobs) + bytes(64), np.uint8)
    off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    return a, off


def run_merge(eng, docs):
    """docs (lists of V2 updates) through Engine.merge_v2_device: results, offsets, lengths, payload bytes, every
    document's first input byte, arena bytes."""
    blobs = [u for us in docs for u in us]
    a, off = _arena(blobs)
    du = np.cumsum([0] + [len(us) for us in docs]).astype(np.uint32)
    ta, to, td = to_device(a, off.view(np.int64), du.view(np.int32))
    r = eng.merge_v2_device(ta, len(a) - 64, to, td, len(blobs), len(docs))
    return _fetch(r, len(docs)) + ([int(x) for x in off[du[:-1]]], len(a) - 64)


def run_doc(eng, op, updates, svs=None):
    """updates through Engine.doc_v2_device ('diff' with svs, 'sv')."""
    a, off = _arena(updates)
    ta, to = to_device(a, off.view(np.int64))
    if op == "diff":
        s, soff = _arena(svs)
        ts, tso = to_device(s, soff.view(np.int64))
        r = eng.doc_v2_device("diff", ta, len(a) - 64, to, len(updates), ts, tso)
    else:
        r = eng.doc_v2_device(op, ta, len(a) - 64, to, len(updates))
    return _fetch(r, len(updates)) + ([int(x) for x in off[:-1]], len(a) - 64)


def check(items, run, nofast=False):
    """items (Doc / Ask) against a run's output: bytes and statuses as the oracle's, and the documents written by
    k_v12_fast -- at their slots, below slot_total -- exactly the flagged ones.  nofast (YGM_V2_NOFAST: there is no
    slot region, the general pass packs from 0): every output at the exclusive scan of the lengths before it.
    -> (claimed, not claimed)."""
    res, off, ln, payload, b0, arena_bytes = run
    n = len(items)
    bad = [d for d in range(n) if not same(items[d].exp, res[d])]
    assert not bad, (len(bad), [(d, items[d].name, items[d].exp[0], res[d][0]) for d in bad[:5]])
    assert payload == sum(ln), (payload, sum(ln))      # (a document counted by both launches would show here)
    if nofast:
        at = 0
        for d in range(n):
            assert off[d] == at, (d, items[d].name, off[d], at)
            at += ln[d]
        return 0, n
    slot_total = 2 * arena_bytes + 64 * n
    got = [off[d] < slot_total for d in range(n)]
    want = [bool(x.claimed) for x in items]
    wrong = [(d, items[d].name, got[d]) for d in range(n) if got[d] != want[d]]
    assert not wrong, (len(wrong), wrong[:8])
    for d in range(n):
        if got[d]:
            assert off[d] == (2 * b0[d] + 64 * d + 15) & ~15, (d, items[d].name)
    return sum(want), n - sum(want)


def merge_check(eng, docs, nofast=False):
    return check(docs, run_merge(eng, [d.v2 for d in docs]), nofast)


def diff_check(eng, asks, nofast=False):
    return check(asks, run_doc(eng, "diff", [a.v2 for a in asks], [a.sv for a in asks]), nofast)


# ---- 1: the size tiers, at their caps
@gpu
@pytest.mark.parametrize("form", ["diff", "merge"])
def test_exact_lengths_at_the_tier_caps(eng, form):
    """V1 results of exactly 3327 / 3328 / 3329 (the small tier's cap), 7167 / 7168 / 7169 (F_IN), 8000, 20 and 2
    bytes: up to 7168 claimed (7 documents), past it the general pass (2)."""
    ex = exact_docs()
    items = [ex[L][form == "diff"] for L in EXACT_L + [20, 0]]
    took = (diff_check if form == "diff" else merge_check)(eng, items)
    assert took == (7, 2)


# ---- 2: every kind of hole at every group position
@gpu
@pytest.mark.parametrize("grid", [None, 1, 3])
def test_holes_at_every_group_position(eng, monkeypatch, grid):
    """The exact-length documents with a passthrough, an empty merge, a throw, a non-ASCII log and a ContentType log
    between them, rotated so each stands at every position of a group of five and of two; the default grid, and one
    and three waves for all groups (YGM_V12F_GRID).  99 documents (seven rotations): 50 claimed, 49 not."""
    if grid:
        monkeypatch.setenv("YGM_V12F_GRID", str(grid))
    docs = group_batch()
    assert len(docs) % 5 and len(docs) % 2
    assert merge_check(eng, docs) == (50, 49)


# ---- 3: LDS slots and column scratch reused, a large document before a small one
@gpu
@pytest.mark.parametrize("form", ["diff", "merge"])
@pytest.mark.parametrize("period", [6, 7])
def test_slot_and_scratch_reuse(monkeypatch, form, period):
    """One wave takes every group (YGM_V12F_GRID=1): a slot that held 3328 / 7168 bytes next holds 20, over >= 9 rounds;
    then the same batch on the same engine with the default grid (the grow-only scratch keeps the first call's
    bytes).  All 60 / 63 documents claimed, both times.  (Stale bytes past a document's end cannot change an output:
    every read of the fast encoder that reaches byte n or later clears `ok` whatever it finds there -- f_vat's
    e < r.n -- so this checks the reuse of slots and scratch, not the zero fill.)"""
    from hocuspocus_amd import Engine
    ex = exact_docs()
    cyc = REUSE_CYCLES[period]
    items = [ex[cyc[d % period]][form == "diff"] for d in range(60 if period == 6 else 63)]
    run = diff_check if form == "diff" else merge_check
    with Engine(0) as e:
        monkeypatch.setenv("YGM_V12F_GRID", "1")
        assert run(e, items) == (len(items), 0)
        monkeypatch.delenv("YGM_V12F_GRID")
        assert run(e, items) == (len(items), 0)


# ---- 4: more documents than the resident grid
@gpu
def test_more_documents_than_the_default_grid(eng):
    """12 000 two- and three-update documents in one call, all claimed.  Observed on the MI355X (256 CUs): the small
    tier's grid is 2048 waves (eight per CU, as the sizing comment in ygm_v2.hip says; read back from the scratch size,
    2048 x 5 x 9 x 3392 bytes), so 10 240 documents are resident and 352 waves take a second group."""
    P = pool()
    docs = [P[d % 97] for d in range(12000)]
    assert merge_check(eng, docs) == (12000, 0)


# ---- 5: the input-status loop past its first stride
@gpu
def test_status_loop_strides(eng):
    """Logs of 2 .. 130 V2 updates, clean (9 documents, claimed) and with a truncated or a non-ASCII update at index
    0, 63, 64 and the last (54 documents, not claimed): status and bytes as the oracle's.  (The loop is a second
    guard: an input that did not transcode has a V1 length of 0, the V1 merge of a document with an empty input
    throws, and v1_st[d] turns the document away too -- a kernel with the stride removed still passes this test.)"""
    docs = stride_docs()
    assert merge_check(eng, docs) == (len(STRIDE_K), 54)


# ---- 6: k_v21f's staging decision (byte parity only: nothing outside shows which kernel took an update)
def _sized(g, c, size):
    """Appends to g an ASCII insert by client c whose V2 form is exactly `size` bytes (length found by bisection)."""
    def n(m):
        return len(v2(upd(c, g.clock[c], [item(4, text("q" * m), origin=g.last)])))
    a, b = 1, size
    while b - a > 1:
        mid = (a + b) // 2
        a, b = (mid, b) if n(mid) <= size else (a, mid)
    assert n(a) == size, (size, n(a))
    g.put(c, [item(4, text("q" * a), origin=g.last)], a)


def _padded(seed, at, pad):
    """64 updates: one-character inserts and, at index `at`, one insert of `pad` characters."""
    g = Log(CLIENTS[:2], seed=seed)
    for j in range(64):
        c = CLIENTS[j % 2]
        if j == at:
            g.put(c, [item(4, text("p" * pad), origin=g.last)], pad)
        else:
            g.plain(c)
    return [v2(u) for u in g.ups]


def _lens(docs):
    return [len(u) for us in docs for u in us]


@functools.lru_cache(None)
def v21_batch(x):
    """The V2 inputs of one staging batch; x more characters in the very first update move every later update.
      wave 0      a 70-update log: its first 64 updates, with one of exactly 128 and one of 129 V2 bytes (F21_MAX)
      wave 1      its last six, then documents of 1, 2, 1 and 54 updates
      wave 2 / 3  64 updates spanning exactly 8192 / 8193 bytes from the wave's 16-byte aligned base
      wave 4      one 8 KB update among one-character ones
      wave 5, 6   a log of 65 (x even) or 127 (x odd) updates: the last wave holds 1 or 63"""
    g = Log(CLIENTS[:3], seed=7)
    g.put(CLIENTS[0], [item(4, text("a" * (1 + x)))], 1 + x)
    for j in range(1, 70):
        c = CLIENTS[j % 3]
        if j in (10, 11):
            _sized(g, c, 118 + j)
        else:
            g.plain(c)
    docs = [[v2(u) for u in g.ups]]
    assert [len(docs[0][j]) for j in (10, 11)] == [128, 129]
    for k, seed in ((1, 50), (2, 51), (1, 52), (54, 53)):
        docs.append([v2(u) for u in small_log(k, CLIENTS[1:3], seed)])
    for want in (8192, 8193):
        u0 = len(_lens(docs))
        assert u0 % 64 == 0
        a0 = sum(_lens(docs))
        pad = 6000
        for _ in range(6):
            w = _padded(60 + want % 2, 30, pad)
            span = (a0 & 15) + sum(len(u) for u in w)
            if span == want:
                break
            pad += want - span
        assert span == want, (want, span)
        docs.append(w)
    docs.append(_padded(62, 5, 8300))
    assert max(len(u) for u in docs[-1]) > 8192
    docs.append([v2(u) for u in small_log(65 if x % 2 == 0 else 127, CLIENTS[:3], 63)])
    n = len(_lens(docs))
    assert n % 64 == (1 if x % 2 == 0 else 63), n
    return docs, sum(_lens(docs)[:64]) % 16


@functools.lru_cache(None)
def v21_batches():
    """One batch per residue of update 64's arena offset mod 16, both last-wave sizes among them."""
    by_r = {}
    for x in range(64):
        docs, r = v21_batch(x)
        by_r.setdefault(r, docs)
        if len(by_r) == 16:
            break
    assert sorted(by_r) == list(range(16))
    assert {len(_lens(d)) % 64 for d in by_r.values()} == {1, 63}
    return by_r


_MERGE_EXP = {}


def _merge_exp(us):
    k = tuple(us)
    if k not in _MERGE_EXP:
        _MERGE_EXP[k] = oracle.merge_updates_v2(us)
    return _MERGE_EXP[k]


@gpu
def test_v21f_staging_residues_and_edges(eng, monkeypatch):
    """Sixteen merge batches, update 64 at every residue mod 16, each with the 128 / 129-byte updates, the 8192 /
    8193-byte waves, the 8 KB update, the passthrough units inside waves and a last wave of 1 or 63: the oracle's bytes,
    by default and with the general transcoder alone (YGM_V21_NOFAST)."""
    for r, docs in sorted(v21_batches().items()):
        exp = [_merge_exp(us) for us in docs]
        got = run_merge(eng, docs)[0]
        monkeypatch.setenv("YGM_V21_NOFAST", "1")
        slow = run_merge(eng, docs)[0]
        monkeypatch.delenv("YGM_V21_NOFAST")
        for d in range(len(docs)):
            assert same(exp[d], got[d]), (r, d)
            assert same(exp[d], slow[d]), (r, d, "general")
        assert got == slow, r


@gpu
@pytest.mark.parametrize("op", ["sv", "diff"])
def test_v21f_one_lane_per_document(eng, monkeypatch, op):
    """The updates of up to 129 V2 bytes of a staging batch as documents of their own through doc_v2_device: the
    state vector (structs only) and the diff against the empty state vector, by default and under YGM_V21_NOFAST."""
    ups = sorted({u for us in v21_batches()[0] for u in us if len(u) <= 129}, key=lambda u: (len(u), u))
    assert {128, 129} <= {len(u) for u in ups}
    if op == "sv":
        exp = [oracle.encode_state_vector_from_update_v2(u) for u in ups]
    else:
        exp = [oracle.diff_update_v2(u, SV0) for u in ups]
    svs = [SV0] * len(ups)
    got = run_doc(eng, op, ups, svs)[0]
    monkeypatch.setenv("YGM_V21_NOFAST", "1")
    slow = run_doc(eng, op, ups, svs)[0]
    for d in range(len(ups)):
        assert same(exp[d], got[d]), (d, ups[d].hex())
    assert got == slow


# ---- 7: V1 inputs to the fast encoder that the exact diff kernel packed
@gpu
def test_deferred_asks_reach_the_fast_encoder(eng):
    """97 diff asks, 64 of them with a 17-entry state vector.  The walker's table holds 16 (k_sv_table), so those go to
    the exact kernel: the docs_fast counter rises by exactly 64.  That kernel (doc_exact in ygm_kernels.hip) places
    its outputs at out_base + the exclusive scan of their byte lengths, with no rounding, so from the second deferred
    ask on the V1 bytes k_v12_fast stages start at any offset mod 16 (sh = a & 15 is not 0); the walker's own outputs
    sit in 16-byte aligned slots.  All 97 claimed."""
    asks = defer_asks()
    n_def = sum(a.deferred for a in asks)
    assert n_def == 64
    before = eng.stats().docs_fast
    assert diff_check(eng, asks) == (97, 0)
    assert eng.stats().docs_fast - before == n_def


# ---- 8: the general kernels over the fast shapes
@gpu
def test_general_kernels_over_fast_shapes(eng, monkeypatch):
    """The exact-length batches and the status-stride batch with YGM_V2_NOFAST=1: the oracle's bytes, and nothing in a
    slot -- without the fast encoder there is no slot region (slot_total is 0 inside the engine), so every document
    sits at the exclusive scan of the output lengths before it."""
    monkeypatch.setenv("YGM_V2_NOFAST", "1")
    ex = exact_docs()
    assert merge_check(eng, [ex[L][0] for L in EXACT_L + [20, 0]], nofast=True) == (0, 9)
    assert diff_check(eng, [ex[L][1] for L in EXACT_L + [20, 0]], nofast=True) == (0, 9)
    assert merge_check(eng, stride_docs(), nofast=True) == (0, 63)


# ---- 9: the V2 host API across chunk boundaries
@gpu
def test_host_api_chunks(eng, monkeypatch):
    """About 3 MB of V2 inputs through merge_updates_v2_batch and diff_update_v2_batch in 1 MB chunks (YGM_CHUNK_MB):
    results in document order, equal to the single-chunk call and to the oracle."""
    base = group_batch()
    per = sum(len(u) for d in base for u in d.v2)
    docs = [base[d % len(base)] for d in range(len(base) * (3 * 2 ** 20 // per + 1))]
    ex = exact_docs()
    abase = [ex[L][1] for L in EXACT_L + [700, 20, 0]] + defer_asks()
    aper = sum(len(a.v2) for a in abase)
    asks = [abase[d % len(abase)] for d in range(len(abase) * (3 * 2 ** 20 // aper + 1))]
    one_m = eng.merge_updates_v2_batch([d.v2 for d in docs])
    one_d = eng.diff_update_v2_batch([a.v2 for a in asks], [a.sv for a in asks])
    monkeypatch.setenv("YGM_CHUNK_MB", "1")
    cut_m = eng.merge_updates_v2_batch([d.v2 for d in docs])
    cut_d = eng.diff_update_v2_batch([a.v2 for a in asks], [a.sv for a in asks])
    assert cut_m == one_m and cut_d == one_d
    assert len(cut_m) == len(docs) and len(cut_d) == len(asks)
    for d, x in enumerate(docs):
        assert same(x.exp, cut_m[d]), (d, x.name)
    for d, x in enumerate(asks):
        assert same(x.exp, cut_d[d]), (d, x.name)

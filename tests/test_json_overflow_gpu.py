"""k_json's second launch on the GPU (ygm_json_v1 / ygm_json_v1_device): the documents whose JSON outgrows their
workspace's output region, listed through the launch's atomics and run again into claimed regions after the workspaces.

The documents are tests/json_overflow_docs.py's: their JSON and their distance from the cap (delta) are known by
construction and pinned against yjs and the host twin in tests/test_json_overflow_docs.py.  Here: the exact boundary
(delta 0 fits, +1 runs again) with the claimed regions' geometry; 1 to 65 listed documents over one to five blocks of
the second launch, at 1, 16 and 64 documents per wave; refusals, an empty and a truncated state between listed
documents; the buffer's regrowth with the fitting documents' outputs carried over; an overflow call between plain
calls on one context; listed documents in two chunks of a host batch; unaligned, unstaged and staged documents under
root names of 1, 7 and 130 bytes; the yjs-made boundary sessions.  Every comparison is exact."""
import collections
import re

import pytest

import json_fixture as jf
import json_overflow_docs as g
from devrun import engine_fixture, read_results, upload

pytestmark = pytest.mark.gpu

JSON_LINE = re.compile(r"^ygm json tiers: docs (\d+) general (\d+) overflow (\d+) overflow_bytes (\d+)$", re.M)
KNOBS = ("YGM_SNAP_NOLDS", "YGM_SNAP_DPW", "YGM_CHUNK_MB")
STAGE = 40960        # docstage::STAGE
APIS = ("batch", "device")

# res: [(status, bytes)]; lines: the call's tier lines; off, len, data_bytes: the device form's places (None: host form)
Out = collections.namedtuple("Out", "res lines off len data_bytes")


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


eng = engine_fixture(compat135=True)


def call(eng, capfd, states, names, api, lead=0):
    """One call over (state, root name) pairs; the device form's first state starts `lead` bytes into its arena.  What
    every test asserts is asserted here: the internal status 65 never comes out, a refused document has no bytes, and
    the payload (the call's bytes_out, and the device result's payload_bytes) is the sum of the status-0 lengths."""
    n = len(states)
    out0 = eng.stats().bytes_out
    capfd.readouterr()
    if api == "batch":
        res = [(0, r) if isinstance(r, bytes) else (r.code, b"") for r in eng.json_batch(states, names)]
        offs = lens = data_bytes = None
    else:
        ta, to, nbytes = upload(states, lead=lead)
        tn, tno, _ = upload(names)
        assert ta.data_ptr() % 16 == 0
        r = eng.json_device(ta, nbytes, to, tn, tno, n)
        res, offs, lens = read_results(r, n, every=True, places=True)
        data_bytes = int(r.data_bytes)
        assert all(offs[d] + lens[d] <= data_bytes for d in range(n))
        assert lens == [len(b) for _, b in res]
        assert int(r.payload_bytes) == sum(len(b) for st, b in res if st == 0)
    lines = [dict(zip(("docs", "general", "overflow", "overflow_bytes"), map(int, ln))) for ln in JSON_LINE.findall(capfd.readouterr().err)]
    assert jf.ST_MORE not in {st for st, _ in res}
    assert all(st == 0 or b == b"" for st, b in res)
    assert eng.stats().bytes_out - out0 == sum(len(b) for st, b in res if st == 0)
    assert sum(ln["docs"] for ln in lines) == n
    return Out(res, lines, offs, lens, data_bytes)


def run(eng, capfd, docs, api, lead=0):
    """call() over Docs, compared with their expectation; the tier lines count exactly the documents that must rerun
    and the claimed bytes are the sum of their 16-aligned lengths."""
    o = call(eng, capfd, [d.u for d in docs], [d.ask for d in docs], api, lead)
    bad = [k for k, d in enumerate(docs) if o.res[k] != (d.status, d.json)]
    assert not bad, (api, len(bad), [(docs[k].name, docs[k].status, o.res[k][0], len(docs[k].json), len(o.res[k][1])) for k in bad[:4]])
    assert sum(ln["overflow"] for ln in o.lines) == sum(d.rerun for d in docs)
    assert sum(ln["overflow_bytes"] for ln in o.lines) == sum(g.al16(len(d.json)) for d in docs if d.rerun)
    return o


def geometry(docs, o):
    """The device form's places: fitting and refused documents in the workspaces, rerun documents in 16-aligned,
    pairwise disjoint regions after them, inside the result's extent.  (The atomics do not fix the regions' order.)"""
    assert len(o.lines) == 1
    b_total = o.data_bytes - o.lines[0]["overflow_bytes"]
    assert b_total > 0
    regions = []
    for k, d in enumerate(docs):
        if d.rerun:
            assert o.off[k] >= b_total and o.off[k] % 16 == 0 and o.off[k] + g.al16(o.len[k]) <= o.data_bytes, d.name
            regions.append((o.off[k], o.off[k] + o.len[k]))
        else:
            assert o.off[k] + o.len[k] <= b_total, d.name
    regions.sort()
    assert all(a[1] <= b[0] for a, b in zip(regions, regions[1:]))
    return b_total


def interleave(over, salt=0):
    """Overflow documents between fitting ones, one or two at a time, so that a document's place on the list is not
    its index: fit, o, fit, o, o, fit, o, fit, o, o, ..."""
    out = []
    for i, d in enumerate(over):
        if i % 3 != 2:
            out.append(g.fit((i + salt) % 4))
        out.append(d)
    return out


@pytest.mark.parametrize("api", APIS)
def test_boundary(eng, capfd, api):
    docs = g.sweep()
    assert [d.delta for d in docs] == list(range(-4, 20))
    o = run(eng, capfd, docs, api)
    assert [ln["overflow"] for ln in o.lines] == [19]
    assert o.lines[0]["overflow_bytes"] == sum(g.al16(len(d.json)) for d in docs if d.delta > 0)
    if api == "device":
        geometry(docs, o)


@pytest.mark.parametrize("dpw,n", [(None, 1), (None, 16), (None, 17), (None, 33), ("1", 5), ("64", 65)])
def test_rerun_grid(eng, capfd, monkeypatch, dpw, n):
    if dpw:
        monkeypatch.setenv("YGM_SNAP_DPW", dpw)
    docs = interleave(g.grid(n))
    assert sum(d.rerun for d in docs) == n and docs[1].rerun and not docs[0].rerun
    for api in APIS:
        o = run(eng, capfd, docs, api)
        assert [ln["overflow"] for ln in o.lines] == [n]
        if api == "device":
            geometry(docs, o)


def test_mixed_lanes(eng, capfd):
    from hocuspocus_amd.engine import EMALFORMED
    grid = g.grid(8)
    cut = grid[3].u[:-3]
    snap = eng.snapshot_batch([cut])[0][0]
    assert snap != 0
    refused9, refused3 = g.late_refusals()
    docs = [g.fit(0), grid[0], refused9, refused3, g.Doc("an empty document", b"", g.ROOT, EMALFORMED, b"", False, 0), g.no_tail(),
            g.Doc("a truncated state", cut, g.ROOT, snap, b"", False, 0), g.absent_ask(), g.fit(1), grid[1], grid[2], refused3, g.fit(2),
            grid[4], refused9, g.fit(3),
            grid[5], g.absent_ask(), refused9, grid[6], g.fit(0), grid[7]]      # (a partial second wave, an overflow document last)
    assert 16 < len(docs) < 32 and docs[-1].rerun and grid[0].delta == 326 and len(g.no_tail().json) == 13934
    n = sum(d.rerun for d in docs)
    assert n == 8
    for api in APIS:
        o = run(eng, capfd, docs, api)
        assert [ln["overflow"] for ln in o.lines] == [n]
        assert [st for st, _ in o.res] == [0, 0, 9, 3, EMALFORMED, 0, snap, 0, 0, 0, 0, 3, 0, 0, 9, 0, 0, 0, 9, 0, 0, 0]
        if api == "device":
            geometry(docs, o)


def test_regrowth(eng, capfd):
    """A fresh context per form: its buffer is sized by the first call's workspaces (capacity 1.25 (B_total + 64)), so
    an overflow region of more than a quarter of that moves the buffer -- with the fitting documents' outputs in it.
    The same batch again finds the buffer large enough, and nothing moves.  The host form sizes the same workspaces
    (the count pass sees the same documents), so the device form's precondition is the host form's too."""
    from hocuspocus_amd import Engine
    fits = [g.fit(0), g.fit(1), g.fit(2)]
    docs = [fits[0], g.big(0), fits[1], g.big(1), fits[2]]
    lines = None
    for api in ("device", "batch"):
        alone = run(eng, capfd, fits, api)      # (a batch without the big ones, on another context)
        e = Engine(0, compat135=True)
        try:
            first = run(e, capfd, docs, api)
            again = run(e, capfd, docs, api)
        finally:
            e.close()
        assert [ln["overflow"] for ln in first.lines] == [2]
        ovf = first.lines[0]["overflow_bytes"]
        assert ovf == g.al16(len(docs[1].json)) + g.al16(len(docs[3].json))
        if api == "device":
            b_total = geometry(docs, first)
            assert ovf > (b_total + 64) / 4, (ovf, b_total)      # the precondition: the buffer had to move
            assert geometry(docs, again) == b_total
            lines = first.lines
        assert first.lines == lines
        assert [first.res[k] for k in (0, 2, 4)] == alone.res
        assert again.res == first.res and again.lines == first.lines


@pytest.mark.parametrize("api", APIS)
def test_call_after_call(eng, capfd, api):
    for n in (1, 17):
        over = interleave(g.grid(n))
        plain = [g.fit(k % 4) if d.rerun else d for k, d in enumerate(over)]
        assert len(plain) == len(over) and not any(d.rerun for d in plain)
        s0 = eng.stats().host_syncs
        p0 = run(eng, capfd, plain, api)
        s1 = eng.stats().host_syncs
        a = run(eng, capfd, over, api)
        s2 = eng.stats().host_syncs
        p1 = run(eng, capfd, plain, api)
        s3 = eng.stats().host_syncs
        b = run(eng, capfd, over, api)
        assert [[ln["overflow"] for ln in o.lines] for o in (p0, a, p1, b)] == [[0], [n], [0], [n]]
        assert [[ln["overflow_bytes"] for ln in o.lines] for o in (p0, p1)] == [[0], [0]]
        assert a.res == b.res and p0.res == p1.res
        assert (s2 - s1) - (s1 - s0) == 1 and s3 - s2 == s1 - s0, (s0, s1, s2, s3)
        if api == "device":
            assert p1.data_bytes == p0.data_bytes and geometry(over, a) == geometry(over, b)


def test_chunks(eng, capfd, monkeypatch):
    grid = g.grid(5)
    fill = [g.filler(48000 + k, k) for k in range(46)]
    docs = grid[:2] + fill + grid[2:]
    assert sum(len(d.u) for d in fill) > (2 << 20) and all(len(d.u) < (1 << 20) for d in docs)
    one = run(eng, capfd, docs, "batch")
    assert [ln["overflow"] for ln in one.lines] == [5]
    monkeypatch.setenv("YGM_CHUNK_MB", "1")
    many = run(eng, capfd, docs, "batch")
    assert len(many.lines) >= 3
    assert sum(ln["overflow"] > 0 for ln in many.lines) >= 2      # listed documents in more than one chunk
    assert sum(ln["overflow"] for ln in many.lines) == one.lines[0]["overflow"]
    assert sum(ln["overflow_bytes"] for ln in many.lines) == one.lines[0]["overflow_bytes"]
    assert many.res == one.res


@pytest.mark.parametrize("lead", [1, 15, 16])
def test_placement(eng, capfd, lead):
    """The device form with the first state `lead` bytes into the arena and per-document root names of 1, 7 and 130
    bytes: the second launch reads states and names where they lie (arena + off, names + off), whatever the first run
    did -- wave 0 staged in LDS, or pushed over the staged bytes by a filler and read from memory."""
    named = g.named_roots()
    assert [len(d.ask) for d in named] == [1] * 4 + [7] * 4 + [130] * 4 and sum(d.rerun for d in named) == 9
    tail = [g.grid(4, b"n" * 130)[3], g.fit(2, b"r"), g.grid(5)[4]]
    results = {}
    for size in (2000, 40000):
        docs = named[:7] + [g.filler(size, 1, b"q" * 9)] + named[7:] + [g.fit(3), g.no_tail(), g.absent_ask()] + tail
        assert len(docs) == 19
        extent = lead % 16 + sum(len(d.u) for d in docs[:16])
        assert (extent <= STAGE) == (size == 2000)      # 2000: wave 0 is staged; 40000: its first run reads memory
        o = run(eng, capfd, docs, "device", lead)
        assert [ln["overflow"] for ln in o.lines] == [9 + 1 + 2]
        geometry(docs, o)
        results[size] = [r for k, r in enumerate(o.res) if k != 7]
    assert results[2000] == results[40000]


@pytest.mark.parametrize("compat", [True, False])
def test_boundary_sessions(capfd, compat):
    from hocuspocus_amd import Engine
    rows = g.session_rows()
    assert len(rows) == 52 and {r[3] for r in rows} == {0, 3, 9}
    e = Engine(0, compat135=compat)
    try:
        for api in APIS:
            o = call(e, capfd, [r[1] for r in rows], [r[2] for r in rows], api)
            bad = [(r[0], r[2], r[3], x[0], x[1][:60]) for r, x in zip(rows, o.res) if not jf.matches(r, *x)]
            assert not bad, (api, compat, len(bad), bad[:4])
            assert [ln["overflow"] for ln in o.lines] == [0]
    finally:
        e.close()

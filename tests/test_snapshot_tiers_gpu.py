"""The snapshot cascade on the GPU (snapshot_dev: k_snap_text with 6 KiB, then 24 KiB of LDS, then k_snap_count / scan /
k_snap, then the pending merge) on the corpus of snapshot_tier_docs.py: every document bit-exact against yjs
(tests/golden/snapshot_tier_edges_v135.json.gz) through the host and the device form, in both delete-set orders, and --
by the call's tier line (YGM_TIER_COUNTS) -- finished by the tier its label names.  A cap that drifts, or a kernel that
takes a document one part over its cap, moves a count even where the bytes still come out right.

Then what only the GPU has: the input's dword shift and the read window past a document's end (every arena residue,
two tail paddings), the staging copy at its limit, documents per wave, the scanned workspace offsets across block
edges, the pending list, and the claim / slot / workspace buffers reused from call to call."""
import re
import time

import numpy as np
import pytest

import snapshot_tier_docs as g
from devrun import engine_fixture, read_results, same, to_device, upload
from snapshot_tier_docs import expected

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^ygm snapshot tiers: docs (\d+) text_first (\d+) text_second (\d+) general (\d+) pending (\d+)$", re.M)
KNOBS = ("YGM_SNAP_NOLDS", "YGM_SNAP_TEXT", "YGM_SNAP_DPW", "YGM_CHUNK_MB")
NOTES = []      # every call's counts, printed when the test ends (the tests read the captured stderr between calls)


@pytest.fixture(autouse=True)
def tier_counts(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    del NOTES[:]
    yield
    print("\n".join(NOTES))


def _engine(compat135):
    from hocuspocus_amd import Engine
    return Engine(0, compat135=compat135)


eng135 = engine_fixture(compat135=True)
eng136 = engine_fixture(compat135=False)


def device_snapshot(eng, us, opts=None, tail=0x00):
    """ygm_snapshot_(opts_)v1_device over an arena from torch (its base 16-aligned), the 64 bytes after it set to `tail`
    -> (status, bytes | None) per document."""
    ta, to, nbytes = upload(us, tail=tail)
    assert ta.data_ptr() % 16 == 0
    topt = to_device(np.asarray(opts, np.uint8))[0] if opts is not None else 0
    r = eng.snapshot_device(ta, nbytes, to, len(us), d_doc_opt=topt)
    return read_results(r, len(us))


def run_counted(eng, capfd, docs, api="batch", opts=None, tail=0x00):
    """One call: results, its tier line as a dict, and what docs_pending / docs_snapshot rose by."""
    capfd.readouterr()
    s = eng.stats()
    before = (s.docs_pending, s.docs_snapshot)
    us = [d.u for d in docs]
    res = eng.snapshot_batch(us, opts) if api == "batch" else device_snapshot(eng, us, opts, tail)
    s = eng.stats()
    lines = LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1, lines
    c = dict(zip(("docs", "text_first", "text_second", "general", "pending"), map(int, lines[0])))
    c["docs_pending"], c["docs_snapshot"] = s.docs_pending - before[0], s.docs_snapshot - before[1]
    return res, c


def parity(docs, res, compat, what, opts=None):
    assert len(res) == len(docs)
    bad = []
    for k, d in enumerate(docs):
        exp = expected(d, compat, bool(opts and opts[k]))
        if not same(exp, (res[k][0], res[k][1] if res[k][1] is not None else b"")):
            bad.append(k)
    assert not bad, (what, len(bad), [(k, docs[k].name, res[k][0]) for k in bad[:6]])


def tier_check(docs, c, what, lds=True, first_cap=g.CAP_FIRST):
    """The call's line against the labels: pending documents count in `general` (k_snap ran them) and in `pending`."""
    tiers = [g.tier_at(d, first_cap) if d.parts is not None else d.tier for d in docs]
    first = tiers.count("first") if lds else 0
    second = tiers.count("second") if lds else 0
    pending = tiers.count("pending")
    NOTES.append("%s %s" % (what, c))
    assert c == dict(docs=len(docs), text_first=first, text_second=second, general=len(docs) - first - second, pending=pending,
                     docs_pending=pending, docs_snapshot=len(docs)), (what, c)


def _family(name):
    f = g.families()
    return f["A"] + f["B"] + f["C"] if name == "ABC" else f[name]


# ---------------------------------------------------------------- parity and counts
@pytest.mark.parametrize("api", ["batch", "device"])
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("family", ["A", "B", "C", "ABC"])
def test_family_is_exact_and_takes_its_tier(eng135, eng136, capfd, family, compat, api):
    docs = _family(family)
    res, c = run_counted(eng135 if compat else eng136, capfd, docs, api)
    parity(docs, res, compat, (family, compat, api))
    tier_check(docs, c, (family, compat, api))


# ---------------------------------------------------------------- workspace knobs
def test_first_launch_of_4_kib_moves_the_cap_to_134(eng135, capfd, monkeypatch):
    docs = _family("A")
    monkeypatch.setenv("YGM_SNAP_TEXT", "4")
    res, c = run_counted(eng135, capfd, docs)
    parity(docs, res, True, "YGM_SNAP_TEXT=4")
    tier_check(docs, c, "YGM_SNAP_TEXT=4", first_cap=g.CAP_4K)
    assert c["text_first"] == 3 * 3 and c["text_second"] == 3 * (2 + 5 + 3)      # parts 132 .. 134 of three kinds; the rest up to 865


@pytest.mark.parametrize("compat", [True, False])
def test_without_the_text_tier_the_bytes_are_the_same(eng135, eng136, capfd, monkeypatch, compat):
    docs = g.unique()
    monkeypatch.setenv("YGM_SNAP_NOLDS", "1")
    res, c = run_counted(eng135 if compat else eng136, capfd, docs)
    parity(docs, res, compat, ("YGM_SNAP_NOLDS", compat))
    tier_check(docs, c, ("YGM_SNAP_NOLDS", compat), lds=False)
    assert c["text_first"] == 0 and c["text_second"] == 0


# ---------------------------------------------------------------- no-GC option bytes
@pytest.mark.parametrize("api", ["batch", "device"])
@pytest.mark.parametrize("compat", [True, False])
def test_every_second_document_is_gc_false(eng135, eng136, capfd, compat, api):
    docs = _family("A") + _family("C")
    opts = [k % 2 for k in range(len(docs))]
    res, c = run_counted(eng135 if compat else eng136, capfd, docs, api, opts)
    parity(docs, res, compat, ("gc: false", compat, api), opts)
    tier_check(docs, c, ("gc: false", compat, api))
    plain = [expected(d, compat) for d in docs]
    assert sum(res[k][1] != plain[k][1] for k in range(1, len(docs), 2)) >= 60      # the option changes the bytes


# ---------------------------------------------------------------- residues
def test_every_arena_residue_and_both_tail_paddings(eng135, capfd):
    """Family D through the device form, the 64 bytes after the arena 0xFF and then 0x00: a parser that consumes a byte
    past a document's end gives two answers."""
    docs = g.family_d()
    runs = []
    for tail in (0xFF, 0x00):
        res, c = run_counted(eng135, capfd, docs, "device", tail=tail)
        parity(docs, res, True, ("D", tail))
        tier_check(docs, c, ("D", tail))
        runs.append(res)
    assert runs[0] == runs[1]
    for batch in g.family_d_last():
        runs = []
        for tail in (0xFF, 0x00):
            res, c = run_counted(eng135, capfd, batch, "device", tail=tail)
            parity(batch, res, True, ("D last", batch[-1].name, tail))
            tier_check(batch, c, ("D last", batch[-1].name, tail))
            runs.append(res)
        assert runs[0] == runs[1], batch[-1].name


def test_every_arena_residue_without_the_text_tier(eng136, capfd, monkeypatch):
    """The same batch through k_snap alone: its staged copy starts at a16 = a & ~15, the lanes' inputs at x - a16."""
    monkeypatch.setenv("YGM_SNAP_NOLDS", "1")
    docs = g.family_d()
    for tail in (0xFF, 0x00):
        res, c = run_counted(eng136, capfd, docs, "device", tail=tail)
        parity(docs, res, False, ("D, text tier off", tail))
        tier_check(docs, c, ("D, text tier off", tail), lds=False)


# ---------------------------------------------------------------- staging
@pytest.mark.parametrize("lds", [False, True])
def test_staging_limit_at_every_residue(eng135, capfd, monkeypatch, lds):
    """Family E: the second group of 16 starts at a & 15 = 0, 1, 8, 15 and b - a16 stands at, one and sixteen below and
    above the 40 960 staged bytes; then a group with one 41 000-byte document.  With the text tier on, the documents
    it claimed are skipped by k_snap and still staged.  (Both sides of the limit give the same bytes: this shows the
    placement is right on each side, not which side a group took.)"""
    if not lds:
        monkeypatch.setenv("YGM_SNAP_NOLDS", "1")
    for r, t, docs in g.family_e():
        for api in ("device", "batch"):
            res, c = run_counted(eng135, capfd, docs, api, tail=0xFF)
            parity(docs, res, True, ("E", r, t, lds, api))
            tier_check(docs, c, ("E", r, t, lds, api), lds=lds)


# ---------------------------------------------------------------- documents per wave
def _mixed(n):
    """n documents of every tier, large and small next to each other."""
    f = g.families()
    pool = f["A"][::4] + f["B"] + f["C"][::5] + f["F"]
    step = 29      # (coprime to the pool's size)
    assert len(pool) % step
    return [pool[(k * step) % len(pool)] for k in range(n)]


@pytest.mark.parametrize("lds", [False, True])
def test_documents_per_wave(eng135, capfd, monkeypatch, lds):
    docs = _mixed(67)
    assert {d.tier for d in docs} == set(g.TIERS)
    if not lds:
        monkeypatch.setenv("YGM_SNAP_NOLDS", "1")
    base, c0 = run_counted(eng135, capfd, docs, "device")
    parity(docs, base, True, ("dpw unset", lds))
    tier_check(docs, c0, ("dpw unset", lds), lds=lds)
    for dpw in (1, 3, 16, 64):
        monkeypatch.setenv("YGM_SNAP_DPW", str(dpw))
        res, c = run_counted(eng135, capfd, docs, "device")
        assert res == base, (dpw, [docs[k].name for k in range(len(docs)) if res[k] != base[k]][:6])
        assert c == c0, (dpw, c)


# ---------------------------------------------------------------- scan
@pytest.mark.parametrize("n", [1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025])
def test_scanned_workspace_offsets_at_block_edges(eng135, capfd, monkeypatch, n):
    """Family F with the text tier off: every document's workspace lies at its scanned offset (256 per scan block)."""
    monkeypatch.setenv("YGM_SNAP_NOLDS", "1")
    docs = g.family_f(n, shift=n % 7)
    res, c = run_counted(eng135, capfd, docs, "device" if n % 2 else "batch")
    parity(docs, res, True, ("F", n))
    tier_check(docs, c, ("F", n), lds=False)


def test_scan_past_1024_blocks(eng135, capfd, monkeypatch):
    """262 400 documents: nb = 1 026 scan blocks, the second round of k_snap_scan_top's loop.  Built with numpy,
    compared per kind of document with gathers."""
    import torch
    monkeypatch.setenv("YGM_SNAP_NOLDS", "1")
    n = 262400
    f = g.families()["F"]
    kinds = np.arange(n) % 7
    lens = np.array([len(d.u) for d in f], np.uint64)
    cyc = np.frombuffer(b"".join(d.u for d in f), np.uint8)
    a = np.concatenate([np.tile(cyc, n // 7), cyc[:int(lens[:n % 7].sum())], np.zeros(64, np.uint8)])
    off = np.concatenate([[0], np.cumsum(lens[kinds])]).astype(np.uint64)
    assert off[-1] == len(a) - 64
    dev = torch.device("cuda", 0)
    ta, to = torch.from_numpy(a).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
    capfd.readouterr()
    s0 = eng135.stats()
    t0 = time.time()
    r = eng135.snapshot_device(ta, len(a) - 64, to, n)
    torch.cuda.synchronize()
    NOTES.append("262 400 documents: %.2f s, %d bytes of workspaces" % (time.time() - t0, int(r.data_bytes)))
    s1 = eng135.stats()
    lines = LINE.findall(capfd.readouterr().err)
    pend = int((kinds == 1).sum())
    assert lines == [(str(n), "0", "0", str(n), str(pend))], lines
    assert s1.docs_pending - s0.docs_pending == pend and s1.docs_snapshot - s0.docs_snapshot == n
    sts, offs, ln, data = read_results(r, n, sync=False, raw=True)      # (the wait is above, inside the timed part)
    for k, d in enumerate(f):
        st, e = expected(d, True)
        sel = kinds == k
        if st:
            assert np.isin(sts[sel], [1, 2, 4, 5]).all(), d.name
            continue
        assert (sts[sel] == 0).all() and (ln[sel] == len(e)).all(), d.name
        got = data[offs[sel][:, None] + np.arange(len(e))[None, :]]
        assert (got == np.frombuffer(e, np.uint8)[None, :]).all(), d.name
    ends = np.sort(offs[sts == 0] + ln[sts == 0])
    assert ends[-1] <= int(r.data_bytes)


# ---------------------------------------------------------------- pending list
@pytest.mark.parametrize("n", [1, 1024, 1025])
def test_pending_list(eng135, eng136, capfd, n):
    """The gap document n times among others (k_pend_plan's stride of 1 024; pend_list is filled in arbitrary order)."""
    f = g.families()["F"]
    others = [d for d in f if d.tier != "pending"] + [g.get("B origin on an absent client"), g.get("B 17 client blocks")]
    docs, j = [], 0
    for k in range(n):
        for _ in range(1 + k % 3):
            docs.append(others[j % len(others)])
            j += 1
        docs.append(f[1])
    for eng, compat in ((eng135, True), (eng136, False)):
        res, c = run_counted(eng, capfd, docs, "device" if compat else "batch")
        parity(docs, res, compat, ("pending", n, compat))
        tier_check(docs, c, ("pending", n, compat))
        assert c["pending"] >= n


# ---------------------------------------------------------------- hand-over and reuse on one context
def test_hand_over_and_reuse_on_one_context(capfd, monkeypatch):
    """One context, call after call: the first launch takes the whole batch; none of it; one document for the second
    launch, first and last; only such documents; then large, small and large batches with the text tier switched off
    and on between the calls, over stale claim bytes, slots and workspaces."""
    f = g.families()
    first = [d for d in f["C"][:40]] + f["filler"]
    none = [d for d in f["B"] if d.tier in ("general", "pending", "throws")]
    second = [d for d in f["A"] if d.tier == "second"]
    small = f["filler"][:5] + [second[0], none[0]]
    large = g.unique()
    steps = [("all first", first, True), ("none", none, True), ("a second one first", [second[0]] + first[:30], True),
             ("a second one last", first[:30] + [second[-1]], True), ("all second", second, True),
             ("large", large, True), ("small, tier off", small, False), ("large, tier off", large, False), ("small", small, True),
             ("large again", large, True), ("none, tier off", none, False), ("all first again", first, True)]
    eng = _engine(True)
    try:
        for what, docs, lds in steps:
            if lds:
                monkeypatch.delenv("YGM_SNAP_NOLDS", raising=False)
            else:
                monkeypatch.setenv("YGM_SNAP_NOLDS", "1")
            res, c = run_counted(eng, capfd, docs, "device" if len(what) % 2 else "batch")
            parity(docs, res, True, what)
            tier_check(docs, c, what, lds=lds)
            if what.startswith("all first"):
                assert c["general"] == 0 and c["text_second"] == 0
            if what == "none":
                assert c["text_first"] == 0 and c["text_second"] == 0
            if what.startswith("a second one"):
                assert c["text_second"] == 1 and c["general"] == 0
            if what == "all second":
                assert c["text_first"] == 0 and c["text_second"] == len(docs) == 15
    finally:
        eng.close()

"""The large-document merge tier (k_big_pick, k_big_scan, k_big_val, k_merge_big in its mid and wide size) on the corpus
of large_tier_docs.py: every document bit-exact against the CPU oracle through both device input forms, and -- by the
raw counters of the call (YGM_TIER_COUNTS: the `ygm large tiers:` line) -- picked, scanned, handed on and finished as
its label says.  A cap that drifts by one, a pick that takes the wrong update or a document handed on for no reason
moves a count even where the bytes still come out right.

Then the scan with one and three workgroups for every task and queue block (YGM_BIG_SCAN_GRID), the 13.5 delete-set
order, batch sequences on one fresh context (the tier's scratch, bitmap and second stream are reused from call to
call), and the sequential replay."""
import re

import pytest

import oracle
import large_tier_docs as g
from devrun import engine_fixture, run_merge, same

pytestmark = pytest.mark.gpu

MERGE = re.compile(r"^ygm merge tiers: docs (\d+) lean_defer (\d+) wide_defer (\d+) to_wave (\d+) to_workgroup (\d+) to_large (\d+) "
                   r"to_seq (\d+)$", re.M)
LARGE = re.compile(r"^ygm large tiers: docs (\d+) positions (\d+) tasks (\d+) slow_queue (\d+) wide_first (\d+) mid_first (\d+) "
                   r"mid_to_wide (\d+) to_seq (\d+)$", re.M)
LARGE_NAMES = ("docs", "positions", "tasks", "slow_queue", "wide_first", "mid_first", "mid_to_wide", "to_seq")
EXACT = ("docs", "positions", "tasks", "wide_first", "mid_first", "mid_to_wide", "to_seq")
FORMS = ["off", "lens"]

# Host waits of one merge call that reaches the large tier, from the reads of ygm_merge_v1_device_finish: the lean
# kernels' counters (read_meta), the general chain's (read_meta), the scan's cnt[] copy, the counters after the mid
# size's launch (mid_defer) and after the tier (big_defer) -- the wide size on the second stream is joined by an event,
# not by the host -- and one more read after the sequential replay when a document reached it.
SYNCS_LARGE, SYNCS_SEQ = 5, 6


@pytest.fixture(autouse=True)
def tier_counts(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    monkeypatch.delenv("YGM_BIG_SCAN_GRID", raising=False)


def _engine(**kw):
    from hocuspocus_amd import Engine
    return Engine(0, **kw)


eng = engine_fixture()
eng135 = engine_fixture(compat135=True)
eng_seq = engine_fixture(force_seq=True)


def run_device(eng, docs, form):
    """docs through the u64-offset device API ('off') or the compact one ('lens': 16-bit update lengths)."""
    return run_merge(eng, docs, form)[0]


def forms_of(docs):
    """Both device input forms; the compact form carries 16-bit update lengths, so a batch with an update of 64 KB or
    more has the offset form only."""
    return FORMS if max(len(u) for d in docs for u in d.us) < 0x10000 else FORMS[:1]


def expect(docs, compat135=False):
    """The oracle's results of a batch, computed once per document (kept on the document)."""
    out = []
    for d in docs:
        cache = d.__dict__.setdefault("_oracle", {})
        if compat135 not in cache:
            cache[compat135] = oracle.merge_updates(d.us, compat135=compat135)
        out.append(cache[compat135])
    return out


def run_counted(eng, capfd, docs, form, host=False):
    """One call: results, the call's two tier lines as a dict, and what the engine's statistics rose by."""
    capfd.readouterr()
    s = eng.stats()
    before = (s.docs_big, s.docs_seq, s.host_syncs)
    if host:
        res = eng.merge_updates_batch([d.us for d in docs])
    else:
        res = run_device(eng, [d.us for d in docs], form)
    s = eng.stats()
    after = (s.docs_big, s.docs_seq, s.host_syncs)
    err = capfd.readouterr().err
    merge, large = MERGE.findall(err), LARGE.findall(err)
    assert len(merge) == 1 and len(large) == 1, err
    c = dict(zip(LARGE_NAMES, map(int, large[0])))
    c["to_large"] = int(merge[0][5])
    c["merge_to_seq"] = int(merge[0][6])
    c.update(zip(("docs_big", "docs_seq", "host_syncs"), (a - b for a, b in zip(after, before))))
    return res, c


def _first_diff(a, b):
    """Where two outputs part: (lengths, the differing offsets' count and first ones, bytes there)."""
    if a is None or b is None:
        return None
    at = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
    return (len(a), len(b), len(at), at[:8], [(a[i], b[i]) for i in at[:8]])


def parity(docs, exp, res, what):
    assert len(res) == len(docs) == len(exp)
    bad = [i for i in range(len(docs)) if not same(exp[i], tuple(res[i]))]
    assert not bad, (what, len(bad), [docs[i].name for i in bad[:6]], exp[bad[0]][0], res[bad[0]][0], _first_diff(exp[bad[0]][1], res[bad[0]][1]))
    for i, d in enumerate(docs):
        if d.valid:
            assert res[i][0] == 0, (what, d.name)


def count_check(docs, c, what, compat135=False, force_seq=False, syncs=True):
    p = g.predicted(docs, compat135=compat135, force_seq=force_seq)
    print(what, c)
    assert {k: c[k] for k in EXACT} == {k: p[k] for k in EXACT}, (what, c, p)
    assert c["slow_queue"] >= p["slow_queue"], (what, c, p)
    assert c["to_large"] == p["docs"] and c["merge_to_seq"] == p["to_seq"], (what, c, p)
    assert c["docs_seq"] == p["to_seq"] and c["docs_big"] == p["docs"] - p["to_seq"], (what, c, p)
    if syncs:
        assert c["host_syncs"] == (SYNCS_SEQ if p["to_seq"] else SYNCS_LARGE), (what, c)


def _batches(families):
    return [(f, i, form) for f in families for i, docs in enumerate(g.families()[f]) for form in forms_of(docs)]


@pytest.mark.parametrize("family,index,form", _batches(g.TIERED))
def test_family_is_exact_and_takes_its_path(eng, capfd, family, index, form):
    docs = g.families()[family][index]
    res, c = run_counted(eng, capfd, docs, form)
    parity(docs, expect(docs), res, (family, index, form))
    count_check(docs, c, (family, index, form))


@pytest.mark.parametrize("family,index,form", _batches(g.PARITY_ONLY))
def test_inputs_the_oracle_decides_are_exact(eng, capfd, family, index, form):
    docs = g.families()[family][index]
    res, c = run_counted(eng, capfd, docs, form)
    exp = expect(docs)
    assert len(res) == len(docs) and all(same(exp[i], tuple(res[i])) for i in range(len(docs))), \
        (family, form, [d.name for i, d in enumerate(docs) if not same(exp[i], tuple(res[i]))][:6])
    assert c["docs"] == c["to_large"] == len(docs)


def test_no_line_with_the_knobs_unset(eng, capfd, monkeypatch):
    docs = g.families()["P"][0]
    monkeypatch.delenv("YGM_TIER_COUNTS", raising=False)
    capfd.readouterr()
    res = run_device(eng, [d.us for d in docs], "off")
    assert "ygm" not in capfd.readouterr().err
    parity(docs, expect(docs), res, "knobs unset")


def test_host_waits_per_call(eng, capfd):
    """Mid list only, both lists (the wide size runs on the second stream: joined on the device), a hand-on from the
    mid size, and a call with a document for the sequential replay."""
    big = g.big_docs()
    small = [g.small_doc(i) for i in range(3)]
    for name, docs, want in (("mid only", small, SYNCS_LARGE), ("both lists", small + [big[1]], SYNCS_LARGE),
                             ("wide only", [big[1]], SYNCS_LARGE),
                             ("hand-on", small + [g.find("L", "L 257 log structs")], SYNCS_LARGE),
                             ("to_seq", small + [g.find("W", "W header: ascending clients")], SYNCS_SEQ),
                             ("to_seq by the wide size", [g.find("L", "L 1025 log structs")], SYNCS_SEQ)):
        res, c = run_counted(eng, capfd, docs, "off")
        parity(docs, expect(docs), res, name)
        count_check(docs, c, name, syncs=False)
        assert c["host_syncs"] == want, (name, c)


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("family", ["S", "P"])
def test_one_scan_workgroup_takes_every_task_in_turn(eng, capfd, monkeypatch, family, grid):
    """YGM_BIG_SCAN_GRID = 1 / 3: every task of the batch through the LDS queue and stage of one workgroup's waves,
    every block of the slow queue through one workgroup's counting sort; bytes and counts equal the unset run's."""
    for index, docs in enumerate(g.families()[family]):
        monkeypatch.delenv("YGM_BIG_SCAN_GRID", raising=False)
        base, c0 = run_counted(eng, capfd, docs, "off")
        parity(docs, expect(docs), base, (family, index, "unset"))
        monkeypatch.setenv("YGM_BIG_SCAN_GRID", str(grid))
        for form in forms_of(docs):
            res, c = run_counted(eng, capfd, docs, form)
            bad = [docs[i].name for i in range(len(docs)) if tuple(res[i]) != tuple(base[i])]
            assert not bad, (family, index, grid, form, bad[:6])
            assert {k: c[k] for k in LARGE_NAMES} == {k: c0[k] for k in LARGE_NAMES}, (family, index, grid, form, c, c0)
            count_check(docs, c, (family, index, grid, form))


@pytest.mark.parametrize("form", FORMS)
def test_delete_set_order_135(eng, eng135, capfd, form):
    """Under compat135 a merged delete set of two clients is written in first-seen order: the tier hands the document
    to the sequential replay; one client stays."""
    docs = g.ds_pair()
    for compat, e in ((False, eng), (True, eng135)):
        res, c = run_counted(e, capfd, docs, form)
        parity(docs, expect(docs, compat135=compat), res, ("ds pair", compat, form))
        count_check(docs, c, ("ds pair", compat, form), compat135=compat)
    assert g.predicted(docs, compat135=True)["to_seq"] == 2 and g.predicted(docs)["to_seq"] == 0


@pytest.mark.parametrize("form", FORMS)
def test_scan_family_135(eng135, capfd, form):
    docs = g.families()["S"][0]
    res, c = run_counted(eng135, capfd, docs, form)
    parity(docs, expect(docs, compat135=True), res, ("S", "135", form))
    count_check(docs, c, ("S", "135", form), compat135=True)


@pytest.mark.parametrize("name", sorted(g.reuse_sequences()))
def test_batch_sequences_on_a_fresh_context(capfd, name):
    """Stale bitmap words, grow-only scratch, the second stream: batch after batch on one context, the device and the
    host API in turn."""
    e = _engine()
    try:
        for n, docs in enumerate(g.reuse_sequences()[name]):
            res, c = run_counted(e, capfd, docs, forms_of(docs)[-1 if n % 4 == 2 else 0], host=n % 2 == 1)
            parity(docs, expect(docs), res, (name, n))
            count_check(docs, c, (name, n), syncs=False)
    finally:
        e.close()


def test_sequential_replay(eng_seq, capfd):
    """Family W through the exact sequential replay (force_seq): every document of the tier reaches it, same bytes."""
    for index, docs in enumerate(g.families()["W"]):
        for form in forms_of(docs):
            res, c = run_counted(eng_seq, capfd, docs, form)
            parity(docs, expect(docs), res, ("W", index, form, "seq"))
            count_check(docs, c, ("W", index, form, "seq"), force_seq=True)

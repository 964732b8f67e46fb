"""The wave tier (k_merge_wave, one wave per document) and the workgroup tier (k_merge_fast, one workgroup per
document) on the corpus of general_tier_docs.py: every document bit-exact against the CPU oracle through both device
input forms, and -- by the raw counters of the call (YGM_TIER_COUNTS) -- finished by the tier its caps name.  A cap that
drifts, or a kernel that takes a document one over its cap, moves a count even where the bytes still come out right.

Then the same tiers with one and three waves / workgroups for the whole batch (YGM_WAVE_GRID, YGM_FAST_GRID: a full
document, then an almost empty one, through the same LDS), the 13.5 delete-set order, and the sequential replay."""
import re

import pytest

import oracle
import general_tier_docs as g
from devrun import engine_fixture, run_merge, same

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^ygm merge tiers: docs (\d+) lean_defer (\d+) wide_defer (\d+) to_wave (\d+) to_workgroup (\d+) to_large (\d+) "
                  r"to_seq (\d+)$", re.M)
FORMS = ["off", "lens"]


@pytest.fixture(autouse=True)
def tier_counts(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    monkeypatch.delenv("YGM_WAVE_GRID", raising=False)
    monkeypatch.delenv("YGM_FAST_GRID", raising=False)


eng = engine_fixture()
eng135 = engine_fixture(compat135=True)
eng_seq = engine_fixture(force_seq=True)

_ORACLE = {}


def expect(key, docs, compat135=False):
    """The oracle's results of a batch, computed once."""
    key = (key, compat135)
    if key not in _ORACLE:
        _ORACLE[key] = [oracle.merge_updates(d.us, compat135=compat135) for d in docs]
    return _ORACLE[key]


def run_counted(eng, capfd, docs, form):
    """One device call: results, the call's tier line as a dict, and what the engine's statistics rose by."""
    capfd.readouterr()
    s = eng.stats()
    before = (s.docs_lean, s.docs_fast, s.docs_seq, s.host_syncs)
    res, _ = run_merge(eng, [d.us for d in docs], form)
    s = eng.stats()
    after = (s.docs_lean, s.docs_fast, s.docs_seq, s.host_syncs)
    lines = LINE.findall(capfd.readouterr().err)
    assert len(lines) == 1, lines
    names = ("docs", "lean_defer", "wide_defer", "to_wave", "to_workgroup", "to_large", "to_seq")
    counts = dict(zip(names, map(int, lines[0])))
    counts.update(zip(("docs_lean", "docs_fast", "docs_seq", "host_syncs"), (a - b for a, b in zip(after, before))))
    return res, counts


def parity(docs, exp, res, what):
    assert len(res) == len(docs) == len(exp)
    bad = [i for i in range(len(docs)) if not same(exp[i], res[i])]
    assert not bad, (what, len(bad), [docs[i].name for i in bad[:6]], exp[bad[0]][0], res[bad[0]][0])
    for i, d in enumerate(docs):
        if d.valid:
            assert res[i][0] == 0, (what, d.name)


def tier_check(docs, c, what):
    """The counters of one call over labelled documents.  Documents of fewer than two updates (the fillers in front
    of the residue documents) are returned as they are by the lean kernel; everything else must pass it by."""
    multi = [d for d in docs if len(d.us) >= 2]
    routed = sum(1 for d in multi if g.routed_by_size(d.us))
    beyond = sum(1 for d in multi if d.tier in ("workgroup", "large"))
    large = sum(1 for d in multi if d.tier == "large")
    print(what, c)
    assert c["docs"] == len(docs), what
    assert c["docs_lean"] == len(docs) - len(multi), (what, c)
    assert c["to_wave"] == len(multi) - routed, (what, c)
    assert c["to_workgroup"] == beyond - routed, (what, c)
    assert c["to_large"] == large, (what, c)
    if not large:      # the two general tiers alone: the lean kernels' counters, then the chain's
        assert c["host_syncs"] == 2 and c["docs_seq"] == 0 and c["to_seq"] == 0, (what, c)
        assert c["docs_fast"] == len(multi), (what, c)


def _batches(families):
    return [(f, i) for f in families for i in range(len(g.families()[f]))]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family,index", _batches(g.TIERED))
def test_family_is_exact_and_takes_its_tier(eng, capfd, family, index, form):
    docs = g.families()[family][index]
    key = "%s %d" % (family, index)
    res, c = run_counted(eng, capfd, docs, form)
    parity(docs, expect(key, docs), res, (key, form))
    tier_check(docs, c, (key, form))
    general = [d for d in docs if d.tier != "large"]
    if len(general) < len(docs):     # without the large tier's documents: one host wait for the whole chain
        res, c = run_counted(eng, capfd, general, form)
        parity(general, expect(key + " general", general), res, (key, form, "general"))
        tier_check(general, c, (key, form, "general"))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("family,index", _batches(g.PARITY_ONLY))
def test_throwing_and_non_canonical_inputs_are_exact(eng, capfd, family, index, form):
    docs = g.families()[family][index]
    key = "%s %d" % (family, index)
    res, c = run_counted(eng, capfd, docs, form)
    exp = expect(key, docs)
    assert len(res) == len(docs) and all(same(exp[i], res[i]) for i in range(len(docs))), \
        (key, form, [d.name for i, d in enumerate(docs) if not same(exp[i], res[i])][:6])
    assert c["docs"] == len(docs)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("compat", [False, True])
def test_delete_set_order(eng, eng135, capfd, compat, form):
    """Family G through the 13.6 engine (clients descending) and the 13.5 one (clients in first-seen order), each
    against the oracle of its version; the tiers are the same."""
    docs = g.families()["G"][0]
    res, c = run_counted(eng135 if compat else eng, capfd, docs, form)
    parity(docs, expect("G 0", docs, compat135=compat), res, ("G", compat, form))
    tier_check(docs, c, ("G", compat, form))


def _reuse(eng, capfd, monkeypatch, docs, key, grid, tier):
    exp = expect(key, docs)
    base, c0 = run_counted(eng, capfd, docs, "off")            # the knobs unset
    assert all(same(exp[i], base[i]) for i in range(len(docs))), key
    monkeypatch.setenv("YGM_WAVE_GRID", str(grid))
    monkeypatch.setenv("YGM_FAST_GRID", str(grid))
    for form in FORMS + ["off"]:                              # (the last: a second call of the same kind on the context)
        res, c = run_counted(eng, capfd, docs, form)
        bad = [docs[i].name for i in range(len(docs)) if res[i] != base[i]]
        assert not bad, (key, grid, form, bad[:6])
        assert {k: c[k] for k in ("to_wave", "to_workgroup", "to_large")} == {k: c0[k] for k in ("to_wave", "to_workgroup", "to_large")}
    multi = sum(1 for d in docs if len(d.us) >= 2)
    assert c0["to_wave"] == multi and c0["to_large"] == 0 and c0["docs_lean"] == 0
    assert c0["to_workgroup"] == (multi if tier == "workgroup" else 0)


@pytest.mark.parametrize("grid", [1, 3])
def test_one_wave_takes_full_and_empty_documents_in_turn(eng, capfd, monkeypatch, grid):
    """YGM_WAVE_GRID = 1 / 3: S = 256 then S = 0, D = 128 then D = 0, 64 clients then 1, an erroring document then a
    valid one, 8176 bytes then 40 -- through the LDS of one wave (the parse arrays share their bytes with the scan's;
    the record counters and the segment counts are reset per document)."""
    wave, _ = g.reuse_batches()
    _reuse(eng, capfd, monkeypatch, wave, "reuse wave", grid, "wave")


@pytest.mark.parametrize("grid", [1, 3])
def test_one_workgroup_takes_full_and_small_documents_in_turn(eng, capfd, monkeypatch, grid):
    """YGM_FAST_GRID = 1 / 3: 16384 bytes, S = 512 and D = 256 in turn with the smallest documents that leave the
    wave tier."""
    _, work = g.reuse_batches()
    _reuse(eng, capfd, monkeypatch, work, "reuse workgroup", grid, "workgroup")


@pytest.mark.parametrize("family", ["D", "E", "G"])
def test_sequential_replay(eng_seq, capfd, family):
    """The same documents through the exact sequential replay (force_seq): every document of two or more updates
    reaches it."""
    docs = g.families()[family][0]
    for form in FORMS:
        res, c = run_counted(eng_seq, capfd, docs, form)
        parity(docs, expect("%s 0" % family, docs), res, (family, form, "seq"))
        multi = sum(1 for d in docs if len(d.us) >= 2)
        print(family, form, c)
        assert c["to_seq"] == multi and c["docs_seq"] == multi, (family, form, c)

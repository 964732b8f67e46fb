"""The SV / diff ring walker (dw_walk<MODE, GATHER>, k_sv_table, the ask plan) on the corpus of walker_docs.py: every
item's status and bytes equal yjs's (the oracle, at test time) through the host and the device forms, and -- by the
call's `ygm walk tiers` line (YGM_TIER_COUNTS), the docs_lean / docs_fast deltas and, in device form, each document's
place below or past slot_total -- the walker finishes exactly the documents labelled "walker".  A walker that defers
what it should take, or takes what it should defer, moves a count even where k_doc gets the bytes right.

What this cannot show: on which side of a staging bet a chunk fell (a chunk staged past the ring and dropped is
staged again: the same bytes and the same counts either way), or which of the two decoders took a struct."""
import ctypes
import re

import numpy as np
import pytest

import walker_docs as g
from devrun import engine_fixture, read_results, upload
from walker_docs import expected, flat

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^ygm walk tiers: op (\w+) docs (\d+) walker (\d+) exact (\d+)$", re.M)
EINVAL = 8
NOTES = []


@pytest.fixture(autouse=True)
def tier_counts(monkeypatch):
    monkeypatch.setenv("YGM_TIER_COUNTS", "1")
    for k in ("YGM_WALK_GRID", "YGM_WALK_WAVES_PER_CU", "YGM_CHUNK_MB"):
        monkeypatch.delenv(k, raising=False)
    del NOTES[:]
    yield
    print("\n".join(NOTES))


eng = engine_fixture()


@pytest.fixture(scope="module")
def fam():
    return g.families()


def _dev(blobs, tail):
    """The blobs back to back in a torch allocation, 64 bytes of `tail` after them -> (arena, offsets, bytes)."""
    ta, to, nbytes = upload(blobs, tail=tail)
    assert ta.data_ptr() % 256 == 0
    return ta, to, nbytes


def _read(r, n):
    res, off, _ = read_results(r, n, places=True)
    return res, off


def call(eng, batch, mode, form="host", tail=0x00):
    """One call -> (results, offsets | None, slot_total)."""
    us, svs = [it[1] for it in batch], [it[2] for it in batch]
    if form == "host":
        return (eng.diff_update_batch(us, svs) if mode == "diff" else eng.encode_state_vector_from_update_batch(us)), None, 0
    ta, to, nb = _dev(us, tail)
    if mode == "diff":
        sa, so, _ = _dev(svs, tail)
        r = eng.diff_device(ta, nb, to, sa, so, len(us))
    else:
        r = eng.sv_device(ta, nb, to, len(us))
    res, off = _read(r, len(us))
    return res, off, 2 * nb + 64 * len(us)


def check(eng, capfd, batch, mode, form="host", tail=0x00, what="", compat135=False, op=None, run=None):
    """One counted call over a batch: bytes and statuses against yjs, the line and the stats against the labels, and in
    device form every document's place against its label.  Returns the results."""
    capfd.readouterr()
    s0 = eng.stats()
    res, off, slot_total = run() if run else call(eng, batch, mode, form, tail)
    s1 = eng.stats()
    lines = LINE.findall(capfd.readouterr().err)
    what = (what, mode, form, tail)
    assert len(res) == len(batch), what
    bad = [(k, batch[k][0], res[k][0], expected(batch[k], mode, compat135)[0]) for k in range(len(batch))
           if res[k] != expected(batch[k], mode, compat135)]
    lab = [it[4 if mode == "diff" else 3] for it in batch]
    n, w = len(batch), lab.count(g.WALKER)
    misplaced = [] if off is None else [(k, batch[k][0], lab[k]) for k in range(n) if (off[k] < slot_total) != (lab[k] == g.WALKER)]
    NOTES.append("%s: %s" % (what, lines))
    assert not bad, (what, len(bad), bad[:8])
    assert not misplaced, (what, len(misplaced), misplaced[:12])
    if n:
        assert lines == [(op or mode, str(n), str(w), str(n - w))], (what, lines, (n, w, n - w))
    assert (s1.docs_lean - s0.docs_lean, s1.docs_fast - s0.docs_fast) == (w, n - w), what
    return res


BATCHES = [(k, i) for k, n in (("A", 12), ("B", 3), ("C", 2), ("D", 2), ("E", 1), ("F", 4), ("G", 2)) for i in range(n)]


# ---------------------------------------------------------------- bytes, counts and places, family by family
@pytest.mark.parametrize("mode", ["sv", "diff"])
@pytest.mark.parametrize("fb", BATCHES, ids=lambda x: "%s%d" % x)
def test_batch_is_exact_and_the_walker_takes_its_label(eng, fam, capfd, fb, mode):
    batch = fam[fb[0]][fb[1]]
    host = check(eng, capfd, batch, mode, "host", what=fb)
    ff = check(eng, capfd, batch, mode, "device", 0xFF, what=fb)
    zz = check(eng, capfd, batch, mode, "device", 0x00, what=fb)
    assert host == ff == zz                        # nothing depends on the bytes after the arena


def test_the_batch_list_covers_the_families(fam):
    assert sorted(set(BATCHES)) == sorted((k, i) for k in "ABCDEFG" for i in range(len(fam[k])))


# ---------------------------------------------------------------- scheduling, grids
@pytest.mark.parametrize("grid", [None, "1", "3"])
@pytest.mark.parametrize("mode", ["sv", "diff"])
def test_scheduling(eng, fam, capfd, monkeypatch, mode, grid):
    """Family H: lanes take new documents while one is mid-document; the batch split and the sort at their edges."""
    if grid:
        monkeypatch.setenv("YGM_WALK_GRID", grid)
    for k, batch in enumerate(fam["H"]):
        check(eng, capfd, batch, mode, "device" if k % 2 else "host", 0xFF, what=("H", k, len(batch), grid))


@pytest.mark.parametrize("grid", ["1", "3"])
@pytest.mark.parametrize("mode", ["sv", "diff"])
def test_small_grids_over_a_to_c(eng, fam, capfd, monkeypatch, mode, grid):
    monkeypatch.setenv("YGM_WALK_GRID", grid)
    for fk in "ABC":
        for i, batch in enumerate(fam[fk]):
            check(eng, capfd, batch, mode, "device", 0xFF, what=(fk, i, "grid", grid))


# ---------------------------------------------------------------- one context, call after call
def test_context_reuse(fam, capfd):
    """An all-walker batch, an all-exact one, a mixed one and a smaller one on one context: a stale defer_list, stale
    statuses or a stale state-vector table would show in the bytes or in the counts."""
    from hocuspocus_amd import Engine
    pool = flat(fam["B"]) + flat(fam["D"]) + flat(fam["F"]) + flat(fam["G"])
    for mode, ix in (("diff", 4), ("sv", 3)):
        allw = [it for it in pool if it[ix] == g.WALKER]
        alle = [it for it in pool if it[ix] == g.EXACT]
        mixed = [x for pair in zip(allw, alle) for x in pair]
        assert len(allw) > 100 and len(alle) > 100
        steps = [("walker", allw), ("exact", alle), ("mixed", mixed), ("smaller", mixed[5:40]), ("exact, fewer", alle[:30]),
                 ("walker again", allw[::-1]), ("one", alle[:1]), ("mixed again", mixed[::-1])]
        with Engine(0) as e:
            for k, (what, batch) in enumerate(steps):
                check(e, capfd, batch, mode, "device" if k % 2 else "host", 0xFF, what=("reuse", what))


# ---------------------------------------------------------------- compat135
def test_compat135_over_cuts_and_delete_sets(fam, capfd):
    from hocuspocus_amd import Engine
    with Engine(0, compat135=True) as e:
        for fk in "CG":
            for i, batch in enumerate(fam[fk]):
                for mode in ("sv", "diff"):
                    check(e, capfd, batch, mode, "device" if i else "host", 0xFF, what=(fk, i, "compat135"), compat135=True)


# ---------------------------------------------------------------- shared states
def _shared_device(eng, states, ask, svs, tail=0xFF):
    import torch
    from hocuspocus_amd import engine as E
    ta, to, nb = _dev(states, tail)
    sa, so, _ = _dev(svs, tail)
    tk = torch.from_numpy(np.asarray(ask, np.int64).astype(np.uint32).view(np.int32)).to(ta.device) if len(ask) else None
    r = E._DevResult()
    st = E.lib().ygm_diff_shared_v1_device(eng._ctx, ta.data_ptr(), nb, to.data_ptr(), len(states), sa.data_ptr(), so.data_ptr(),
                                           tk.data_ptr() if tk is not None else None, len(ask), None, ctypes.byref(r))
    assert st == 0, st
    res, off = _read(r, len(ask))
    return res, off


def test_shared_states(eng, capfd):
    """Family I through ygm_diff_shared_v1 and its device form: every ask against yjs, the line `op diff_shared`, and
    the asks' places against slot_total = 2 * (sum of the asked states' lengths) + 64 * asks."""
    states, ask, items = g.family_i()
    svs = [it[2] for it in items]
    host = check(eng, capfd, items, "diff", what="I host", op="diff_shared",
                 run=lambda: (eng.diff_update_shared_batch(states, ask, svs), None, 0))
    total = 2 * sum(len(states[a]) for a in ask) + 64 * len(ask)
    for tail in (0xFF, 0x00):
        dev = check(eng, capfd, items, "diff", "device", tail, what="I device", op="diff_shared",
                    run=lambda: _shared_device(eng, states, ask, svs, tail) + (total,))
        assert dev == host


def test_shared_states_refused_ids(eng, capfd):
    """State ids at or past n_states, and an id below its predecessor: those asks carry YGM_EINVAL (the exact kernel's
    list holds them: they count as `exact`), their neighbours are answered as before."""
    states, ask, items = g.family_i()
    lo = ask.index(1)                              # one ask of state 1, two of state 2, the rest of state 3
    sl = slice(lo, lo + 40)
    ask, items = [a - 1 for a in ask[sl]], items[sl]
    states = states[1:1 + max(ask) + 1]
    assert ask[:4] == [0, 1, 1, 2] and len(states) == 3
    svs = [it[2] for it in items]
    n = len(states)
    bad_at = {4: n, 11: n + 7, 12: 0xFFFFFFFF, 25: 1, 39: n}      # (25: below its predecessor)
    ask2 = list(ask)
    for k, v in bad_at.items():
        ask2[k] = v
    # an ask after a refused one is judged against the refused id as written: keep the followers non-decreasing
    refused = {k for k in range(len(ask2)) if ask2[k] >= n or (k and ask2[k - 1] > ask2[k])}
    assert set(bad_at) <= refused
    capfd.readouterr()
    s0 = eng.stats()
    total = 2 * sum(len(states[a]) for k, a in enumerate(ask2) if k not in refused) + 64 * len(ask2)
    res, off = _shared_device(eng, states, ask2, svs)
    s1 = eng.stats()
    lines = LINE.findall(capfd.readouterr().err)
    lab = [g.EXACT if k in refused else items[k][4] for k in range(len(items))]
    for k, it in enumerate(items):
        if k in refused:
            assert res[k] == (EINVAL, None), (k, res[k])
        else:
            assert res[k] == expected(it, "diff"), (k, it[0])
            assert (off[k] < total) == (lab[k] == g.WALKER), (k, it[0])
    w = lab.count(g.WALKER)
    assert lines == [("diff_shared", str(len(items)), str(w), str(len(items) - w))], lines
    assert (s1.docs_lean - s0.docs_lean, s1.docs_fast - s0.docs_fast) == (w, len(items) - w)

"""SyncStep2 for gc: false documents on the GPU (ygm_sync_step2_opts_v1, ygm_sync_step2_shared_opts_v1): the reference
answers a SyncStep1 with Y.encodeStateAsUpdate(doc, sv) of the live, uncollected document (MessageReceiver.ts:137-138
over a Y.Doc built with yDocOptions { gc: false }, Hocuspocus.ts:331-344), so the deleted Items travel with their content.
Pinned by tests/golden/step2_nogc_v135.json.gz (tools/step2_corpus.js nogc: the bundle's own replies over the no-GC
snapshot corpus, pending states kept; rows where 13.5's writeString throws on a cut surrogate pair are null)."""
import pytest

import oracle
from golden import nogc_fixtures, step2_nogc_rows

pytestmark = pytest.mark.gpu


def _check(rows, res):
    bad = []
    for k, ((_u, _sv, exp, _), got) in enumerate(zip(rows, res)):
        if exp is None:
            if got[0] != 4:   # YGM_ESURROGATE, as the step2 tests of the collected corpus expect
                bad.append(k)
        elif got != (0, exp):
            bad.append(k)
    return bad


def test_gpu_step2_nogc_vs_yjs():
    """Every row with option 1 in 13.5 mode against the bundle's replies."""
    from hocuspocus_amd import Engine
    r = step2_nogc_rows()
    with Engine(0, compat135=True) as e:
        s0 = e.stats().docs_pending
        res = e.sync_step2_batch([u for u, *_ in r], [sv for _, sv, *_ in r], [1] * len(r))
        assert e.stats().docs_pending - s0 >= 100   # the pendingnogc states took the three-way merge
    bad = _check(r, res)
    assert not bad, f"{len(bad)} replies differ from yjs, first {bad[:5]}: {res[bad[0]]}"


def test_gpu_step2_nogc_default_mode():
    """13.6 default mode: the bundle's replies with their delete sets rewritten client-descending (the derived
    expectation test_snapshot_nogc.py checks against the host-compiled kernel code and the oracle).  Where 13.5 throws on
    a cut surrogate pair the default mode writes U+FFFD: for states that integrate completely that reply is the oracle's
    keep-parentSub diff of the GPU's no-GC snapshot."""
    from hocuspocus_amd import Engine
    from golden import ds_to_desc
    r = step2_nogc_rows()
    rows = nogc_fixtures()
    with Engine(0) as e:
        snaps = dict(zip([u for u, _ in rows], e.snapshot_batch([u for u, _ in rows], [1] * len(rows))))
        res = e.sync_step2_batch([u for u, *_ in r], [sv for _, sv, *_ in r], [1] * len(r))
    pend = {u for u, _ in rows[320:400]}
    bad = []
    for k, ((u, sv, exp, _), got) in enumerate(zip(r, res)):
        if exp is not None:
            ok = got == (0, bytes.fromhex(ds_to_desc(exp.hex())))
        elif u in pend:
            ok = got[0] == 0
        else:
            ok = got == oracle.diff_update(snaps[u][1], sv, keep_sub=True)
        if not ok:
            bad.append(k)
    assert not bad, f"{len(bad)} differ, first {bad[:5]}"


def test_gpu_step2_shared_nogc_equals_pairs():
    """The shared form in one call: a no-GC state with three asks, a collected state with two, a no-GC pending state
    with two and a state with no ask; each ask equals the pair form with its state's option."""
    from hocuspocus_amd import Engine
    r = step2_nogc_rows()
    rows = nogc_fixtures()
    by_state = {}
    for u, sv, _e, _ in r:
        by_state.setdefault(u, []).append(sv)
    s_nogc, s_gc, s_pend, s_none = rows[3][0], rows[170][0], rows[325][0], rows[8][0]
    states, opts = [s_nogc, s_gc, s_pend, s_none], [1, 0, 1, 1]
    asks = [(0, sv) for sv in by_state[s_nogc][:3]] + [(1, sv) for sv in by_state[s_gc][:2]] + [(2, sv) for sv in by_state[s_pend][2:4]]
    with Engine(0, compat135=True) as e:
        s0 = e.stats().docs_pending
        got = e.sync_step2_shared_batch(states, [a for a, _ in asks], [sv for _, sv in asks], opts)
        assert e.stats().docs_pending - s0 == 2, "the pending state's two asks take the three-way merge"
        pairs = e.sync_step2_batch([states[a] for a, _ in asks], [sv for _, sv in asks], [opts[a] for a, _ in asks])
        other = e.sync_step2_batch([states[a] for a, _ in asks], [sv for _, sv in asks], [1 - opts[a] for a, _ in asks])
    assert got == pairs and all(st == 0 for st, _ in got)
    assert got[0] != other[0], "the option changes the reply of a state with deletions"
    exp = {(u, sv): e for u, sv, e, _ in r}
    for (a, sv), g in zip(asks, got):
        if opts[a]:
            assert g == (0, exp[(states[a], sv)])


def test_gpu_step2_shared_nogc_split_state_and_bad_byte(monkeypatch):
    """One no-GC state whose asks alone exceed a 1 MB chunk budget is staged (and snapshotted) in several chunks, each
    carrying its option byte; a collected state follows it.  The replies equal the unchunked call's.  A bad option byte
    gives each ask of its state YGM_EINVAL and leaves the other state's asks alone."""
    from hocuspocus_amd import Engine
    from hocuspocus_amd.engine import EINVAL
    rows = nogc_fixtures()
    by_state = {}
    for u, sv, e, _ in step2_nogc_rows():
        if e is not None:
            by_state.setdefault(u, []).append((sv, e))
    big = max((u for u, _ in rows[:320] if len(by_state.get(u, [])) >= 3), key=len)
    other = rows[425][0]
    n_big = (1 << 20) // len(big) + 200
    states, opts = [big, other], [1, 0]
    asks = [0] * n_big + [1] * 3
    svs = [by_state[big][k % 3][0] for k in range(n_big)] + [sv for sv, _ in by_state[other][:3]]
    with Engine(0, compat135=True) as e:
        ref = e.sync_step2_shared_batch(states, asks, svs, opts)
    assert ref[:3] == [(0, by_state[big][k][1]) for k in range(3)] and all(st == 0 for st, _ in ref)
    monkeypatch.setenv("YGM_CHUNK_MB", "1")
    with Engine(0, compat135=True) as e:
        s0 = e.stats().docs_snapshot
        got = e.sync_step2_shared_batch(states, asks, svs, opts)
        assert e.stats().docs_snapshot - s0 >= 3, "the state was not split over chunks"
        bad = e.sync_step2_shared_batch(states, asks, svs, [4, 0])
    assert got == ref
    assert bad[:n_big] == [(EINVAL, None)] * n_big and bad[n_big:] == ref[n_big:]

"""Many versions restored from one stored state on the GPU (ygm_version_restore_shared_v1 and its device-resident form,
through engine.py): fixture parity in both yjs modes with per-ask options, ask counts around a wave and a scan block
in every shape the plan and status kernels index by, statuses carried from state and version to the ask alone, bad ids,
the copy kernel's alignment sweep behind leading asks, one state split over several chunks, and the old entry points
beside the new one.  Every expectation is yjs 13.5.16's, from tests/golden/version_history_v135.json.gz
(test_version_shared.py) and, grouped by equal state, tests/golden/version_v135.json.gz (test_version.py) -- never the
pair form run here."""
import numpy as np
import pytest

from devrun import engine_fixture, read_results, upload
from golden import REFUSALS, UNSUP_STATE, _sv, expected, fixtures, history_docs, version_rows

pytestmark = pytest.mark.gpu

EINVAL = 8


eng135 = engine_fixture(compat135=True)


@pytest.fixture(scope="module")
def corpus():
    """-> (states, asks): every document of the history fixture, then the rows of version_v135 grouped by equal state
    (first-seen order, a state's rows in row order); an ask is (state index, row with version / restored / restored_nogc)"""
    states, asks = [], []
    for d in history_docs():
        states.append(d["state"])
        asks += [(len(states) - 1, v) for v in d["versions"]]
    ix, by = {}, []
    for r in version_rows():
        if r["state"] not in ix:
            ix[r["state"]] = len(by)
            by.append([])
        by[ix[r["state"]]].append(r)
    for s, rs in zip(ix, by):
        states.append(s)
        asks += [(len(states) - 1, r) for r in rs]
    return states, asks


def _want(row, opt, mode=1):
    e = expected(row, "restored_nogc" if opt else "restored", mode)
    return (EINVAL, None) if e is None else (0, e)


def _device_call(e, states, ask_state, versions, opts=None):
    import torch
    ts, tso, sb = upload(states)
    tv, tvo, _ = upload(versions)
    dev = ts.device
    ta = torch.from_numpy(np.asarray(ask_state, np.int64).astype(np.uint32).view(np.int32).copy()).to(dev) if len(ask_state) else torch.zeros(1, dtype=torch.int32, device=dev)
    topt = 0 if opts is None else torch.from_numpy(np.asarray(list(opts) + [0], np.uint8)).to(dev)
    r = e.version_restore_shared_device(ts, sb, tso, len(states), tv, tvo, ta, len(ask_state), d_restored_opt=topt)
    return read_results(r, len(ask_state))


# ---------------------------------------------------------------------------------------- fixture parity
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("form", ["host", "device"])
def test_gpu_shared_fixture_parity(corpus, form, mode):
    """Every ask of both fixtures in one call, options alternating per ask: yjs's bytes (their client-descending rewrite
    in the default mode), YGM_EINVAL where yjs throws; each state snapshotted once, each restored document once."""
    from hocuspocus_amd import Engine
    states, asks = corpus
    ask_state, versions = [a for a, _ in asks], [r["version"] for _, r in asks]
    opts = [k % 2 for k in range(len(asks))]
    assert len(states) > 100 and len(asks) > len(states) + 150
    with Engine(0, compat135=bool(mode)) as e:
        s0 = e.stats()
        if form == "host":
            got = e.restore_version_shared_batch(states, ask_state, versions, opts)
        else:
            got = _device_call(e, states, ask_state, versions, opts)
        s1 = e.stats()
    bad = [k for k, ((_, r), o) in enumerate(zip(asks, opts)) if got[k] != _want(r, o, mode)]
    assert not bad, f"{len(bad)} of {len(asks)} differ, first {bad[:6]}"
    assert s1.docs_snapshot - s0.docs_snapshot == len(states) + len(asks)


# ---------------------------------------------------------------------------------------- ask counts and shapes
SHAPES = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 1, 0))   # asks per state, in proportion


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_gpu_shared_ask_counts(eng135, n):
    """n asks over 3 states: spread over all of them, a state with no ask at the front, in the middle and at the end,
    and all asks on one state; options alternate inside every wave."""
    docs = [d for d in history_docs() if d["family"] in ("text", "clients", "many")][:3]
    assert len(docs) == 3
    states = [d["state"] for d in docs]
    for shape in SHAPES:
        live = [s for s in range(3) if shape[s]]
        ask_state = sorted(live[k % len(live)] for k in range(n))
        rows = [docs[s]["versions"][(3 * k) % len(docs[s]["versions"])] for k, s in enumerate(ask_state)]
        opts = [k % 2 for k in range(n)]
        got = eng135.restore_version_shared_batch(states, ask_state, [r["version"] for r in rows], opts)
        assert got == [_want(r, o) for r, o in zip(rows, opts)], shape
        assert eng135.restore_version_shared_batch(states, ask_state, [r["version"] for r in rows]) == [_want(r, 0) for r in rows], shape


# ---------------------------------------------------------------------------------------- statuses
def _state7_row():
    return [r for r in version_rows() if r["note"] == "cut at a struct boundary"][0]


def test_gpu_shared_statuses(eng135):
    """An EUNSUPPORTED state and an empty state carry their status to each of their asks, the neighbouring states' asks
    unchanged; every row of the refusal table fails only its own ask among good asks of the same state."""
    docs = history_docs()
    a, c = docs[1], docs[2]
    s7 = _state7_row()
    assert s7["version"] == _sv([(7, 3)])
    states = [a["state"], UNSUP_STATE, s7["state"], b"", c["state"]]
    ask_state, versions, want = [], [], []

    def ask(s, v, w):
        ask_state.append(s); versions.append(v); want.append(w)
    for v in a["versions"][:4]:
        ask(0, v["version"], _want(v, 0))
    for v in (_sv([(5, 1)]), _sv([]), a["versions"][0]["version"]):
        ask(1, v, (9, None))
    for _n, mk, w in REFUSALS:
        ask(2, s7["version"], (0, s7["restored"]))
        ask(2, mk(), (w, None))
    ask(2, s7["version"], (0, s7["restored"]))
    for v in (_sv([]), s7["version"]):
        ask(3, v, (1, None))
    for v in c["versions"][:4]:
        ask(4, v["version"], _want(v, 0))
    assert eng135.restore_version_shared_batch(states, ask_state, versions) == want
    assert _device_call(eng135, states, ask_state, versions) == want


def test_gpu_shared_bad_option_bytes(eng135):
    """A bad option byte at ask 0, in the middle of a wave and at the last ask: YGM_EINVAL there and nothing else."""
    docs = [d for d in history_docs() if d["family"] in ("text", "clients")][:4]
    states = [d["state"] for d in docs]
    asks = [(s, v) for s, d in enumerate(docs) for v in d["versions"]][:70]
    assert len(asks) == 70
    ask_state, versions = [s for s, _ in asks], [v["version"] for _, v in asks]
    opts = [k % 2 for k in range(70)]
    ref = [_want(v, o) for (_, v), o in zip(asks, opts)]
    assert eng135.restore_version_shared_batch(states, ask_state, versions, opts) == ref
    for b in (2, 0xFF):
        o = list(opts)
        for k in (0, 37, 69):
            o[k] = b
        got = eng135.restore_version_shared_batch(states, ask_state, versions, o)
        for k in range(70):
            assert got[k] == ((EINVAL, None) if k in (0, 37, 69) else ref[k]), (b, k)


# ---------------------------------------------------------------------------------------- bad ids
def test_gpu_shared_bad_ids(eng135):
    """Host form: an out-of-range or decreasing id is refused before any device work.  Device form: such an id is never
    used as an index, and that ask alone carries YGM_EINVAL."""
    from hocuspocus_amd.engine import YjsError
    docs = [d for d in history_docs() if d["family"] == "clients"][:3]
    states = [d["state"] for d in docs]
    calls = eng135.stats().calls
    for bad_ask in ([1, 0], [0, 3], [3], [0, 1, 0]):
        with pytest.raises(YjsError) as ei:
            eng135.restore_version_shared_batch(states, bad_ask, [docs[0]["versions"][0]["version"]] * len(bad_ask))
        assert ei.value.code == EINVAL
    assert eng135.stats().calls == calls
    ask_state = [0, 1, 0, 1, 2, 9]   # ask 2 is below its predecessor, ask 5 out of range
    rows = [docs[min(s, 2)]["versions"][k] for k, s in enumerate(ask_state)]
    got = _device_call(eng135, states, ask_state, [r["version"] for r in rows])
    assert got == [(EINVAL, None) if k in (2, 5) else _want(r, 0) for k, r in enumerate(rows)]


# ---------------------------------------------------------------------------------------- alignment
def test_gpu_shared_alignment_sweep(eng135):
    """The 32 align rows (kept runs starting at every source phase mod 16) as asks behind 0, 1 and 5 leading asks of
    another state: the destination phases vary while the sources stay in place."""
    al = [r for r in version_rows() if r["family"] == "align"]
    assert len(al) == 32 and len({r["state"] for r in al}) == 32
    lead = history_docs()[0]
    states = [lead["state"]] + [r["state"] for r in al]
    for n_lead in (0, 1, 5):
        lv = lead["versions"][:n_lead]
        ask_state = [0] * n_lead + list(range(1, 33))
        versions = [v["version"] for v in lv] + [r["version"] for r in al]
        got = eng135.restore_version_shared_batch(states, ask_state, versions, [1] * len(versions))
        assert got == [_want(v, 1) for v in lv] + [(0, r["restored_nogc"]) for r in al], n_lead
        got = eng135.restore_version_shared_batch(states, ask_state, versions)
        assert got == [_want(v, 0) for v in lv] + [(0, r["restored"]) for r in al], n_lead


# ---------------------------------------------------------------------------------------- chunking
def test_gpu_shared_chunked_host_api(monkeypatch):
    """YGM_CHUNK_MB=1: the ~300 KB state's six asks are 2.1 MB of virtual bytes, split two asks per chunk over three
    chunks that each stage and snapshot the state again; small states before and after it.  Equal to the unchunked
    result and to the fixture; each chunk stages its asks' option bytes."""
    from hocuspocus_amd import Engine
    docs = history_docs()
    big = [d for d in docs if d["family"] == "large"][0]
    small = [d for d in docs if d["family"] == "clients"][:2]
    order = [small[0], big, small[1]]
    states = [d["state"] for d in order]
    asks = [(s, v) for s, d in enumerate(order) for v in (d["versions"] if d is big else d["versions"][:3])]
    ask_state, versions = [s for s, _ in asks], [v["version"] for _, v in asks]
    opts = [1 if k % 3 == 0 else 0 for k in range(len(asks))]
    assert len(big["versions"]) >= 6
    with Engine(0, compat135=True) as e:
        s0 = e.stats()
        ref = e.restore_version_shared_batch(states, ask_state, versions, opts)
        s1 = e.stats()
    assert s1.calls - s0.calls == 2 and s1.docs_snapshot - s0.docs_snapshot == 3 + len(asks)
    monkeypatch.setenv("YGM_CHUNK_MB", "1")
    with Engine(0, compat135=True) as e:
        s0 = e.stats()
        got = e.restore_version_shared_batch(states, ask_state, versions, opts)
        s1 = e.stats()
    assert got == ref
    assert ref == [_want(v, o) for (_, v), o in zip(asks, opts)]
    # at least the three chunks of the split state and one more, two snapshot batches each
    assert s1.calls - s0.calls >= 8, "the batch was not chunked"
    assert s1.docs_snapshot - s0.docs_snapshot >= 5 + len(asks)


# ---------------------------------------------------------------------------------------- the old entry points
def test_gpu_shared_leaves_old_entry_points_unchanged(eng135):
    """restore_version_batch and snapshot_batch on the same context return the same bytes before and after a shared
    call."""
    rows = fixtures()[:80]
    us = [u for u, _ in rows]
    good = [r for r in version_rows() if r["restored"] is not None][:40]
    st, vs = [r["state"] for r in good], [r["version"] for r in good]
    snap = eng135.snapshot_batch(us)
    pair = eng135.restore_version_batch(st, vs)
    assert snap == [(0, e) for _, e in rows] and pair == [(0, r["restored"]) for r in good]
    d = history_docs()[0]
    n = len(d["versions"])
    assert eng135.restore_version_shared_batch([d["state"]], [0] * n, [v["version"] for v in d["versions"]]) == [_want(v, 0) for v in d["versions"]]
    assert eng135.snapshot_batch(us) == snap
    assert eng135.restore_version_batch(st, vs) == pair

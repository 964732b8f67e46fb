"""Version history on the GPU (ygm_version_take_v1 / ygm_version_restore_v1 and their device-resident forms, through
engine.py): fixture parity in both yjs modes, batch sizes around a wave, option bytes, mixed statuses, the copy
kernel's alignment sweep, the chunked host API, and the old entry points beside the new ones.  The vectors are those
of test_version.py (tests/golden/version_v135.json.gz)."""
import numpy as np
import pytest

from devrun import engine_fixture, read_results, upload
from golden import REFUSALS, UNSUP_STATE, _sv, expected, fixtures, version_rows

pytestmark = pytest.mark.gpu

eng135 = engine_fixture(compat135=True)


@pytest.fixture(scope="module")
def rows():
    return version_rows()


@pytest.fixture(scope="module")
def good(rows):
    """Rows yjs answers, with their 13.5 expectations."""
    return [r for r in rows if r["restored"] is not None]


def _check(rows, take, res, resn, mode):
    bad = []
    for k, r in enumerate(rows):
        if take is not None and take[k] != (0, expected(r, "take", mode)):
            bad.append((k, "take"))
        for key, g in (("restored", res), ("restored_nogc", resn)):
            e = expected(r, key, mode)
            if e is None:
                if g[k][0] != 8:
                    bad.append((k, key + " not EINVAL"))
            elif g[k] != (0, e):
                bad.append((k, key))
    return bad


@pytest.mark.parametrize("mode", [1, 0])
def test_gpu_version_fixture_parity(rows, mode):
    """Every row through the host API: take, restored (option 0) and restored_nogc (option 1), the 13.5 bytes and their
    client-descending rewrite in the default mode; rows yjs throws on carry YGM_EINVAL; the pending and crafted
    families leave pending parts after the cut."""
    from hocuspocus_amd import Engine
    states, versions = [r["state"] for r in rows], [r["version"] for r in rows]
    with Engine(0, compat135=bool(mode)) as e:
        s0 = e.stats()
        take = e.take_version_batch(states)
        s1 = e.stats()
        assert s1.docs_snapshot - s0.docs_snapshot == len(rows)
        res = e.restore_version_batch(states, versions)
        s2 = e.stats()
        assert s2.docs_snapshot - s1.docs_snapshot == 2 * len(rows)
        resn = e.restore_version_batch(states, versions, [1] * len(rows))
        bad = _check(rows, take, res, resn, mode)
        assert not bad, f"{len(bad)} results differ, first {bad[:6]}"
        for fam in ("pending", "crafted"):
            sub = [r for r in rows if r["family"] == fam]
            p0 = e.stats().docs_pending
            e.restore_version_batch([r["state"] for r in sub], [r["version"] for r in sub])
            assert e.stats().docs_pending > p0, fam


@pytest.mark.parametrize("mode", [1, 0])
def test_gpu_version_device_forms(rows, mode):
    """The same parity through ygm_version_take_v1_device / ygm_version_restore_v1_device, options alternating."""
    import torch
    from hocuspocus_amd import Engine
    n = len(rows)
    ts, tso, sb = upload([r["state"] for r in rows])
    tv, tvo, _ = upload([r["version"] for r in rows])
    opts = [k % 2 for k in range(n)]
    topt = torch.from_numpy(np.asarray(opts, np.uint8)).to(ts.device)
    with Engine(0, compat135=bool(mode)) as e:
        take = read_results(e.version_take_device(ts, sb, tso, n), n)
        got = read_results(e.version_restore_device(ts, tso, tv, tvo, n, d_restored_opt=topt), n)
        got0 = read_results(e.version_restore_device(ts, tso, tv, tvo, n), n)
    res = [got0[k] for k in range(n)]
    resn = [got[k] if opts[k] else (0, expected(rows[k], "restored_nogc", mode)) if rows[k]["restored"] is not None else (8, None) for k in range(n)]
    bad = _check(rows, take, res, resn, mode)
    assert not bad, f"{len(bad)} results differ, first {bad[:6]}"
    assert all(got[k] == got0[k] for k in range(n) if not opts[k])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_gpu_version_batch_sizes(eng135, good, n):
    """Batches around a wave and a scan block; options 0 and 1 alternate inside every wave."""
    sub = [good[(7 * k) % len(good)] for k in range(n)]
    opts = [k % 2 for k in range(n)]
    take = eng135.take_version_batch([r["state"] for r in sub])
    res = eng135.restore_version_batch([r["state"] for r in sub], [r["version"] for r in sub], opts)
    assert take == [(0, r["take"]) for r in sub]
    assert res == [(0, r["restored_nogc"] if o else r["restored"]) for r, o in zip(sub, opts)]
    assert eng135.restore_version_batch([r["state"] for r in sub], [r["version"] for r in sub]) == [(0, r["restored"]) for r in sub]


def test_gpu_version_bad_option_bytes(eng135, good):
    """A bad option byte at index 0, in the middle of a wave and at the last document: YGM_EINVAL there, the neighbours'
    bytes unchanged."""
    sub = good[:70]
    st, vs = [r["state"] for r in sub], [r["version"] for r in sub]
    opts = [k % 2 for k in range(len(sub))]
    ref = eng135.restore_version_batch(st, vs, opts)
    assert ref == [(0, r["restored_nogc"] if o else r["restored"]) for r, o in zip(sub, opts)]
    for v in (2, 0xFF):
        o = list(opts)
        for k in (0, 37, len(sub) - 1):
            o[k] = v
        got = eng135.restore_version_batch(st, vs, o)
        for k in range(len(sub)):
            assert got[k] == ((8, None) if k in (0, 37, len(sub) - 1) else ref[k]), (v, k)


def test_gpu_version_mixed_statuses(eng135, good, rows):
    """A malformed version, a clock beyond the state, an EUNSUPPORTED state and every row of the refusal table, each
    between good neighbours whose bytes do not change."""
    state7 = [r for r in rows if r["note"] == "cut at a struct boundary"][0]["state"]
    cases = [(state7, mk(), want) for _n, mk, want in REFUSALS] + [(UNSUP_STATE, _sv([(5, 1)]), 9), (b"", _sv([]), 1)]
    st, vs, want = [], [], []
    for k, (s, v, w) in enumerate(cases):
        g = good[(5 * k) % len(good)]
        st += [g["state"], s]; vs += [g["version"], v]; want += [(0, g["restored"]), (w, None)]
    g = good[-1]
    st.append(g["state"]); vs.append(g["version"]); want.append((0, g["restored"]))
    assert eng135.restore_version_batch(st, vs) == want
    take = eng135.take_version_batch(st)
    assert [t[0] for t in take] == [9 if s == UNSUP_STATE else 1 if s == b"" else 0 for s in st]


def test_gpu_version_alignment_sweep(eng135, rows):
    """32 copies of one edge document under root names of 1..32 bytes: the kept runs start at every source phase mod
    16; alone, and shifted through the batch so the destination phases vary too."""
    al = [r for r in rows if r["family"] == "align"]
    assert len(al) == 32 and len({len(r["state"]) for r in al}) == 32
    for shift in (0, 1, 5):
        sub = al[shift:] + al[:shift]
        res = eng135.restore_version_batch([r["state"] for r in sub], [r["version"] for r in sub], [1] * 32)
        assert res == [(0, r["restored_nogc"]) for r in sub], shift
        assert eng135.restore_version_batch([r["state"] for r in sub], [r["version"] for r in sub]) == [(0, r["restored"]) for r in sub]


def test_gpu_version_chunked_host_api(good, monkeypatch):
    """YGM_CHUNK_MB=1 over a little more than 2 MB of rows equals the unchunked result: each chunk carries its slice of
    the versions and of the option bytes."""
    from hocuspocus_amd import Engine
    size = sum(len(r["state"]) for r in good)
    reps = (2 * 1024 * 1024 + 100000) // size + 1
    sub = good * reps
    assert 2 * 1024 * 1024 < sum(len(r["state"]) for r in sub) < 3 * 1024 * 1024
    st, vs = [r["state"] for r in sub], [r["version"] for r in sub]
    opts = [1 if k % 3 == 0 else 0 for k in range(len(sub))]
    with Engine(0, compat135=True) as e:
        ref = e.restore_version_batch(st, vs, opts)
        ref_take = e.take_version_batch(st)
    monkeypatch.setenv("YGM_CHUNK_MB", "1")
    with Engine(0, compat135=True) as e:
        s0 = e.stats().calls
        got = e.restore_version_batch(st, vs, opts)
        assert e.stats().calls - s0 >= 6, "the batch was not chunked"
        got_take = e.take_version_batch(st)
    assert got == ref and got_take == ref_take
    assert all(ref[k] == (0, sub[k]["restored_nogc"] if opts[k] else sub[k]["restored"]) for k in range(len(sub)))
    assert ref_take == [(0, r["take"]) for r in sub]


def test_gpu_old_entry_points_unchanged(eng135, good):
    """snapshot_batch on the same context returns the same bytes before and after a restore call."""
    rows = fixtures()[:80]
    us = [u for u, _ in rows]
    before = eng135.snapshot_batch(us)
    assert before == [(0, e) for _, e in rows]
    eng135.restore_version_batch([r["state"] for r in good[:40]], [r["version"] for r in good[:40]])
    eng135.take_version_batch([r["state"] for r in good[:40]])
    assert eng135.snapshot_batch(us) == before
    assert eng135.snapshot_batch(us, [1] * len(us)) == eng135.snapshot_batch(us, bytes([1]) * len(us))

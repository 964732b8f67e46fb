"""Snapshots of gc: false documents on the GPU (ygm_snapshot_opts_v1 and its device-resident form, through engine.py):
fixture parity in both yjs modes, no change without options, both option values in one wave and beside the flat-text
tier, tier membership against the host-built flat-text twin, bad option bytes, and the chunked host API.  The vectors
and the host twins are those of test_snapshot_nogc.py."""
import shutil

import numpy as np
import pytest

from devrun import engine_fixture, read_results, to_device, upload
from golden import fixtures, nogc_fixtures, text_fixtures
from twins import NOGC, build_twin, run_snaptext

pytestmark = pytest.mark.gpu


eng135 = engine_fixture(compat135=True)


@pytest.fixture(scope="module")
def nrows():
    return nogc_fixtures()


def _bad(res, exp):
    return [k for k in range(len(exp)) if res[k] != exp[k]]


def test_gpu_nogc_fixture_parity(eng135, nrows):
    """Every row with option 1, 13.5 mode (the bundle's bytes) and the 13.6 default (client-descending delete sets),
    the pending rows through the three-way merge."""
    from golden import ds_to_desc
    from hocuspocus_amd import Engine
    us = [u for u, _ in nrows]
    s0 = eng135.stats()
    res = eng135.snapshot_batch(us, [1] * len(us))
    bad = _bad(res, [(0, e) for _, e in nrows])
    assert not bad, f"{len(bad)} documents differ from yjs (gc: false), first {bad[:5]}: {res[bad[0]]}"
    assert eng135.stats().docs_pending - s0.docs_pending >= 40
    with Engine(0) as e:
        res = e.snapshot_batch(us, bytes([1]) * len(us))
    bad = _bad(res, [(0, bytes.fromhex(ds_to_desc(x.hex()))) for _, x in nrows])
    assert not bad, f"default mode: {len(bad)} documents differ, first {bad[:5]}"


def test_gpu_no_options_no_change(eng135):
    """The old entry point, the new one with NULL and the new one with an all-zero array: the same, the fixtures' bytes."""
    rows = fixtures()
    us = [u for u, _ in rows]
    old = eng135.snapshot_batch(us)
    assert old == [(0, e) for _, e in rows]
    from hocuspocus_amd import engine as eng
    import ctypes
    arena, off = eng._pack(us)
    res = eng._Result()
    assert eng.lib().ygm_snapshot_opts_v1(eng135._ctx, arena, eng._ptr(off), None, len(us), ctypes.byref(res)) == 0
    assert eng135._unpack(res) == old
    assert eng135.snapshot_batch(us, bytes(len(us))) == old


def _mixed_batch(nrows):
    """48 documents: 12 general and 12 flat-text updates that have both expectations, interleaved, each twice at adjacent
    indices with options 0 then 1 -> (updates, options, expected)"""
    gen, txt = fixtures(), text_fixtures()
    us, opts, exp = [], [], []
    for k in range(12):
        for gc_row, ng_row in ((gen[k], nrows[400 + k]), (txt[k], nrows[424 + k])):
            assert gc_row[0] == ng_row[0]
            us += [gc_row[0], gc_row[0]]
            opts += [0, 1]
            exp += [(0, gc_row[1]), (0, ng_row[1])]
    return us, opts, exp


@pytest.mark.parametrize("env", [None, "YGM_SNAP_DPW", "YGM_SNAP_NOLDS"])
def test_gpu_mixed_lanes(eng135, nrows, monkeypatch, env):
    """Both option values in one k_snap wave (16 documents per wave) and next to documents k_snap_text claims; with one
    document per wave; and with the flat-text tier off (every document in k_snap, options alternating lane by lane)."""
    us, opts, exp = _mixed_batch(nrows)
    assert len(us) == 48 and sum(a != b for a, b in zip(exp[0::2], exp[1::2])) >= 20
    if env:
        monkeypatch.setenv(env, "1")
    res = eng135.snapshot_batch(us, opts)
    bad = _bad(res, exp)
    assert not bad, f"{env}: {len(bad)} documents differ, first {bad[:5]}"


def _device_snapshot(eng, us, opts):
    """ygm_snapshot_opts_v1_device -> ((status, bytes | None) per document, their offsets, the arena's bytes)"""
    ta, to, nbytes = upload(us)
    topt = to_device(np.asarray(opts, np.uint8))[0] if opts is not None else 0
    r = eng.snapshot_device(ta, nbytes, to, len(us), d_doc_opt=topt)
    out, offs, _ = read_results(r, len(us), places=True)
    return out, offs, nbytes


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_gpu_tier_membership(eng135, nrows, tmp_path):
    """The documents whose output lies in the slot region (off < 2 arena_bytes + 64 n_docs: k_snap_text claimed them)
    are those the host-built flat-text twin takes with the same option at 6 KiB or, failing that, 24 KiB (the two
    launches).  The batch holds no-GC documents for each launch: small flat text, flat text past the 6 KiB workspace
    (the largest text sessions, run as gc: false documents), and general documents for k_snap; options alternate."""
    exe = build_twin(tmp_path, "snaptext")
    txt = text_fixtures()
    us = [u for u, _ in nrows[150:200]] + [u for u, _ in txt[296:320]] + [u for u, _ in nrows[424:448]]
    opts = [(k + 1) % 2 if k % 3 else 1 for k in range(len(us))]
    want, first, second = set(), set(), set()
    for o in (0, 1):
        t6, eq6, _ = run_snaptext(exe, tmp_path, us, 1 | (NOGC if o else 0), 6144)
        t24, eq24, _ = run_snaptext(exe, tmp_path, us, 1 | (NOGC if o else 0), 24576)
        assert all(eq6[k] for k in t6) and all(eq24[k] for k in t24)
        mine = {k for k in range(len(us)) if opts[k] == o}
        want |= (set(t6) | set(t24)) & mine
        if o:
            first, second = set(t6) & mine, (set(t24) - set(t6)) & mine
    assert first and second, "the batch needs a no-GC document for each launch of k_snap_text"
    assert len(want) < len(us)
    res, offs, arena_bytes = _device_snapshot(eng135, us, opts)
    slots = {k for k in range(len(us)) if res[k][0] == 0 and offs[k] < 2 * arena_bytes + 64 * len(us)}
    assert slots == want, f"only on the GPU {sorted(slots - want)[:5]}, only in the twin {sorted(want - slots)[:5]}"
    assert res == eng135.snapshot_batch(us, opts)


def test_gpu_bad_option_bytes(eng135, nrows):
    """Option bytes 2 and 0xFF at index 0, in the middle of a wave and at the last document: YGM_EINVAL for those, their
    neighbours' bytes as without them."""
    from hocuspocus_amd.engine import EINVAL
    us = [u for u, _ in nrows[130:170]]   # 30 general sessions, then 10 flat-text ones
    opts = [1] * len(us)
    ref = eng135.snapshot_batch(us, opts)
    assert all(st == 0 for st, _ in ref)
    for v in (2, 0xFF):
        o = list(opts)
        for k in (0, 21, len(us) - 1):
            o[k] = v
        got = eng135.snapshot_batch(us, o)
        for k in range(len(us)):
            assert got[k] == ((EINVAL, None) if k in (0, 21, len(us) - 1) else ref[k]), (v, k)
    o = [0] * len(us)
    o[5] = 3
    got = eng135.snapshot_batch(us, o)
    ref0 = eng135.snapshot_batch(us)
    assert got[5] == (EINVAL, None) and got[:5] + got[6:] == ref0[:5] + ref0[6:]


def test_gpu_chunked_host_api(nrows, monkeypatch):
    """YGM_CHUNK_MB=1 over a little more than 2 MB of fixture rows with options of period 3: each chunk carries its slice
    of the option array, whatever the phase at its boundary."""
    from hocuspocus_amd import Engine
    base = [u for u, _ in nrows]
    reps = (2 * 1024 * 1024 + 100000) // sum(len(u) for u in base) + 1
    us = base * reps
    assert 2 * 1024 * 1024 < sum(len(u) for u in us) < 3 * 1024 * 1024
    opts = [1 if k % 3 == 0 else 0 for k in range(len(us))]
    with Engine(0, compat135=True) as e:
        ref = e.snapshot_batch(us, opts)
    monkeypatch.setenv("YGM_CHUNK_MB", "1")
    with Engine(0, compat135=True) as e:
        s0 = e.stats().calls
        got = e.snapshot_batch(us, opts)
        assert e.stats().calls - s0 >= 3, "the batch was not chunked"
    assert got == ref
    # and the unchunked reference is right: the option-1 documents give the no-GC vectors
    assert all(ref[k] == (0, nrows[k % len(base)][1]) for k in range(len(us)) if opts[k])
    assert sum(ref[k] != (0, nrows[k % len(base)][1]) for k in range(len(us)) if not opts[k]) > len(us) // 3

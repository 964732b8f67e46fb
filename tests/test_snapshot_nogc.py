"""Snapshots of documents created with gc: false (yDocOptions, packages/server/src/types.ts:152-154, per document
through onCreateDocument, Hocuspocus.ts:331-344):

    snapshot(u) = Y.encodeStateAsUpdate(Y.applyUpdate(new Y.Doc({gc: false}), u))

tryGcDeleteSet does not run, so a deleted Item keeps its content and a deleted type keeps its children as deleted
Items; everything else (integration, the delete set, the merge pass) is as in test_snapshot.py.

The checker is yjs 13.5.16 through tests/golden/snapshot_nogc_v135.json.gz (tools/snap_fixture.py
160:61:60:nogc 120:62:80:textnogc 40:63:60:subnogc 80:64:120:pendingnogc 24:11:80:nogc 24:21:150:textnogc: the
generator's sessions, snapshotted into a gc: false document; 410 of the 448 expectations differ from the
garbage-collected ones; the last two parts are the first 24 sessions of snapshot_v135 and snapshot_text_v135, so those
updates have both expectations) and step2_nogc_v135.json.gz
(tools/step2_corpus.js nogc).  Here: the fixtures and the kernel code host-compiled (tools/snapdev, flag bit 32 =
snap::F_SNAP_NOGC); the GPU tests are in test_snapshot_nogc_gpu.py / test_step2_nogc_gpu.py."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

from golden import S2FIX, fixtures, nogc_fixtures, step2_nogc_rows, text_fixtures
from twins import BUNDLE, NODE, NOGC, ROOT, _kernel_outputs, _parts_reply, _resolve_pending, build_twin, read_in, read_res, run_snaptext, write_in

# the fixture's parts: (first row, rows, seed, maxOps, mode)
PARTS = ((0, 160, 61, 60, "nogc"), (160, 120, 62, 80, "textnogc"), (280, 40, 63, 60, "subnogc"), (320, 80, 64, 120, "pendingnogc"),
         (400, 24, 11, 80, "nogc"), (424, 24, 21, 150, "textnogc"))


def test_nogc_fixtures_present():
    rows = nogc_fixtures()
    assert len(rows) == 448 and all(u and e for u, e in rows)
    r = step2_nogc_rows()
    assert len(r) == 1406
    assert sum(1 for *_, e, _eq in r if e is None) == 26      # 13.5's writeString throws on a cut surrogate pair
    assert sum(eq for *_, eq in r) == 1140                    # rows where plain diffUpdate(snapshot, sv) is the reply


@pytest.mark.skipif(not (NODE and BUNDLE), reason="node + the yjs bundle are needed to regenerate")
def test_nogc_fixtures_regenerate(tmp_path):
    """The committed vectors are what the generator's no-GC modes produce from the bundle (first sessions of each part)."""
    rows = nogc_fixtures()
    for r0, _n, seed, ops, mode in PARTS:
        a, b = str(tmp_path / "in.bin"), str(tmp_path / "exp.bin")
        subprocess.run([NODE, os.path.join(ROOT, "tools", "snap_corpus.js"), "15", str(seed), a, b, str(ops), mode], check=True, timeout=120,
                       capture_output=True)
        part = rows[r0:r0 + 15]
        assert read_in(a) == [u for u, _ in part], mode
        assert [e for _, e in read_res(b)] == [e for _, e in part], mode


@pytest.mark.skipif(not (NODE and BUNDLE), reason="node + the yjs bundle are needed to regenerate")
def test_nogc_modes_keep_the_sessions(tmp_path):
    """A no-GC mode replays the sessions of its base mode: the same updates, another expectation."""
    a, b, c, d = (str(tmp_path / x) for x in ("a.bin", "b.bin", "c.bin", "d.bin"))
    for base, mode in (("", "nogc"), ("text", "textnogc"), ("subdoc", "subnogc"), ("pending", "pendingnogc")):
        subprocess.run([NODE, os.path.join(ROOT, "tools", "snap_corpus.js"), "12", "7", a, b, "60"] + ([base] if base else []), check=True, timeout=120)
        subprocess.run([NODE, os.path.join(ROOT, "tools", "snap_corpus.js"), "12", "7", c, d, "60", mode], check=True, timeout=120, capture_output=True)
        assert read_in(a) == read_in(c), mode


@pytest.mark.skipif(not (NODE and BUNDLE), reason="node + the yjs bundle (image) needed")
def test_step2_nogc_fixtures_regenerate(tmp_path):
    out = str(tmp_path / "s2.json.gz")
    subprocess.run([NODE, os.path.join(ROOT, "tools", "step2_corpus.js"), out, "nogc"], check=True, timeout=600, capture_output=True)
    assert json.load(gzip.open(out, "rt"))["rows"] == json.load(gzip.open(S2FIX, "rt"))["rows"]


def test_shared_parts_have_both_expectations():
    """The last two parts replay the first sessions of the garbage-collected corpora: same updates, other bytes."""
    rows = nogc_fixtures()
    for r0, src in ((400, fixtures()), (424, text_fixtures())):
        assert [u for u, _ in rows[r0:r0 + 24]] == [u for u, _ in src[:24]]
        assert sum(a[1] != b[1] for a, b in zip(rows[r0:r0 + 24], src[:24])) >= 20


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
@pytest.mark.parametrize("mode", [1, 0])
def test_nogc_kernel_code_on_host(tmp_path, mode):
    """ygm_snapshot.hpp host-compiled with the no-GC bit against every row (13.5 mode; 13.6 default: the expected delete
    set rewritten client-descending); pending rows' three updates merged by the oracle, as the engine's merge does."""
    from golden import ds_to_desc
    exe = build_twin(tmp_path, "snapdev")
    rows = nogc_fixtures()
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_in(a, [u for u, _ in rows])
    subprocess.run([exe, a, b, str(mode | NOGC)], check=True, timeout=120)
    got = read_res(b)
    assert sum(st == 64 for st, _ in got) >= 40   # the pendingnogc part
    exp = [(0, e) if mode else (0, bytes.fromhex(ds_to_desc(e.hex()))) for _, e in rows]
    res = [_resolve_pending(st, body, bool(mode)) for st, body in got]
    bad = [k for k in range(len(rows)) if res[k] != exp[k]]
    assert not bad, f"{len(bad)} documents differ, first {bad[:5]}"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
@pytest.mark.parametrize("mode", [1, 0])
def test_nogc_text_kernel_code_on_host(tmp_path, mode):
    """ygm_snap_text.hpp host-compiled with the no-GC bit: every document it takes equals yjs and the general code, and
    it takes the flat-text part (the envelope does not depend on GC: at least 90 % of the textnogc rows at 6 KiB)."""
    from golden import ds_to_desc
    exe = build_twin(tmp_path, "snaptext")
    rows = nogc_fixtures()
    taken, eq, got = run_snaptext(exe, tmp_path, [u for u, _ in rows], mode | NOGC, 6144)
    text = range(PARTS[1][0], PARTS[1][0] + PARTS[1][1])
    n_text = sum(k in text for k in taken)
    assert n_text >= (9 * len(text) + 9) // 10, f"the flat-text twin took {n_text} of {len(text)} textnogc rows"
    assert all(eq[k] == 1 for k in taken), "text path differs from the general kernel code"
    for k in taken:
        exp = rows[k][1] if mode else bytes.fromhex(ds_to_desc(rows[k][1].hex()))
        assert got[k] == (0, exp), f"document {k} differs from yjs"


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_without_the_flag_the_twins_collect(tmp_path):
    """Without the bit nothing changes: a sample of the garbage-collected vectors through both twins."""
    sd, stx = build_twin(tmp_path, "snapdev"), build_twin(tmp_path, "snaptext")
    rows = fixtures()[:60] + text_fixtures()[:60]
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_in(a, [u for u, _ in rows])
    subprocess.run([sd, a, b, "1"], check=True, timeout=120)
    assert read_res(b) == [(0, e) for _, e in rows]
    taken, eq, got = run_snaptext(stx, tmp_path, [u for u, _ in rows], 1, 6144)
    assert len(taken) >= 50 and all(eq[k] == 1 for k in taken)
    assert all(got[k] == (0, rows[k][1]) for k in taken)
    # the no-GC inputs, collected, are other bytes for a clear majority (the generator counted 410 of 448)
    nrows = nogc_fixtures()
    write_in(a, [u for u, _ in nrows])
    subprocess.run([sd, a, b, "1"], check=True, timeout=120)
    res = read_res(b)
    assert sum(st == 0 and r != e for (st, r), (_, e) in zip(res, nrows)) > len(nrows) // 2


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
@pytest.mark.parametrize("mode", [1, 0])
def test_step2_nogc_decomposition_on_host(tmp_path, mode):
    """The engine's SyncStep2 steps with the kernel code host-compiled (no-GC bit) and the oracle's diff / merge: the
    no-GC snapshot diffed keeping the parentSub bit -- a pending state's three parts diffed and merged -- is yjs's reply
    on every row (13.5), and the client-descending rewrite of it in the default mode."""
    from golden import ds_to_desc
    r = step2_nogc_rows()
    uniq = list(dict.fromkeys(u for u, *_ in r))
    outs = dict(zip(uniq, _kernel_outputs(tmp_path, uniq, mode | NOGC)))
    assert sum(st == 64 for st, _ in outs.values()) >= 40
    bad = []
    for k, (u, sv, exp, _eq) in enumerate(r):
        got = _parts_reply(outs[u][1], outs[u][0], sv, bool(mode))
        if exp is None:
            if mode and got[0] != 4:
                bad.append(k)
        elif got != (0, exp if mode else bytes.fromhex(ds_to_desc(exp.hex()))):
            bad.append(k)
    assert not bad, f"{len(bad)} rows differ, first {bad[:5]}"


def test_sharded_engine_routes_options_with_their_documents():
    """ShardedEngine.snapshot_batch / sync_step2_batch: each shard gets its documents' options, results in caller order."""
    from hocuspocus_amd.shard import ShardedEngine, shard_of

    class Double:
        def __init__(self):
            self.calls = []

        def snapshot_batch(self, updates, opts=None):
            self.calls.append(("snapshot", list(updates), None if opts is None else list(opts)))
            return [(0, u + bytes([0 if opts is None else int(o)])) for u, o in zip(updates, opts or [0] * len(updates))]

        def sync_step2_batch(self, states, svs, opts=None):
            self.calls.append(("step2", list(states), None if opts is None else list(opts)))
            return [(0, s + v + bytes([int(o)])) for s, v, o in zip(states, svs, opts)]

    names = [f"doc-{k}" for k in range(12)]
    ups = [bytes([k]) for k in range(12)]
    opts = bytes(k % 3 == 0 for k in range(12))
    se = ShardedEngine(engines=[Double(), Double()])
    try:
        assert se.snapshot_batch(names, ups, opts) == [(0, ups[k] + bytes([opts[k]])) for k in range(12)]
        assert se.sync_step2_batch(names, ups, ups, list(opts)) == [(0, ups[k] * 2 + bytes([opts[k]])) for k in range(12)]
        assert se.snapshot_batch(names, ups) == [(0, u + b"\0") for u in ups]
        for s, e in enumerate(se.engines):
            mine = [k for k in range(12) if shard_of(names[k], 2) == s]
            assert mine and e.calls[0] == ("snapshot", [ups[k] for k in mine], [opts[k] for k in mine])
            assert e.calls[1] == ("step2", [ups[k] for k in mine], [opts[k] for k in mine])
            assert e.calls[2] == ("snapshot", [ups[k] for k in mine], None)
    finally:
        se.close()

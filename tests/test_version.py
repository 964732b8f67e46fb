"""Version history on the host: Y.encodeSnapshot(Y.snapshot(doc)) (take) and Y.createDocFromSnapshot (restore) as

    restore(state, version) = snapshot( cut(S, version.sv) ++ version.ds ),   S = the no-GC snapshot of the state

with the device code host-compiled (tools/snapdev/versiondev.cpp: ygm_version.hpp's cut between ygm_snapshot.hpp's
passes, the steps of ygm_version_restore_v1 in order) against yjs 13.5.16 through tests/golden/version_v135.json.gz
(tools/version_corpus.js: general, text, pending, subdoc, crafted, edge and align families; "throws" where yjs throws).
The GPU tests are in test_version_gpu.py."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

from golden import REFUSALS, VFIX, _sv, expected, version_rows, version_to_desc
from twins import BUNDLE, NODE, ROOT, _resolve_pending, run_twin

FAMILIES = ("general", "text", "pending", "subdoc", "crafted", "edge", "align")


def test_version_fixtures_present():
    rows = version_rows()
    fam = {f: [r for r in rows if r["family"] == f] for f in FAMILIES}
    assert all(len(v) >= 30 for v in fam.values()), {f: len(v) for f, v in fam.items()}
    assert os.path.getsize(VFIX) <= 800 * 1024
    assert sum(r["restored"] is None for r in fam["crafted"]) >= 5          # a clock above the state's: yjs throws
    assert all((r["restored"] is None) == (r["restored_nogc"] is None) for r in rows)
    assert sum(r["restored"] != r["restored_nogc"] for r in rows if r["restored"] is not None) >= 100
    notes = " | ".join(r["note"] for r in fam["edge"])
    for want in ("struct boundary", "clock 1", "surrogate pair", "ContentAny", "ContentJSON", "ContentDeleted", "straddled GC", "clock 0",
                 "every client absent", "equal to the state", "200 bytes cut to 100", "130 structs cut to 5", "empty document",
                 "1 clients", "2 clients", "63 clients", "64 clients", "65 clients", "300 clients"):
        assert want in notes, want


@pytest.mark.skipif(not (NODE and BUNDLE) or shutil.which("g++") is None, reason="node, the yjs bundle and g++ are needed to regenerate")
def test_version_fixtures_regenerate(tmp_path):
    """The committed vectors are what the seeded generator produces from the bundle; it checks its own requirements (90 %
    of the non-edge rows differ from the plain snapshot, no answered row refused by the host twin) and prints them."""
    out = str(tmp_path / "v.json.gz")
    r = subprocess.run([NODE, os.path.join(ROOT, "tools", "version_corpus.js"), out, "1"], check=True, timeout=300, capture_output=True, text=True)
    assert json.load(gzip.open(out, "rt"))["rows"] == json.load(gzip.open(VFIX, "rt"))["rows"]
    fam = json.loads(r.stdout.splitlines()[0])
    assert set(fam) == set(FAMILIES)
    for f in FAMILIES[:5]:
        assert fam[f]["differ_from_snapshot"] * 10 >= (fam[f]["rows"] - fam[f]["throws"]) * 9, (f, fam[f])


def test_version_to_desc_helper():
    v = bytes.fromhex("02 03 01 00 02 09 02 01 01 05 01 02 03 06 09 03".replace(" ", ""))
    assert version_to_desc(v) == bytes.fromhex("02 09 02 01 01 05 01 03 01 00 02 02 09 03 03 06".replace(" ", ""))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
@pytest.mark.parametrize("mode", [1, 0])
def test_version_kernel_code_on_host(tmp_path, mode):
    """Every row: take, restored and restored_nogc are yjs's bytes (13.5 mode), and their client-descending rewrite in
    the default mode; a row yjs throws on is refused; pending results merged by the oracle, as the engine's merge does."""
    rows = version_rows()
    got = run_twin(tmp_path, [(r["state"], r["version"]) for r in rows], mode)
    bad, pend = [], 0
    for k, (r, (take, _cut, res, resn)) in enumerate(zip(rows, got)):
        if take != (0, expected(r, "take", mode)):
            bad.append((k, "take"))
        for key, g in (("restored", res), ("restored_nogc", resn)):
            e = expected(r, key, mode)
            pend += g[0] == 64
            if e is None:
                if g[0] in (0, 64):
                    bad.append((k, key + " not refused"))
            elif _resolve_pending(g[0], g[1], bool(mode)) != (0, e):
                bad.append((k, key))
    assert not bad, f"{len(bad)} results differ, first {bad[:6]}"
    assert pend >= 10   # versions that are not causally closed, ranges past the kept clocks


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_version_throwing_rows_are_einval(tmp_path):
    """A clock above the state's (the crafted family's throwing rows): the cut's YGM_EINVAL, as the header documents."""
    rows = [r for r in version_rows() if r["restored"] is None]
    got = run_twin(tmp_path, [(r["state"], r["version"]) for r in rows], 1)
    assert rows and all(cut[0] == 8 and res[0] == 8 and resn[0] == 8 for _t, cut, res, resn in got)


def _state7():
    rows = [r for r in version_rows() if r["note"] == "cut at a struct boundary"]
    return rows[0]["state"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_version_refusals_on_host(tmp_path):
    """Each row of the header's refusal table, with hand-built versions; good rows beside them are unaffected; bytes
    after the state vector are ignored; exactly 4096 entries are accepted."""
    st = _state7()
    good = _sv([(7, 3)])
    pairs = [(st, good)] + [(st, mk()) for _n, mk, _s in REFUSALS] + [(st, good + b"\x99\x01"), (st, _sv([(7, 3)] + [(1000 + i, 0) for i in range(4095)]))]
    got = run_twin(tmp_path, pairs, 1)
    ref = got[0]
    assert ref[1][0] == 0 and ref[2][0] == 0 and ref[2][1]
    for (name, _mk, want), g in zip(REFUSALS, got[1:]):
        assert g[0] == ref[0], name            # take does not read the version
        assert (g[1][0], g[2][0], g[3][0]) == (want, want, want), (name, g[1][0], g[2][0])
    assert got[-2][1:] == ref[1:] and got[-1][2:] == ref[2:]


def test_engine_binding_surface():
    """The ctypes binding declares the four entry points (the header's symbols are checked by test_abi.py)."""
    import hocuspocus_amd.engine as E
    for name in ("take_version_batch", "restore_version_batch", "version_take_device", "version_restore_device"):
        assert callable(getattr(E.Engine, name)), name

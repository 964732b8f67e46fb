"""Many versions restored from one stored state (ygm_version_restore_shared_v1 and its device-resident form): the
boundary -- include/ygm.h declares the two entry points, the built library exports them, the ctypes binding lists
them, a null context is refused before any device work -- and the fixture tests/golden/version_history_v135.json.gz
(tools/version_history_corpus.js: documents with one state and a timeline of versions, yjs 13.5.16's restored bytes or
"throws" per version), checked pair by pair on the host twin of the device code (tools/snapdev/versiondev.cpp).  No
compute calls: runs without a GPU.  The GPU tests are in test_version_shared_gpu.py."""
import ctypes
import gzip
import json
import os
import re
import shutil
import subprocess

import pytest

from golden import HFIX, expected, history_docs
from twins import BUNDLE, NODE, ROOT, _resolve_pending, run_twin

import hocuspocus_amd.engine as eng

FAMILIES = ("text", "clients", "many", "pending", "crafted", "empty", "large")
NEW = ("ygm_version_restore_shared_v1", "ygm_version_restore_shared_v1_device")


def header():
    src = open(os.path.join(ROOT, "include", "ygm.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _args(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header())
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_shared_restore():
    assert _args(NEW[0]) == ["ygm_ctx *ctx", "const uint8_t *states", "const uint64_t *state_off", "uint32_t n_states",
                             "const uint8_t *versions", "const uint64_t *version_off", "const uint32_t *ask_state",
                             "const uint8_t *restored_opt", "uint32_t n_asks", "ygm_result *out"]
    assert _args(NEW[1]) == ["ygm_ctx *ctx", "const uint8_t *d_states", "uint64_t states_bytes", "const uint64_t *d_state_off",
                             "uint32_t n_states", "const uint8_t *d_versions", "const uint64_t *d_version_off",
                             "const uint32_t *d_ask_state", "const uint8_t *d_restored_opt", "uint32_t n_asks", "void *stream",
                             "ygm_device_result *out"]
    assert "no form that restores many versions" not in open(os.path.join(ROOT, "include", "ygm.h")).read()


def test_library_exports_the_shared_restore():
    L = ctypes.CDLL(eng.LIB_PATH)
    for f in NEW:
        assert hasattr(L, f), f


def test_binding_lists_the_shared_restore():
    for f in NEW:
        assert f in eng.EXPORTS, f
    for name in ("restore_version_shared_batch", "version_restore_shared_device"):
        assert callable(getattr(eng.Engine, name)), name


def test_null_context_is_einval():
    L = eng.lib()
    off = (ctypes.c_uint64 * 2)(0, 2)
    v_off = (ctypes.c_uint64 * 2)(0, 2)
    ask = (ctypes.c_uint32 * 1)(0)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    res = eng._Result()
    assert L.ygm_version_restore_shared_v1(None, b"\x00\x00", vp(off), 1, b"\x00\x00", vp(v_off), vp(ask), None, 1, ctypes.byref(res)) == eng.EINVAL
    dres = eng._DevResult()
    assert L.ygm_version_restore_shared_v1_device(None, None, 0, None, 0, None, None, None, None, 0, None, ctypes.byref(dres)) == eng.EINVAL


def test_history_fixture_present():
    docs = history_docs()
    assert os.path.getsize(HFIX) <= 400 * 1024
    fam = {f: [d for d in docs if d["family"] == f] for f in FAMILIES}
    assert all(fam.values()), {f: len(v) for f, v in fam.items()}
    assert len(fam["text"][0]["versions"]) >= 40
    assert len(fam["clients"]) >= 3
    assert any(len(d["versions"]) >= 5 for d in fam["many"])
    for d in fam["crafted"]:
        notes = [v["note"] for v in d["versions"]]
        assert "good" in notes and "ahead of the state" in notes and "from a different document" in notes
        assert all((v["restored"] is None) == (v["note"] != "good") for v in d["versions"])   # yjs throws on the other two
    assert [(d["state"], len(d["versions"])) for d in fam["empty"]] == [(b"\x00\x00", 1)]
    assert 280 * 1024 < len(fam["large"][0]["state"]) < 320 * 1024 and len(fam["large"][0]["versions"]) >= 5
    assert all((v["restored"] is None) == (v["restored_nogc"] is None) for d in docs for v in d["versions"])
    # the 300-client document: its state vector has 300 entries (one byte of count 0xAC 0x02 would follow the delete set)
    assert len(fam["many"][0]["state"]) > 3000


@pytest.mark.skipif(not (NODE and BUNDLE), reason="node and the yjs bundle are needed to regenerate")
def test_history_fixture_regenerates(tmp_path):
    """The committed documents are what the seeded generator produces from the bundle; it checks its own requirements
    (90 % of the answered versions differ from the plain snapshot, the size cap) and prints the family counts."""
    out = str(tmp_path / "h.json.gz")
    r = subprocess.run([NODE, os.path.join(ROOT, "tools", "version_history_corpus.js"), out, "1"], check=True, timeout=300, capture_output=True,
                       text=True)
    assert json.load(gzip.open(out, "rt"))["docs"] == json.load(gzip.open(HFIX, "rt"))["docs"]
    fam = json.loads(r.stdout.splitlines()[0])
    assert set(fam) == set(FAMILIES)
    answered = sum(f["versions"] - f["throws"] for f in fam.values())
    assert sum(f["differ_from_snapshot"] for f in fam.values()) * 10 >= answered * 9


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
@pytest.mark.parametrize("mode", [1, 0])
def test_history_fixture_on_host_twin(tmp_path, mode):
    """Every (state, version) of the fixture through the host twin in pair form: yjs's bytes (13.5 mode) and their
    client-descending rewrite in the default mode; a version yjs throws on is refused.  This validates the fixture, not
    the shared form."""
    docs = history_docs()
    flat = [(d, v) for d in docs for v in d["versions"]]
    got = run_twin(tmp_path, [(d["state"], v["version"]) for d, v in flat], mode)
    bad = []
    for k, ((_d, v), (_take, _cut, res, resn)) in enumerate(zip(flat, got)):
        for key, g in (("restored", res), ("restored_nogc", resn)):
            e = expected(v, key, mode)
            if e is None:
                if g[0] in (0, 64):
                    bad.append((k, key + " not refused"))
            elif _resolve_pending(g[0], g[1], bool(mode)) != (0, e):
                bad.append((k, key))
    assert not bad, f"{len(bad)} results differ, first {bad[:6]}"

"""The shared-state boundary (many state vectors answered from one state): include/ygm.h declares the four entry
points, the built library exports them, the host forms refuse a null context before any device work, and the
ctypes mirror of ygm_stats_t carries the appended docs_snapshot counter.  No compute calls: runs without a GPU."""
import ctypes
import os
import re

from conftest import ROOT

import hocuspocus_amd.engine as eng

SHARED = ("ygm_diff_shared_v1", "ygm_sync_step2_shared_v1", "ygm_diff_shared_v1_device", "ygm_sync_step2_shared_v1_device")


def header():
    src = open(os.path.join(ROOT, "include", "ygm.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_shared_forms():
    src = header()
    for f in SHARED:
        assert re.search(r"\bint\s+%s\s*\(" % f, src), f
        assert f in eng.EXPORTS
    # the host forms: states, n_states, state vectors, ask -> state, n_asks, result
    m = re.search(r"int\s+ygm_sync_step2_shared_v1\s*\(([^)]*)\)", src)
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9 and args[3].startswith("uint32_t") and args[6].startswith("const uint32_t *")
    assert args[7].startswith("uint32_t") and args[8].startswith("ygm_result")


def test_library_exports_the_shared_forms():
    L = ctypes.CDLL(eng.LIB_PATH)
    for f in SHARED:
        assert hasattr(L, f), f


def test_null_context_is_einval():
    L = eng.lib()
    res = eng._Result()
    off = (ctypes.c_uint64 * 2)(0, 2)
    sv_off = (ctypes.c_uint64 * 2)(0, 1)
    ask = (ctypes.c_uint32 * 1)(0)
    state = b"\x00\x00"
    for f in ("ygm_sync_step2_shared_v1", "ygm_diff_shared_v1"):
        st = getattr(L, f)(None, state, ctypes.cast(off, ctypes.c_void_p), 1, b"\x00", ctypes.cast(sv_off, ctypes.c_void_p),
                           ctypes.cast(ask, ctypes.c_void_p), 1, ctypes.byref(res))
        assert st == eng.EINVAL, f
    # the plain forms of the calls that have an options form: the bindings reach them only through that form (with a
    # null option pointer), so they are called here -- a null context returns before any device work
    st_off, sv = ctypes.cast(off, ctypes.c_void_p), ctypes.cast(sv_off, ctypes.c_void_p)
    assert L.ygm_snapshot_v1(None, state, st_off, 1, ctypes.byref(res)) == eng.EINVAL
    assert L.ygm_sync_step2_v1(None, state, st_off, b"\x00", sv, 1, ctypes.byref(res)) == eng.EINVAL
    dres = eng._DevResult()
    assert L.ygm_snapshot_v1_device(None, None, 0, None, 0, None, ctypes.byref(dres)) == eng.EINVAL
    assert L.ygm_sync_step2_v1_device(None, None, 0, None, None, None, 0, None, ctypes.byref(dres)) == eng.EINVAL
    assert L.ygm_sync_step2_shared_v1_device(None, None, 0, None, 0, None, None, None, 0, None, ctypes.byref(dres)) == eng.EINVAL


def test_stats_mirror_ends_with_docs_snapshot():
    assert eng.Stats._fields_[-1] == ("docs_snapshot", ctypes.c_uint64)
    # the C struct: docs_snapshot is its last member, the mirror has one entry per member
    m = re.search(r"typedef struct \{([^}]*)\}\s*ygm_stats_t;", header(), flags=re.S)
    names = [n.strip() for decl in m.group(1).split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names[-1] == "docs_snapshot"
    assert names == [n for n, _ in eng.Stats._fields_]

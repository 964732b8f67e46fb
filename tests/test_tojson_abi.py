"""ygm_tojson_v1 / ygm_tojson_v1_device through the layers, without a GPU: the C header declares them with their three
kinds, the library exports them where it is built, the Python engine and the Node engine bind them with the same
values, the addon has their row, and the call's argument checks (a bad kind, an empty batch) answer before any device
work."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "packages", "extension-gpu-merge")
KINDS = {"MAP": 0, "ARRAY": 1, "TEXT": 2}


def test_header_declares_both_entry_points():
    h = open(os.path.join(ROOT, "include", "ygm.h")).read()
    host = re.search(r"int\s+ygm_tojson_v1\s*\(([^;]*)\);", h)
    dev = re.search(r"int\s+ygm_tojson_v1_device\s*\(([^;]*)\);", h)
    assert host and dev
    assert [a.split()[-1].lstrip("*") for a in host.group(1).split(",")] == ["ctx", "states", "state_off", "names", "name_off", "kind", "n_docs", "out"]
    assert [a.split()[-1].lstrip("*") for a in dev.group(1).split(",")] == ["ctx", "d_states", "states_bytes", "d_state_off", "d_names", "d_name_off",
                                                                           "kind", "n_docs", "stream", "out"]
    flat = " ".join(h.replace("*", " ").split())
    assert "Replaces no single reference interface: the batched form of a custom webhook transformer's `fromYdoc`, extension-webhook/src/index.ts:27-31,119" in flat
    for out_of_scope in ("shortest-round-trip decimal of non-integer doubles", "XML strings of nested Xml types", "toDelta", "multi-root object form"):
        assert out_of_scope in flat, out_of_scope


def test_the_three_kinds_agree_in_header_python_and_node():
    import hocuspocus_amd.engine as eng
    h = open(os.path.join(ROOT, "include", "ygm.h")).read()
    js = open(os.path.join(PKG, "src", "engine.js")).read()
    for name, v in KINDS.items():
        assert int(re.search(r"#define\s+YGM_TOJSON_%s\s+(\d+)u" % name, h).group(1)) == v
        assert getattr(eng, "TOJSON_" + name) == v
        assert int(re.search(r"const TOJSON_%s = (\d+)" % name, js).group(1)) == v
    exports = re.search(r"module\.exports = \{([^}]*)\}", js).group(1)
    assert all("TOJSON_" + name in exports for name in KINDS)
    assert re.search(r"toJson: \{ native: 'toJson', pack: packPair", js)
    addon = open(os.path.join(PKG, "addon", "ygm_napi.c")).read()
    assert '{ "toJson", SHAPE_PAIR, TAIL_U32, run_tojson }' in addon and "ygm_tojson_v1(j->h->ctx" in addon
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    for fn in ("toJsonMany", "sharedJsonOf", "versionSharedJson"):
        assert fn in dts, fn


def test_library_exports_them_where_it_is_built():
    import hocuspocus_amd.engine as eng
    if os.path.exists(eng.LIB_PATH):
        L = ctypes.CDLL(eng.LIB_PATH)
        assert hasattr(L, "ygm_tojson_v1") and hasattr(L, "ygm_tojson_v1_device")
    src = open(os.path.join(ROOT, "hocuspocus_amd", "csrc", "Makefile")).read()
    assert "ygm_tojson.hip" in src


def test_engine_binds_them():
    import hocuspocus_amd.engine as eng
    assert "ygm_tojson_v1" in eng.EXPORTS and "ygm_tojson_v1_device" in eng.EXPORTS
    assert callable(eng.Engine.tojson_batch) and callable(eng.Engine.tojson_device)
    # their signatures, from the table lib() sets every argtypes / restype from (tests/test_abi.py holds it to the header)
    assert eng.SIGNATURES["ygm_tojson_v1"] == (("p", "p", "p", "p", "p", "u32", "u32", "res"), "int")
    assert eng.SIGNATURES["ygm_tojson_v1_device"] == (("p", "p", "u64", "p", "p", "p", "u32", "u32", "p", "dres"), "int")
    order = list(eng.SIGNATURES)
    assert order.index("ygm_tojson_v1") == order.index("ygm_json_fields_v1") + 1
    assert order.index("ygm_tojson_v1_device") == order.index("ygm_json_fields_v1_device") + 1


def test_a_bad_kind_is_einval_and_an_empty_batch_works_before_any_device_work():
    """The host form's argument checks need no context: a kind other than the three is YGM_EINVAL for the call, with
    every other argument valid; so is a missing context, whatever the kind (an empty batch included: nothing to run it
    on).  With a context an empty batch gives an empty result (tests/test_tojson_gpu.py)."""
    import numpy as np
    import hocuspocus_amd.engine as eng
    if not os.path.exists(eng.LIB_PATH):
        pytest.skip("the library is not built")
    L = eng.lib()
    st = bytes.fromhex("0101ad02002801016d01610177036f6e6500")
    off = np.array([0, len(st)], np.uint64)
    noff = np.array([0, 1], np.uint64)
    res = eng._Result()
    ctx = ctypes.c_void_p(1)      # (never dereferenced: the kind is checked first)
    for bad in (3, 4, 0xFFFFFFFF):
        rc = L.ygm_tojson_v1(ctx, ctypes.c_char_p(st), off.ctypes.data_as(ctypes.c_void_p), ctypes.c_char_p(b"m"),
                             noff.ctypes.data_as(ctypes.c_void_p), bad, 1, ctypes.byref(res))
        assert rc == eng.EINVAL
        dres = eng._DevResult()
        assert L.ygm_tojson_v1_device(ctx, None, 0, None, None, None, bad, 0, None, ctypes.byref(dres)) == eng.EINVAL
    for kind in (0, 1, 2):
        assert L.ygm_tojson_v1(None, None, None, None, None, kind, 0, ctypes.byref(res)) == eng.EINVAL
        assert L.ygm_tojson_v1(ctx, None, None, None, None, kind, 0, None) == eng.EINVAL
    with pytest.raises(ValueError):
        eng.Engine.tojson_batch(None, [st], [], 0)

"""ygm_json_v1 / ygm_json_v1_device through the layers, without a GPU: the C header declares them, the library exports
them where it is built, the Python engine binds them."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_both_entry_points():
    h = open(os.path.join(ROOT, "include", "ygm.h")).read()
    assert re.search(r"#define\s+YGM_JSON_PROSEMIRROR\s+0u", h)
    host = re.search(r"int\s+ygm_json_v1\s*\(([^;]*)\);", h)
    dev = re.search(r"int\s+ygm_json_v1_device\s*\(([^;]*)\);", h)
    assert host and dev
    assert [a.split()[-1].lstrip("*") for a in host.group(1).split(",")] == ["ctx", "states", "state_off", "names", "name_off", "kind", "n_docs", "out"]
    assert [a.split()[-1].lstrip("*") for a in dev.group(1).split(",")] == ["ctx", "d_states", "states_bytes", "d_state_off", "d_names", "d_name_off",
                                                                           "kind", "n_docs", "stream", "out"]
    assert "extension-webhook/src/index.ts:119" in h and "transformer/src/Prosemirror.ts:26" in h


def test_library_exports_them_where_it_is_built():
    import hocuspocus_amd.engine as eng
    if os.path.exists(eng.LIB_PATH):
        L = ctypes.CDLL(eng.LIB_PATH)
        assert hasattr(L, "ygm_json_v1") and hasattr(L, "ygm_json_v1_device")
    src = open(os.path.join(ROOT, "hocuspocus_amd", "csrc", "Makefile")).read()
    assert "ygm_json.hip" in src


def test_engine_binds_them():
    import hocuspocus_amd.engine as eng
    assert "ygm_json_v1" in eng.EXPORTS and "ygm_json_v1_device" in eng.EXPORTS
    assert eng.JSON_PROSEMIRROR == 0
    assert callable(eng.Engine.json_batch) and callable(eng.Engine.json_device)
    # their signatures, from the table lib() sets every argtypes / restype from (tests/test_abi.py holds it to the header)
    assert eng.SIGNATURES["ygm_json_v1"] == (("p", "p", "p", "p", "p", "u32", "u32", "res"), "int")
    assert eng.SIGNATURES["ygm_json_v1_device"] == (("p", "p", "u64", "p", "p", "p", "u32", "u32", "p", "dres"), "int")

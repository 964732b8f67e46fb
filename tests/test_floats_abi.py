"""YGM_F_FLOATS through the layers, without a GPU: the C header defines the flag as the one free bit and documents it
beside the three JSON calls without touching a sentence the other ABI tests hold, the Python engine and the Node engine
agree on its value and take it as an option, the launchers pick the kernels' FLOATS instantiations by it, and the
conversion's header stays out of every other kernel."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "packages", "extension-gpu-merge")
CSRC = os.path.join(ROOT, "hocuspocus_amd", "csrc")


def header():
    return open(os.path.join(ROOT, "include", "ygm.h")).read()


def test_header_defines_the_flag_as_the_free_bit():
    h = header()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(YGM_F_\w+)\s+(\d+)u", h)}
    assert flags["YGM_F_FLOATS"] == 8
    assert sorted(flags.values()) == [1, 2, 4, 8, 16, 32, 64]          # every bit once: 8 was the free one
    flat = " ".join(h.replace("*", " ").split())
    assert flat.count("With YGM_F_FLOATS (ygm_open)") == 3              # ygm_json_v1, ygm_json_fields_v1, ygm_tojson_v1
    for still in ("more than 15 significant digits or with an exponent", "BigInt", "Uint8Array", "__proto__", "hashed mark names",
                  "ygm_convert_v2_to_v1 keeps its refusal"):
        assert still in flat, still


def test_every_phrase_the_other_abi_tests_hold_is_still_there():
    h = header()
    flat = " ".join(h.replace("*", " ").split())
    assert "Replaces no single reference interface: the batched form of a custom webhook transformer's `fromYdoc`, extension-webhook/src/index.ts:27-31,119" in flat
    for phrase in ("shortest-round-trip decimal of non-integer doubles", "XML strings of nested Xml types", "toDelta", "multi-root object form",
                   "a finite non-integer number, or an integer above 2^53", "a number in an attribute, mark or embed that is not an integer JSON.stringify writes without an exponent",
                   "(as ygm_convert_v2_to_v1 refuses it)"):
        assert phrase in flat, phrase
    assert "extension-webhook/src/index.ts:119" in h and "transformer/src/Prosemirror.ts:26" in h
    assert "int ygm_open(int device, uint32_t flags, ygm_ctx **out);" in h


def test_python_and_node_agree_on_the_value_and_take_the_option():
    import hocuspocus_amd.engine as eng
    assert eng.F_FLOATS == 8 and (eng.F_COMPAT_135, eng.F_FORCE_SEQ) == (1, 2)
    sig = inspect.signature(eng.Engine.__init__)
    assert list(sig.parameters) == ["self", "device", "compat135", "force_seq", "floats"] and sig.parameters["floats"].default is False
    js = open(os.path.join(PKG, "src", "engine.js")).read()
    m = re.search(r"this\.flags = \(opts\.compat135 \? (\d+) : 0\) \| \(opts\.floats \? (\d+) : 0\)", js)
    assert m and (int(m.group(1)), int(m.group(2))) == (eng.F_COMPAT_135, eng.F_FLOATS)
    idx = open(os.path.join(PKG, "src", "index.js")).read()
    assert "compat135: c.compat135, floats: c.floats," in idx
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    opts = re.search(r"export interface GpuEngineOptions \{(.*?)\n\}", dts, re.S).group(1)
    assert "floats?: boolean" in opts
    assert "export interface GpuMergeConfiguration extends GpuEngineOptions" in dts   # the extension's options carry it


def test_launchers_pick_the_instantiations_by_the_flag():
    v1 = open(os.path.join(CSRC, "ygm_v1.hpp")).read()
    assert re.search(r"constexpr uint32_t F_FLOATS = 8u;", v1)
    tj = open(os.path.join(CSRC, "ygm_tojson.hip")).read()
    pj = open(os.path.join(CSRC, "ygm_json.hip")).read()
    assert "flags & F_FLOATS ? k_tojson<true> : k_tojson<false>" in tj
    assert "flags & F_FLOATS ? (fields ? k_json<true, true> : k_json<false, true>) : (fields ? k_json<true, false> : k_json<false, false>)" in pj
    # no device code reads the bit: the option is compile time alone
    for f in os.listdir(CSRC):
        if f.endswith((".hpp", ".hip", ".cpp")):
            src = open(os.path.join(CSRC, f)).read()
            assert len(re.findall(r"\bF_FLOATS\b", src)) == {"ygm_v1.hpp": 1, "ygm_tojson.hip": 1, "ygm_json.hip": 1}.get(f, 0), f
    # the table is global-memory data, generated; the V2 -> V1 conversion keeps its own form of any_json
    d = open(os.path.join(CSRC, "ygm_dtoa.hpp")).read()
    assert 'static __device__ const uint64_t POW5[K_MAX - K_MIN + 1][2]' in d and '#include "ygm_dtoa_pow5.inc"' in d
    v2 = open(os.path.join(CSRC, "ygm_v2.hpp")).read()
    assert "template <class O, bool TOJSON = false, bool FLOATS = false>" in v2
    assert "int e = any_json(q, m);" in v2 and "return any_json(q2, o);" in v2


def test_host_tools_take_the_switch():
    for t in ("jsondev", "jsonfieldsdev", "tojsondev"):
        src = open(os.path.join(ROOT, "tools", "snapdev", t + ".cpp")).read()
        assert '"--floats"' in src and "[--floats]" in src, t
    assert os.path.exists(os.path.join(ROOT, "tools", "snapdev", "dtoadev.cpp"))

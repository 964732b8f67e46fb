"""toJSON of stored Map, Array and Text roots (ygm_tojson_v1), without a GPU: the committed fixture, its regeneration
from the committed tool, and k_tojson's sequential code (ygm_tojson.hpp) host-compiled through
tools/snapdev/tojsondev.cpp against every row of the fixture -- serialized roots and refusals -- with the overflow
protocol's second run, at the workspace's own cap and at a small forced one, and once more under the address and
undefined-behaviour sanitizers."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

import tojson_fixture as tf

ROOT = tf.ROOT
NODE = shutil.which("node")
BUNDLE = os.path.exists("/opt/conda/share/jupyter/lab/static/3502.fbe0c610be82ba1360db.js")
ESC = '"q\\" b\\\\ \\b\\f\\n\\r\\t \\u0001\\u001f \x7f \u2028 \U0001F600'      # the escape string, as written (without its closing quote)
BIG = "a 4 KB string of 0x01 bytes in a Map"


def js(note, i=0):
    st, name, kind, b, status = tf.edge(note, i)
    assert status == 0, note
    return b.decode()


def status(note, i=0):
    return tf.edge(note, i)[4]


def test_fixture_present_made_from_the_committed_inputs_with_pinned_counts():
    fix = tf.load()
    assert set(fix["inputs"]) == {s + ".json.gz" for s in tf.SETS}
    for name, sha in fix["inputs"].items():
        assert tf.input_sha256(name) == sha, name
    assert fix["inputs"]["snapshot_v135.json.gz"] == "c05ad5084753138c517a7305184e5526f6dca310163cd0ab76802d8b212ac957"
    assert fix["inputs"]["snapshot_nogc_v135.json.gz"] == "d3b2e39a7c4b44cde834d9d2b57ec989f354066112833206a93c285cc8cfc0fb"
    got = {}
    trivial = (b"{}".hex(), b"[]".hex(), b'""'.hex())
    for s in tf.SETS:
        assert len(fix["sets"][s]) == len(tf.set_states(s))
        rows = [r for asks in fix["sets"][s] for r in asks]
        got[s] = (len(rows), sum(r[2] == 0 for r in rows), sum(r[2] != 0 for r in rows))
        assert (fix["counts"][s]["asks"], fix["counts"][s]["ok"], fix["counts"][s]["refused"]) == got[s]
        for asks in fix["sets"][s]:
            assert len(asks) % 3 == 0 and [r[1] for r in asks] == [0, 1, 2] * (len(asks) // 3)      # every root as each kind
            assert [r[0] for r in asks[-3:]] == [fix["absent"]] * 3 and [r[2] for r in asks[-3:]] == [0, 0, 0]
        assert all(len(r) == 4 for asks in fix["sets"][s][:fix["full"]] for r in asks)
        assert all(len(r) == 5 for asks in fix["sets"][s][fix["full"]:] for r in asks)
        full = [r for asks in fix["sets"][s][:fix["full"]] for r in asks if r[2] == 0]
        assert sum(r[3] in trivial for r in full) > len(full) // 2       # mostly {}, [] or ""
    assert got == {"snapshot_v135": (6321, 5498, 823), "snapshot_text_v135": (1917, 1598, 319), "snapshot_pending_v135": (3558, 3117, 441),
                   "snapshot_subdoc_v135": (5031, 4172, 859), "snapshot_nogc_v135": (5304, 4573, 731)}
    # every refusal in the sets is YGM_EUNSUPPORTED: a fragment's elements asked as an Array, a Text's strings asked as one
    assert {r[2] for s in tf.SETS for asks in fix["sets"][s] for r in asks} == {0, 9}
    full_absent = [asks[-3:] for s in tf.SETS for asks in fix["sets"][s][:fix["full"]]]
    assert full_absent and all([bytes.fromhex(r[3]) for r in a] == [b"{}", b"[]", b'""'] for a in full_absent)
    # the seeded random sessions: each root asked with its own kind; >= 90 % serialized, at least half of those > 64 bytes
    rnd = [r for e in fix["random"] for r in e["asks"]]
    ok = [r for r in rnd if r[2] == 0]
    assert all([(bytes.fromhex(r[0]), r[1]) for r in e["asks"]] == [(b"m", 0), (b"a", 1), (b"t", 2)] for e in fix["random"])
    assert (len(fix["random"]), len(rnd), len(ok), sum(len(r[3]) // 2 > 64 for r in ok)) == (160, 480, 465, 321)
    assert len(ok) * 10 >= len(rnd) * 9 and 321 * 2 >= len(ok) and {r[2] for r in rnd} == {0, 3}
    assert fix["counts"]["random"] == {"sessions": 160, "asks": 480, "ok": 465, "over64": 321}
    assert len({e["state"] for e in fix["random"]}) == 160
    assert len(fix["edges"]) >= 32 and sum(len(e["asks"]) for e in fix["edges"]) >= 47
    assert os.path.getsize(tf.FIX) <= max(os.path.getsize(os.path.join(tf.GOLDEN, f)) for f in os.listdir(tf.GOLDEN) if f != "tojson_v135.json.gz"
                                          and os.path.isfile(os.path.join(tf.GOLDEN, f)))
    assert os.path.getsize(tf.FIX) < (1 << 20)


def test_edge_sessions_say_what_they_are_named_for():
    assert [js("an empty root, as each kind", i) for i in range(3)] == ["{}", "[]", '""']
    assert [js("an absent root, as each kind", i) for i in range(3)] == ["{}", "[]", '""']
    assert js('keys "10", "9", "a", "04" set in that order') == '{"9":"v9","10":"v10","a":"va","04":"v04"}'
    assert js("a key set twice") == '{"a":"three","b":"two"}'
    assert js("a key set then deleted, alone") == "{}"
    assert js("a key set then deleted beside a live one") == '{"b":"two"}'
    assert js("two clients setting one key concurrently") == '{"k":"from-b","only-b":1,"first":"f"}'
    assert js("a value undefined in a Map") == '{"a":1,"b":2}'
    assert js("undefined inside an Any object and an Any array") == '{"o":{"y":[null,1]}}'
    assert js("undefined inside an Any object and an Any array", 1) == "[[null],{}]"
    assert js("an undefined Array element and ContentJSON elements") == '[null,1,{"a":1},null,7]'
    assert js("an undefined Array element and ContentJSON elements", 1) == '{"k":"v"}'       # (key u: undefined, dropped)
    kinds = js("values of every kind")
    assert kinds == ('{"s":' + ESC + '","n":-42,"nz":0,"t":true,"f":false,"z":null,"o":{"2":"index","k":[1,"two",{"deep":null}],"e":{}},'
                     '"arr":[[],{},0]}')
    assert json.loads(kinds)["s"] == 'q" b\\ \b\f\n\r\t \u0001\u001f \u007f \u2028 \U0001F600'
    assert js("values of every kind", 1) == '[' + ESC + '",-42,0,true,false,null,{"2":"index","k":[1,"two",{"deep":null}],"e":{}},[[],{},0]]'
    assert js("numbers 1700000000000, 4294967296, 2^53, Infinity, NaN") == (
        '{"now":1700000000000,"u32":4294967296,"big":9007199254740992,"inf":null,"ninf":null,"nan":null,"in":{"at":[1700000000001,null]}}')
    assert js("numbers 1700000000000, 4294967296, 2^53, Infinity, NaN", 1) == "[1700000000000,4294967296,9007199254740992,null,null]"
    assert js("Array items of several elements with a deleted run in the middle") == '[0,1,2,{"seven":7},[8]]'
    deep = js("Map in Array in Map, 40 deep")
    assert deep.startswith('{"k0":["before1",{"k2":["before3",{"k4":') and deep.count("[") == 20 and deep.count("{") == 21
    assert '{"bottom":"here"}' in deep and deep.endswith('"beside6":6}]}]}],"beside0":0}')
    assert js("a nested Text with formats, an embed and a deleted middle") == '{"t":"plain bold tail"}'
    assert js("a nested Text with formats, an embed and a deleted middle", 1) == '["in \\"array\\"\\n","next"]'
    assert js("a Text cut through a surrogate pair") == '"a�X�btail"'
    assert js("a Text root with every escape class") == ESC + ' end"'
    mixed = "a root holding both map entries and list items, asked as each kind"
    assert (js(mixed, 0), status(mixed, 1), js(mixed, 2)) == ('{"attr":{"v":1}}', 9, '"text"')
    assert js("a state with pending structs") == '{"from-b":{"n":2},"shared":"start","from-a":1}'
    assert js("a state with pending structs", 1) == '["one","two"]'                              # (not "after-the-gap")
    st, _, _, big, _ = tf.edge(BIG)
    assert big == b'{"ctl":"' + b"\\u0001" * 4096 + b'"}' and len(big) > 5 * len(st)
    statuses = {(e["note"], i): r[2] for e in tf.load()["edges"] if e["note"].startswith("refused: ") for i, r in enumerate(e["asks"])}
    assert sorted(statuses.values()) == [1] + [3] * 3 + [9] * 11, statuses
    for note, want in (("a nested XmlElement", 9), ("a ContentBinary in an Array", 9), ("a Uint8Array inside an Any", 9), ("a ContentDoc", 9),
                       ("a live ContentString in an Array's list", 9), ("a live ContentEmbed in an Array's list", 9),
                       ("a live Map entry that is a ContentBinary", 9), ("a Y.Map key __proto__ with a live entry", 9),
                       ("a finite non-integer number", 3), ("an integer above 2^53", 3), ("a BigInt", 1)):
        assert statuses[("refused: " + note, 0)] == want, note
    assert [statuses[("refused: a nested XmlFragment, XmlHook and XmlText in an Array", i)] for i in range(3)] == [9, 9, 9]
    for e in tf.load()["edges"] + tf.load()["random"]:
        for r in e["asks"]:
            if r[2] == 0:
                json.loads(bytes.fromhex(r[3]))      # every recorded JSON parses
            else:
                assert r[3] == ""


@pytest.mark.skipif(not (NODE and BUNDLE), reason="node + the yjs bundle are needed to regenerate")
def test_fixture_regenerates(tmp_path):
    """The first 20 states of every set, the random sessions and the edge sessions are what the committed tool makes
    from the bundle."""
    out = str(tmp_path / "j.json.gz")
    subprocess.run([NODE, os.path.join(ROOT, "tools", "tojson_corpus.js"), out, "20"], check=True, timeout=120, stdout=subprocess.DEVNULL)
    got = json.load(gzip.open(out, "rt"))
    fix = tf.load()
    assert got["inputs"] == fix["inputs"] and got["absent"] == fix["absent"] and got["full"] == fix["full"]
    for s in tf.SETS:
        assert got["sets"][s] == fix["sets"][s][:20], s
    assert got["random"] == fix["random"]
    assert got["edges"] == fix["edges"]


def build(tmp_path_factory, name, flags):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", *flags, "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "snapdev", "tojsondev.cpp")], check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def tojsondev(tmp_path_factory):
    return build(tmp_path_factory, "tojsondev", ["-O1"])


def run_rows(exe, tmp_path, rows, flags, cap):
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    tf.write_asks(a, [(r[1], r[2], r[3]) for r in rows])
    subprocess.run([exe, a, b, flags, str(cap)], check=True, timeout=900)
    got = tf.read_tojsondev(b)
    assert len(got) == len(rows)
    bad = [(r[0], r[2], r[3], r[4], g[0], g[2][:60]) for r, g in zip(rows, got) if not tf.matches(r, g[0], g[2])]
    assert not bad, (len(bad), bad[:5])
    return got


@pytest.mark.parametrize("flags", ["1", "0"])
def test_kernel_code_on_host_vs_every_row(tojsondev, tmp_path, flags):
    """The twin gives the fixture's status and bytes for every row, refusals included, with either flags value; only
    the 4 KB control string takes the second run, and comes out of it with the recorded bytes."""
    rows = tf.expectations()
    got = run_rows(tojsondev, tmp_path, rows, flags, 0)
    assert len(rows) == 22131 + 480 + sum(len(e["asks"]) for e in tf.load()["edges"])
    assert [r[0] for r, g in zip(rows, got) if g[1]] == [BIG]


def test_forced_small_cap_reruns_every_longer_json(tojsondev, tmp_path):
    """With the first run's region cut to 48 bytes, every JSON longer than that takes the overflow protocol's second
    run -- into a region of exactly its recorded length -- and every row still comes out as recorded."""
    rows = tf.expectations()
    got = run_rows(tojsondev, tmp_path, rows, "1", 48)
    reran = [bool(g[1]) for g in got]
    assert reran == [r[4] == 0 and r[7] > 48 for r in rows] and sum(reran) > 1000


def test_sanitizer_build_over_the_fixture(tmp_path_factory, tmp_path):
    """The harness as the stand-alone program it is, built with -fsanitize=address,undefined and run once over every
    row (the walk's bounds: its stack frames, the piece cursors, the exact-size output regions), then over the edge and
    random sessions with the forced cap."""
    exe = build(tmp_path_factory, "tojsondev_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    run_rows(exe, tmp_path, tf.expectations(), "1", 0)
    run_rows(exe, tmp_path, tf.expectations(sets=()), "0", 48)

"""Stored documents as ProseMirror JSON (ygm_json_v1), without a GPU: the committed fixture, its regeneration from the
committed tool, and k_json's sequential code (ygm_json.hpp) host-compiled through tools/snapdev/jsondev.cpp against
every row of the fixture -- serialized roots and refusals -- with the overflow protocol's second run."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

import json_fixture as jf

ROOT = jf.ROOT
NODE = shutil.which("node")
BUNDLE = os.path.exists("/opt/conda/share/jupyter/lab/static/3502.fbe0c610be82ba1360db.js")
P = '{"type":"doc","content":['      # every document starts so


def js(note):
    st, b, status = jf.edge(note)
    assert status == 0, note
    return b.decode()


def test_fixture_present_made_from_the_committed_inputs_with_pinned_counts():
    fix = jf.load()
    assert set(fix["inputs"]) == {s + ".json.gz" for s in jf.SETS}
    for name, sha in fix["inputs"].items():
        assert jf.input_sha256(name) == sha, name
    got = {}
    for s in jf.SETS:
        assert len(fix["sets"][s]) == len(jf.set_states(s))
        rows = [r for roots in fix["sets"][s] for r in roots[:-1]]      # (the last ask of a state is the absent name)
        got[s] = (len(rows), sum(r[1] == 0 for r in rows), sum(r[1] != 0 for r in rows))
        assert (fix["counts"][s]["roots"], fix["counts"][s]["ok"], fix["counts"][s]["refused"]) == got[s]
        for roots in fix["sets"][s]:
            assert roots[-1][0] == fix["absent"] and roots[-1][1] == 0
        assert all(len(r) == 3 for roots in fix["sets"][s][:fix["full"]] for r in roots)
    assert got == {"snapshot_v135": (1667, 833, 834), "snapshot_text_v135": (319, 0, 319), "snapshot_pending_v135": (866, 429, 437),
                   "snapshot_subdoc_v135": (1417, 784, 633), "snapshot_nogc_v135": (1320, 610, 710)}
    four = [got[s] for s in jf.SETS[:4]]
    assert (sum(g[0] for g in four), sum(g[1] for g in four)) == (4269, 2046)
    assert sum(fix["counts"][s]["marks"] for s in jf.SETS) == 667 and sum(fix["counts"][s]["attrs"] for s in jf.SETS) == 1017
    # every refusal in the sets is a root of another kind asked as a fragment
    assert {r[1] for s in jf.SETS for roots in fix["sets"][s] for r in roots} == {0, 9}
    empty = bytes(P + "]}", "ascii")
    full_absent = [roots[-1] for s in jf.SETS for roots in fix["sets"][s][:fix["full"]]]
    assert full_absent and all(bytes.fromhex(r[2]) == empty for r in full_absent)
    assert len(fix["edges"]) >= 36
    assert os.path.getsize(jf.FIX) <= max(os.path.getsize(os.path.join(jf.GOLDEN, f)) for f in os.listdir(jf.GOLDEN) if f != "json_v135.json.gz"
                                          and os.path.isfile(os.path.join(jf.GOLDEN, f)))


def test_edge_sessions_say_what_they_are_named_for():
    assert js("an empty fragment") == P + "]}"
    assert js("an XmlText directly under the fragment") == (
        P + '[{"type":"text","text":"top"}],{"type":"paragraph","content":[{"type":"text","text":"after"}]},[{"type":"text","text":"again"}]]}')
    assert js("a paragraph without children") == P + '{"type":"paragraph"}]}'
    assert js("a paragraph with an empty XmlText") == P + '{"type":"paragraph","content":[]}]}'
    assert js("a paragraph whose children are all deleted") == P + '{"type":"paragraph"}]}'
    assert "gone" not in js("a deleted subtree between two live ones") and js("a deleted subtree between two live ones").count('"paragraph"') == 2
    deep = js("nesting 40 deep")
    assert deep.count('"content":[') == 41 and '{"type":"n39","content":[{"type":"text","text":"bottom"}]}' in deep
    assert '"type":"n5","attrs":{"depth":5},"content"' in deep
    assert '"attrs":{"a":"three","b":"two"}' in js("attrs: a key set twice")
    assert "attrs" not in js("attrs: a key set then deleted, alone")
    assert '"attrs":{"b":"two"}' in js("attrs: a key set then deleted beside a live one")
    assert '"attrs":{"9":"v9","10":"v10","a":"va","04":"v04"}' in js('attrs: keys "10", "9", "a", "04" set in that order')
    assert '"k":"from-b"' in js("attrs: two clients setting one key concurrently")
    kinds = js("attrs: values of every kind")
    for lit in ('"n":-42', '"t":true', '"z":null', '"o":{"2":"index","k":[1,"two",{"deep":null}],"e":{}}', '"arr":[[],{},0]',
                '"s":"q\\" b\\\\ \\b\\f\\n\\r\\t \\u0001\\u001f \x7f \u2028 \U0001F600"'):
        assert lit in kinds, lit
    assert json.loads(kinds)["content"][0]["attrs"]["s"] == 'q" b\\ \b\f\n\r\t \u0001\u001f \u007f \u2028 \U0001F600'
    statuses = {e["note"]: e["roots"][0][1] for e in jf.load()["edges"] if e["note"].startswith("refused: ")}
    assert sorted(statuses.values()) == [1] + [3] * 3 + [9] * 7, statuses
    assert statuses["refused: a float attribute"] == 3 and statuses["refused: a hashed mark name"] == 9
    bold = '"marks":[{"type":"bold","attrs":true}]'
    assert js("marks: on then off") == (P + '{"type":"paragraph","content":[{"type":"text","text":"plain "},{"type":"text","text":"bold",' + bold +
                                       '},{"type":"text","text":" plain"}]}]}')
    two = js("marks: two marks, one re-set in place, one removed and re-added")
    assert '"text":"bbbb","marks":[{"type":"italic","attrs":true},{"type":"bold","attrs":{"v":2}}]' in two      # re-set: in place
    assert '"text":"cccc","marks":[{"type":"italic","attrs":true}]' in two
    assert '"text":"dddd","marks":[{"type":"italic","attrs":true},{"type":"bold","attrs":true}]' in two          # re-added: last
    assert js("marks: the same value set twice between strings (two ops with equal marks)") == (
        P + '{"type":"paragraph","content":[{"type":"text","text":"one",' + bold + '},{"type":"text","text":"two",' + bold + "}]}]}")
    assert '{"type":"text","text":"abcd"},{"type":"text","text":"ef"}' in js("marks: a deleted format item")
    assert js("marks: a format at the end of the list").endswith('"text":"tail",' + bold + "}]}]}")
    emb = js("marks: across an embed")
    assert '{"type":"text","text":{"rule":true}},' in emb
    assert '{"type":"text","text":{"image":"x.png","w":3},"marks":[{"type":"link","attrs":{"href":"https://example.org/?a=\\"b\\""}}]}' in emb
    assert ('"marks":[{"type":"9","attrs":"nine"},{"type":"10","attrs":"ten"},{"type":"b","attrs":true},{"type":"04","attrs":"text"},'
            '{"type":"a","attrs":1}]') in js("marks: index-like mark keys")
    vals = js("marks: values true, {}, a string, an object")
    for lit in ('"attrs":true', '"attrs":{}', '"attrs":"str \\"q\\""', '"attrs":{"x":[1,null],"y":{"z":false}}'):
        assert lit in vals, lit
    assert '"text":"leftright",' + bold in js("marks: a deleted string between two strings under equal marks (one op)")
    esc = js("strings: every escape class")
    assert '"text":"q\\" b\\\\ \\b\\f\\n\\r\\t \\u0001\\u001f \x7f \u2028 \U0001F600 end"' in esc
    assert js("strings: an emoji split by a concurrent insert").count("�") == 2
    assert '{"type":"no\\"de\\\\","attrs":{"k\\"e\\ny":"v"}' in js("strings: a node name and an attribute key that contain a quote")
    pend = js("state: pending structs with an integrated part")
    assert '"attrs":{"level":1}' in pend and '"text":"from-b",' + bold in pend
    st, big, _ = jf.edge("overflow: 64 one-character strings, each under one more mark")
    assert len(big) > 20 * len(st) and json.loads(big)["content"][0]["content"][63]["marks"][63]["type"] == "mark-number-63"
    for e in jf.load()["edges"]:
        for r in e["roots"]:
            if r[1] == 0:
                json.loads(bytes.fromhex(r[2]))      # every recorded JSON parses


@pytest.mark.skipif(not (NODE and BUNDLE), reason="node + the yjs bundle are needed to regenerate")
def test_fixture_regenerates(tmp_path):
    """The first 20 rows of every set and the edge sessions are what the committed tool makes from the bundle."""
    out = str(tmp_path / "j.json.gz")
    subprocess.run([NODE, os.path.join(ROOT, "tools", "json_corpus.js"), out, "20"], check=True, timeout=120, stdout=subprocess.DEVNULL)
    got = json.load(gzip.open(out, "rt"))
    fix = jf.load()
    assert got["inputs"] == fix["inputs"] and got["absent"] == fix["absent"] and got["full"] == fix["full"]
    for s in jf.SETS:
        assert got["sets"][s] == fix["sets"][s][:20], s
    assert got["edges"] == fix["edges"]


@pytest.fixture(scope="module")
def jsondev(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("jsondev") / "jsondev")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "snapdev", "jsondev.cpp")], check=True, timeout=300)
    return exe


@pytest.mark.parametrize("flags", ["1", "0"])
def test_kernel_code_on_host_vs_every_row(jsondev, tmp_path, flags):
    """The twin gives the fixture's status and bytes for every row, refusals included, with either flags value; only
    the overflow session takes the second run, and comes out of it with the recorded bytes."""
    rows = jf.expectations()
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    jf.write_asks(a, [(r[1], r[2]) for r in rows])
    subprocess.run([jsondev, a, b, flags], check=True, timeout=600)
    got = jf.read_jsondev(b)
    assert len(got) == len(rows) == 1788 + 5589 + sum(len(e["roots"]) for e in jf.load()["edges"])
    bad = [(r[0], r[2], r[3], g[0], g[2][:60]) for r, g in zip(rows, got) if not jf.matches(r, g[0], g[2])]
    assert not bad, (len(bad), bad[:5])
    reran = [r[0] for r, g in zip(rows, got) if g[1]]
    assert reran == ["overflow: 64 one-character strings, each under one more mark"]

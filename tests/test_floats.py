"""Non-integer numbers in stored-document JSON (YGM_F_FLOATS), without a GPU: the walkers' FLOATS instantiations
host-compiled through tools/snapdev/{tojsondev,jsondev,jsonfieldsdev}.cpp --floats against every row of
tests/golden/floats_v135.json.gz (yjs 13.5.16's JSON of states that hold floats), the same tools without the switch
(every row that holds a float is still YGM_ENONCANON, every other row unchanged), hand-written Array documents of the
V8 fixture's numbers, the overflow protocol's second run for numbers that grow from 9 to 24 bytes, and once more under
the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

import floats_fixture as ff
import json_fixture as jf
import tojson_fixture as tf
from hocuspocus_amd.engine import encode_fields

ROOT = ff.ROOT
NODE = shutil.which("node")
BUNDLE = os.path.exists("/opt/conda/share/jupyter/lab/static/3502.fbe0c610be82ba1360db.js")
TOOLS = ("tojsondev", "jsondev", "jsonfieldsdev")


def build(tmp_path_factory, tag, flags):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    d = tmp_path_factory.mktemp(tag)
    for t in TOOLS:
        subprocess.run(["g++", *flags, "-std=c++17", "-o", str(d / t), os.path.join(ROOT, "tools", "snapdev", t + ".cpp")], check=True, timeout=900)
    return d


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    return build(tmp_path_factory, "floatsdev", ["-O1"])


def tojson(d, tmp_path, asks, floats, cap=0):
    """asks = [(state, name, kind)] -> [(status, reran, bytes)]"""
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    tf.write_asks(a, asks)
    subprocess.run([str(d / "tojsondev"), *(["--floats"] if floats else []), a, b, "0", str(cap)], check=True, timeout=900)
    return tf.read_tojsondev(b)


def pm(d, tmp_path, tool, asks, floats):
    """asks = [(state, name or encoded field list)] -> [(status, reran, bytes)]"""
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    jf.write_asks(a, asks)
    subprocess.run([str(d / tool), a, b, "0", *(["--floats"] if floats else [])], check=True, timeout=900)   # (the switch may stand anywhere)
    return jf.read_jsondev(b)


def same(rows, got, floats):
    want = ff.want(rows, floats)
    bad = [(r[0], r[2], w[0], g[0], w[1][:80], g[2][:80]) for r, w, g in zip(rows, want, got) if (g[0], g[2]) != w]
    assert len(got) == len(rows) and not bad, (floats, len(bad), bad[:4])


def test_fixture_holds_what_it_is_named_for():
    tj, pj, fj = ff.tojson_rows(), ff.json_rows(), ff.fields_rows()
    by = {}
    for r in tj:
        by.setdefault(r[0], []).append(r)
    # the float families that tojson_v135 / json_v135 pin as refusals: serialized with the flag, status 3 without
    fam = by["refused: a finite non-integer number"]
    assert [(r[4], r[5], r[6]) for r in fam] == [(0, b'{"w":1.5}', 3), (0, b'[{"deep":[0.25]}]', 3)]
    assert [(r[4], r[5], r[6]) for r in by["refused: an integer above 2^53"]] == [(0, b'{"w":1152921504606847000}', 3)]
    assert [(r[4], r[6]) for r in by["a float before a BigInt, and a float after a Uint8Array"]] == [(1, 3), (9, 9)]
    assert [(r[4], r[6]) for r in by["integers only (the flag changes nothing)"]] == [(0, 0)] * 3
    inf = by["Infinity and NaN beside floats"]
    assert inf[0][5] == b'{"inf":null,"half":0.5,"nan":null,"ninf":null}' and inf[1][5] == b"[null,0.25,null]"
    bare = by["every edge value, bare, in a Map and an Array"][1]
    for s in (b"5e-324", b"2.2250738585072014e-308", b"1.7976931348623157e+308", b"0.30000000000000004", b"1e+21", b"999999999999999900000",
              b"1152921504606847000", b"18446744073709552000", b"0.000001", b"1e-7", b"1.5e-7", b"0.10000000149011612", b"-1.5", b"100.25"):
        assert b"," + s + b"," in bare[5], s
    assert bare[4] == 0 and bare[6] == 3 and by["every edge value nested in objects and arrays inside an Any"][0][5].count(b"5e-324") >= 4
    rnd = [r for r in tj if r[0].startswith("random session ")]
    assert len(rnd) == 3 * 120 and sum(r[4] == 0 and r[6] == 3 for r in rnd) >= 100      # floaty forced on: refused today
    assert {(r[4], r[6]) for r in rnd} <= {(0, 0), (0, 3)}
    pby = {}
    for r in pj:
        pby.setdefault(r[0], []).append(r)
    for note, piece in (("refused: a float attribute", b'"attrs":{"w":1.5}'), ("refused: a float in a mark", b'{"type":"size","attrs":{"pt":10.5}}'),
                        ("refused: a float in an embed", b'"text":{"ratio":0.5}')):
        r = pby[note][0]
        assert (r[3], r[5]) == (0, 3) and piece in r[4], note
    # the state's parse refuses these with the flag too, whatever root is asked (the absent one included)
    for note in ("a 17-digit float inside an embed, the only float (refused with the flag too)",
                 "a float with an exponent inside a mark (refused with the flag too)"):
        assert [(r[3], r[5]) for r in pby[note]] == [(3, 3)] * 2, note
    assert [(r[3], r[5]) for r in pby["an attribute that is not finite (refused with the flag too)"]] == [(3, 3), (0, 0)]
    assert [(r[3], r[5]) for r in fj] == [(0, 3), (0, 3), (0, 0), (0, 3), (0, 0)]          # refused only when the float's field is reached
    assert fj[1][4].startswith(b'{"first":{"type":"doc"') and b'"second":{' in fj[1][4] and b'"width":0.5' in fj[1][4]
    assert os.path.getsize(ff.FLOATS_FIX) <= max(os.path.getsize(os.path.join(ff.GOLDEN, f)) for f in os.listdir(ff.GOLDEN)
                                                 if os.path.isfile(os.path.join(ff.GOLDEN, f)))


@pytest.mark.parametrize("floats", [True, False])
def test_walkers_on_host_vs_every_row(tools, tmp_path, floats):
    """With --floats every string and status equals yjs's; without it every row that holds a float is still status 3
    and every other row is what it was."""
    tj, pj, fj = ff.tojson_rows(), ff.json_rows(), ff.fields_rows()
    same(tj, tojson(tools, tmp_path, [(r[1], r[2], r[3]) for r in tj], floats), floats)
    same(pj, pm(tools, tmp_path, "jsondev", [(r[1], r[2]) for r in pj], floats), floats)
    same(fj, pm(tools, tmp_path, "jsonfieldsdev", [(r[1], encode_fields(r[2])) for r in fj], floats), floats)
    if not floats:
        assert sum(r[-1] == 3 and r[-3] == 0 for r in tj + pj + fj) >= 180


def test_array_documents_of_the_v8_numbers(tools, tmp_path):
    """Documents written out by hand, 512 numbers each, as the GPU test batches them: every string is V8's."""
    v8 = ff.v8_doubles()
    docs = [ff.array_doc([x for x, _ in v8[i:i + 512]], 7 + i) for i in range(0, len(v8), 512)]
    for (state, js), i in zip(docs, range(0, len(v8), 512)):
        assert js == ("[" + ",".join(s for _, s in v8[i:i + 512]) + "]").encode()
    got = tojson(tools, tmp_path, [(d[0], b"a", ff.ARRAY) for d in docs], True)
    assert [(g[0], g[2]) for g in got] == [(0, d[1]) for d in docs]
    off = tojson(tools, tmp_path, [(d[0], b"a", ff.ARRAY) for d in docs], False)
    assert [(g[0], g[2]) for g in off] == [(3, b"")] * len(docs)


def test_numbers_that_grow_take_the_second_run(tools, tmp_path):
    """512 times -1.7976931348623157e+308: 24 bytes of JSON for 9 of state, more than the workspace's output region
    holds -- the document runs again into a region of exactly the recorded length."""
    state, js = ff.array_doc([ff.LONGEST] * 512)
    assert len(js) == 512 * 25 + 1 and len(state) < 512 * 9 + 16
    got = tojson(tools, tmp_path, [(state, b"a", ff.ARRAY)], True)
    assert got == [(0, 1, js)]
    small = ff.array_doc([1.5, 0.25])
    assert tojson(tools, tmp_path, [(small[0], b"a", ff.ARRAY)], True) == [(0, 0, small[1])]
    # with a small forced cap every longer JSON of the fixture reruns and still comes out as recorded
    tj = ff.tojson_rows()
    forced = tojson(tools, tmp_path, [(r[1], r[2], r[3]) for r in tj], True, cap=48)
    same(tj, forced, True)
    assert [bool(g[1]) for g in forced] == [r[4] == 0 and len(r[5]) > 48 for r in tj]


def test_sanitizer_builds_over_the_fixture(tmp_path_factory, tmp_path):
    """The three harnesses as the stand-alone programs they are, built with -fsanitize=address,undefined and run once
    over every row with --floats, the hand-written documents and the forced cap included."""
    d = build(tmp_path_factory, "floatsdev_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    tj, pj, fj = ff.tojson_rows(), ff.json_rows(), ff.fields_rows()
    same(tj, tojson(d, tmp_path, [(r[1], r[2], r[3]) for r in tj], True), True)
    same(tj, tojson(d, tmp_path, [(r[1], r[2], r[3]) for r in tj], True, cap=48), True)
    same(pj, pm(d, tmp_path, "jsondev", [(r[1], r[2]) for r in pj], True), True)
    same(fj, pm(d, tmp_path, "jsonfieldsdev", [(r[1], encode_fields(r[2])) for r in fj], True), True)
    state, js = ff.array_doc([ff.LONGEST] * 512)
    v8 = ff.array_doc([x for x, _ in ff.v8_doubles()[:512]])
    assert tojson(d, tmp_path, [(state, b"a", ff.ARRAY), (v8[0], b"a", ff.ARRAY)], True) == [(0, 1, js), (0, 1, v8[1])]


@pytest.mark.skipif(not (NODE and BUNDLE), reason="node + the yjs bundle are needed to regenerate")
def test_fixture_regenerates(tmp_path):
    import gzip
    import json
    out = str(tmp_path / "f.json.gz")
    subprocess.run([NODE, os.path.join(ROOT, "tools", "floats_corpus.js"), out], check=True, timeout=300, stdout=subprocess.DEVNULL)
    assert json.load(gzip.open(out, "rt")) == ff.load(ff.FLOATS_FIX)

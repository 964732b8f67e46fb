"""Every field of a stored document as one JSON object (ygm_json_fields_v1), without a GPU: the committed fixture, its
regeneration from the committed tool, k_json's fields code (ygm_json.hpp) host-compiled through
tools/snapdev/jsonfieldsdev.cpp against every row of the fixture -- objects and refusals, with the overflow protocol's
second run -- the field-list decoder's refusals, and the Python encoder of field lists."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

import json_fields_fixture as ff
import json_fixture as jf

ROOT = jf.ROOT
NODE = shutil.which("node")
BUNDLE = os.path.exists("/opt/conda/share/jupyter/lab/static/3502.fbe0c610be82ba1360db.js")
EINVAL = 8
EMPTY_STATE = b"\x00\x00"      # Y.encodeStateAsUpdate(new Y.Doc())
E = ff.EMPTY_DOC.decode()


def obj(note, k):
    r = ff.edge(note)[k]
    assert r.status == 0, (note, k)
    return r.json.decode()


def statuses(note):
    return [r.status for r in ff.edge(note)]


def test_fixture_present_made_from_the_committed_inputs():
    fix = ff.load()
    assert set(fix["inputs"]) == {s + ".json.gz" for s in ff.SETS}
    for name, sha in fix["inputs"].items():
        assert jf.input_sha256(name) == sha, name
    single = jf.load()
    for s in ff.SETS:
        assert len(fix["sets"][s]) == len(jf.set_states(s))
        for e, roots in zip(fix["sets"][s], single["sets"][s]):
            share = [r[0] for r in roots[:-1]]      # json_v135 lists a state's roots in doc.share order
            assert sorted(e["keys"]) == sorted(share)
            assert e["asks"][0][0] is None
            listed = share[::-1] + [fix["absent"]]
            assert e["asks"][1][0] == listed + listed[:1]      # reversed, an absent name, the first once more
            # the third ask: the roots json_v135 serializes, reversed (absent when there is none)
            good = [r[0] for r in roots[:-1] if r[1] == 0][::-1]
            assert [a[0] for a in e["asks"][2:]] == ([good] if good else [])
    assert os.path.getsize(ff.FIX) <= max(os.path.getsize(os.path.join(jf.GOLDEN, f)) for f in os.listdir(jf.GOLDEN)
                                          if f != os.path.basename(ff.FIX) and os.path.isfile(os.path.join(jf.GOLDEN, f)))
    rows = ff.rows()
    assert {r.status for r in rows} == {0, 3, 9}
    multi = [r for r in rows if r.status == 0 and r.fields and len(set(r.fields)) >= 2]
    assert len(multi) > 1000
    for r in ff.rows(sets=(), edges=True):
        if r.status == 0:
            json.loads(r.json)


def test_objects_are_their_single_field_jsons_joined_in_key_order():
    """Ties the fixture to json_v135: an all-fields object is '{' + "key": the root's recorded JSON, ... + '}' in the
    recorded key order, and the first refusing root in that order gives the status."""
    single = jf.load()
    checked = 0
    for s in ff.SETS:
        for e, roots in zip(ff.load()["sets"][s][:ff.load()["full"]], single["sets"][s]):
            by = {r[0]: r for r in roots[:-1]}
            a = e["asks"][0]
            refusals = [by[k][1] for k in e["keys"] if by[k][1] != 0]
            assert a[1] == (refusals[0] if refusals else 0)
            asks = ([(a, e["keys"])] if a[1] == 0 else []) + [(g, g[0]) for g in e["asks"][2:]]
            for ask, order in asks:      # (a listed ask of the sets holds no index key: its order is the list's)
                assert not any(bytes.fromhex(k).isdigit() for k in order) or ask is a
                want = "{" + ",".join(json.dumps(bytes.fromhex(k).decode(), ensure_ascii=False) + ":" + bytes.fromhex(by[k][2]).decode()
                                      for k in order) + "}"
                assert ask[1] == 0 and bytes.fromhex(ask[2]).decode() == want
                checked += 1
    assert checked >= 100


def test_edge_sessions_say_what_they_are_named_for():
    p = '{"type":"doc","content":[{"type":"paragraph","content":[{"type":"text","text":"%s"}]}]}'
    assert [obj("no roots", k) for k in range(4)] == ["{}", '{"a":%s}' % E, '{"a":%s}' % E, '{"":%s}' % E]
    one = p % "only"
    assert [obj("one root", k) for k in range(4)] == ['{"default":%s}' % one] * 3 + ['{"no-such-root":%s,"default":%s}' % (E, one)]
    odd = "roots named 2, 10, b, 01, the empty name, 4294967295 and a name to escape"
    esc = '"a\\"\\\\\\n\\u0001é"'
    assert obj(odd, 0) == ('{"2":%s,"10":%s,"b":%s,"01":%s,"":%s,"4294967295":%s,%s:%s}'
                           % tuple([p % "in 0", p % "in 1", p % "in 2", p % "in 3", p % "in 4", p % "in 5", esc, p % "in 6"]))
    # reversed, the absent name, the first once more: index keys first, the others where they first stand
    assert obj(odd, 1) == ('{"2":%s,"10":%s,%s:%s,"4294967295":%s,"":%s,"01":%s,"b":%s,"no-such-root":%s}'
                           % (p % "in 0", p % "in 1", esc, p % "in 6", p % "in 5", p % "in 4", p % "in 3", p % "in 2", E))
    assert obj(odd, 2) == '{"2":%s,"9":%s,"10":%s,"b":%s,"":%s}' % (p % "in 0", E, p % "in 1", p % "in 2", p % "in 4")
    assert obj(odd, 3) == '{"0":%s,"4294967294":%s,"4294967295":%s,"00":%s}' % (E, E, p % "in 5", E)
    assert statuses("a __proto__ root") == [9, 9, 9, 0, 0]
    assert list(json.loads(obj("a __proto__ root", 4))) == ["__proto_", "__proto__x", "first"]
    assert statuses("two roots, the second refuses with 9") == [9, 9, 9, 0, 9, 9]
    # "1" is written first whatever the list says: its refusal (3) is the document's; __proto__ counts where it stands
    assert statuses("two roots, the first in output order refuses with 3, the other with 9") == [3, 3, 3, 9, 3, 3]
    assert obj("a map-only root beside a fragment", 0) == '{"meta":%s,"default":%s}' % (E, p % "x")
    assert statuses("a Y.Text root beside a fragment root") == [9, 0, 9, 9]
    assert obj("an empty Y.Text root beside a fragment root", 0) == '{"title":%s,"default":%s}' % (E, p % "x")
    pend = "a root named only by pending structs"
    assert [k.decode() for k in ff.edge(pend)[0].keys] == ["base", "late"]      # in doc.share, though only pending structs name it
    assert obj(pend, 0) == '{"base":%s,"late":%s}' % (p % "kept", E) and obj(pend, 1) == '{"late":%s}' % E
    big = ff.edge("overflow: six roots that fit one by one, an object that does not")
    assert big[0].length == 288265 and list(json.loads(big[0].json)) == ["root-%d" % i for i in range(6)]


@pytest.mark.skipif(not (NODE and BUNDLE), reason="node + the yjs bundle are needed to regenerate")
def test_fixture_regenerates(tmp_path):
    """The first 20 rows of every set and the edge sessions are what the committed tool makes from the bundle."""
    out = str(tmp_path / "f.json.gz")
    subprocess.run([NODE, os.path.join(ROOT, "tools", "json_fields_corpus.js"), out, "20"], check=True, timeout=120, stdout=subprocess.DEVNULL)
    got = json.load(gzip.open(out, "rt"))
    fix = ff.load()
    assert got["inputs"] == fix["inputs"] and got["absent"] == fix["absent"] and got["full"] == fix["full"]
    for s in ff.SETS:
        assert got["sets"][s] == fix["sets"][s][:20], s
    assert got["edges"] == fix["edges"]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("jsonfieldsdev") / "jsonfieldsdev")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "snapdev", "jsonfieldsdev.cpp")], check=True, timeout=300)
    return exe


def run_twin(twin, tmp_path, asks, flags="1"):
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    jf.write_asks(a, asks)
    subprocess.run([twin, a, b, flags], check=True, timeout=600)
    got = jf.read_jsondev(b)
    assert len(got) == len(asks)
    return got


@pytest.mark.parametrize("flags", ["1", "0"])
def test_kernel_code_on_host_vs_every_row(twin, tmp_path, flags):
    """The twin gives the fixture's status and bytes for every row, refusals included, with either flags value; the
    objects that outgrow their output region take the second run and come out of it with the recorded bytes."""
    rows = ff.rows()
    got = run_twin(twin, tmp_path, list(zip([r.state for r in rows], ff.field_lists(rows))), flags)
    bad = [(r.label, r.fields, r.status, g[0], g[2][:60]) for r, g in zip(rows, got) if not ff.matches(r, g[0], g[2])]
    assert not bad, (len(bad), bad[:5])
    reran = {r.label for r, g in zip(rows, got) if g[1]}
    assert "overflow: six roots that fit one by one, an object that does not" in reran
    assert "no roots" not in reran and "one root" not in reran


def vs(n):
    out = bytearray()
    while n > 127:
        out.append(0x80 | (n & 127))
        n >>= 7
    out.append(n)
    return bytes(out)


BAD_LISTS = {
    "a length past the list's end": b"\x05abcd",
    "a length past the end after a good name": b"\x01a\x03bc",
    "a length cut inside its varuint": b"\x01a\x81",
    "a 6-byte varuint": b"\x81\x80\x80\x80\x80\x00",
    "a 5-byte varuint of 2^34": b"\x80\x80\x80\x80\x40",
    "a non-minimal varuint": b"\x81\x00a",
    "a non-minimal zero": b"\x80\x00",
    "a lone continuation byte": b"\x01\x80",
    "an overlong encoding": b"\x02\xc0\xaf",
    "a surrogate": b"\x03\xed\xa0\x80",
    "a name cut inside a character": b"\x02a\xc3",
    "1025 names": b"".join(vs(len(b"n%d" % i)) + b"n%d" % i for i in range(1025)),
}
GOOD_LISTS = {
    "1024 names": b"".join(vs(len(b"n%d" % i)) + b"n%d" % i for i in range(1024)),
    "1024 times one name": b"\x01a" * 1024,
    "a two-byte varuint": vs(200) + b"k" * 200,
    "the empty name twice": b"\x00\x00",
}


def test_field_list_refusals(twin, tmp_path):
    """A bad list is YGM_EINVAL for its document whatever the state holds; a refused state's own status comes first."""
    one = ff.edge("one root")[0].state
    refused = ff.edge("two roots, the first in output order refuses with 3, the other with 9")[0].state
    cut = one[:-3]
    asks = [(st, fl) for fl in BAD_LISTS.values() for st in (EMPTY_STATE, one)]
    got = run_twin(twin, tmp_path, asks)
    assert [(g[0], g[2]) for g in got] == [(EINVAL, b"")] * len(asks), [(k, g[0]) for k, g in zip(BAD_LISTS, got[::2]) if g[0] != EINVAL]
    good = run_twin(twin, tmp_path, [(EMPTY_STATE, fl) for fl in GOOD_LISTS.values()])
    assert [g[0] for g in good] == [0] * len(GOOD_LISTS)
    assert list(json.loads(good[0][2])) == ["n%d" % i for i in range(1024)] and good[0][1] == 1      # (the object alone reruns)
    assert good[1][2] == b'{"a":%s}' % ff.EMPTY_DOC and good[2][2] == b'{"%s":%s}' % (b"k" * 200, ff.EMPTY_DOC)
    assert good[3][2] == b'{"":%s}' % ff.EMPTY_DOC
    # the state's status comes before the list's: a truncated state, an empty state, a parse-level refusal
    first = run_twin(twin, tmp_path, [(cut, BAD_LISTS["a 6-byte varuint"]), (b"", BAD_LISTS["a non-minimal varuint"]), (cut, b"")])
    assert first[0][0] == first[2][0] != 0 and first[0][0] != EINVAL and first[1][0] == 1
    # ...but a root's refusal does not: the list is looked at before any root is walked
    assert run_twin(twin, tmp_path, [(refused, BAD_LISTS["a surrogate"])])[0][0] == EINVAL


def test_engine_encoder_round_trips_names(twin, tmp_path):
    from hocuspocus_amd.engine import encode_fields
    assert encode_fields(None) == encode_fields([]) == b""
    names = ["", "a", "b" * 127, "c" * 128, "é" * 64, "d" * 16384]
    assert encode_fields([""]) == b"\x00" and encode_fields(["a"]) == b"\x01a"
    assert encode_fields(["b" * 127])[:2] == b"\x7fb" and encode_fields(["c" * 128])[:3] == b"\x80\x01c"
    assert encode_fields(["é" * 64])[:2] == b"\x80\x01" and encode_fields([b"\xc3\xa9"]) == b"\x02\xc3\xa9"
    assert encode_fields(["d" * 16384])[:3] == b"\x80\x80\x01"
    got = run_twin(twin, tmp_path, [(EMPTY_STATE, encode_fields([n])) for n in names] + [(EMPTY_STATE, encode_fields(names))])
    for n, g in zip(names, got):
        assert g[0] == 0 and json.loads(g[2]) == {n: json.loads(ff.EMPTY_DOC)}, len(n)
    assert got[-1][0] == 0 and list(json.loads(got[-1][2])) == names

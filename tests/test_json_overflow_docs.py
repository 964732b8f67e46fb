"""The documents of the JSON overflow tests (tests/json_overflow_docs.py), without a GPU: the by-construction JSON
against yjs (tests/golden/json_overflow_v135.json.gz), the fixture's regeneration from the committed tools, and
k_json's sequential code host-compiled (tools/snapdev/jsondev.cpp) over every row -- with its second run taken exactly
by the documents whose restated delta is positive, which ties caps_out to the library's Caps::out."""
import json
import os
import shutil
import subprocess

import pytest

import json_fixture as jf
import json_overflow_docs as g

ROOT = jf.ROOT
FIX = os.path.join(jf.GOLDEN, "json_overflow_v135.json.gz")
NODE = shutil.which("node")
BUNDLE = os.path.exists("/opt/conda/share/jupyter/lab/static/3502.fbe0c610be82ba1360db.js")


def by_ask():
    return {(r[1], r[2]): r for r in g.built_rows()}


def test_expect_equals_yjs_for_every_document_by_construction():
    rows = by_ask()
    docs = g.unique()
    assert len(rows) == 2 * len(g.states()) and len(docs) == len(g.states()) + 1      # (one state is asked by both names)
    for d in docs:
        assert jf.matches(rows[(d.u, d.ask)], d.status, d.json), d.name
        absent = rows[(d.u, g.ABSENT)]
        assert absent[3] == 0 and absent[4] == g.EMPTY, d.name
    fix = g.load()
    assert bytes.fromhex(fix["absent"]) == g.ABSENT
    big = [r for r in g.built_rows() if r[4] is None]
    assert big and all(r[6] > fix["hash_over"] for r in big)
    assert all(r[6] <= fix["hash_over"] for r in g.built_rows() + g.session_rows() if r[4] is not None)
    assert os.path.getsize(FIX) <= 16384


def test_the_figures_of_the_family():
    """K = 21 with tail z fits with 12 bytes to spare, K = 22 does not; the restated cap against the documents' sizes."""
    d21, d22, d64 = g.family("", 21), g.family("", 22), g.family("", 64)
    assert (len(d21.u), len(d21.json), g.caps_out(len(d21.u), 45)) == (384, 7140, 7152) and not d21.rerun
    assert (len(d22.json), g.caps_out(len(d22.u), 47)) == (7783, 7457) and d22.rerun
    assert (len(d64.json), g.caps_out(len(d64.u), 131)) == (60073, 20270)
    assert len(g.no_tail().json) == 13934 and g.no_tail().rerun
    assert g.absent_ask().json == g.EMPTY and len(g.EMPTY) == 27 and not g.absent_ask().rerun and g.absent_ask().delta > 0
    assert [(d.status, d.rerun, d.json) for d in g.late_refusals()] == [(9, False, b""), (3, False, b"")]
    assert all(d.delta > 0 for d in g.late_refusals())
    assert [g.delta(d) for d in g.sweep()] == list(range(-4, 20))
    assert {0, 1, 16, 17} <= {g.delta(d) for d in g.sweep()}
    assert [d.rerun for d in g.sweep()] == [False] * 5 + [True] * 19
    assert all(d.rerun for d in g.grid(65) + [g.big(0), g.big(1)]) and not any(g.fit(s).rerun for s in range(4))
    assert len(g.filler(48000).u) == 48000 and len(g.filler(40001, 3, b"r").u) == 40001


def test_grid_is_pairwise_distinct():
    docs = g.grid(65)
    assert len({d.u for d in docs}) == len({d.json for d in docs}) == 65
    assert {int(d.name.split()[3]) for d in docs} == set(range(22, 41))
    for root in (b"r", b"n" * 130):
        assert len({d.json for d in g.grid(3, root)} | {d.json for d in docs}) == 65      # (the JSON does not hold the root's name)
        assert not {d.u for d in g.grid(3, root)} & {d.u for d in docs}


def test_boundary_sessions_say_what_they_are_named_for():
    ses = {e["note"]: e["roots"] for e in g.load()["sessions"]}
    st = {n: r[0][1] for n, r in ses.items()}
    js = {n: bytes.fromhex(r[0][2]).decode() for n, r in ses.items() if r[0][1] == 0}
    assert len(ses) == 26 and all(len(r) == 2 and bytes.fromhex(r[1][0]) == g.ABSENT for r in ses.values())
    idx = [n for n in ses if n.startswith("index keys as attributes")][0]
    assert '"attrs":{"0":"v0","7":"v7","4294967294":"v4294967294","4294967295":"v4294967295","00":"v00","-1":"v-1"' in js[idx]
    mk = [n for n in ses if n.startswith("index keys as marks")][0]
    assert js[mk].index('"type":"0"') < js[mk].index('"type":"7"') < js[mk].index('"type":"4294967294"') < js[mk].index('"type":"4294967295"')
    assert {n[10:]: s for n, s in st.items() if n.startswith("mark name ")} == {
        "--AbCd0123": 9, "-AbCd0123x": 0, "c--AbCd012": 0, "c--AbCd01_2": 0, "c--AbCd0123x": 0, "é--AbCd0123": 9, "c--========": 9}
    assert js["a hashed mark set and nulled before any live string"].endswith('[{"type":"text","text":"tail"}]}]}')
    assert {n[18:]: s for n, s in st.items() if n.startswith("attribute integer ")} == {
        "2147483647": 0, "-2147483647": 0, "2147483648": 3, "-2147483648": 3, "0": 0, "-0": 0}
    assert '"attrs":{"n":0}' in js["attribute integer -0"]
    assert '"attrs":100000000000000000000}' in js["mark numbers 1e20, -0, 123456789012"] and '{"z":0}' in js["mark numbers 1e20, -0, 123456789012"]
    assert st["mark number 1e21"] == 3 and st["mark number of 16 digits"] == 3
    # what the state's parse refuses is refused for every name; a refusal in the root's subtree is not
    for n, r in ses.items():
        whole = n in ("mark number 1e21", "mark number of 16 digits", "attribute integer -2147483648")
        assert (r[1][1], r[1][2]) == ((3, "") if whole else (0, g.EMPTY.hex())), n
    assert '"type":"1.5e3","attrs":"2.5e10"' in js["a mark key and string values that hold digits, dots and e"]
    four = js["four XmlTexts in one element: the first ends bold, one is empty, then an element, then text"]
    assert four == ('{"type":"doc","content":[{"type":"paragraph","content":[{"type":"text","text":"ends-bold","marks":[{"type":"bold","attrs":true}]},'
                    '{"type":"text","text":"plain"},{"type":"inner","content":[{"type":"text","text":"inside"}]},{"type":"text","text":"last"}]}]}')
    assert js["empty XmlTexts directly under the fragment, between elements"].startswith('{"type":"doc","content":[[],{"type":"paragraph"')
    assert '"text":{}}' in js["embed values {} and an array"] and '"text":[1,[2,"x"],{}],"marks"' in js["embed values {} and an array"]
    assert [s for n, s in st.items() if n.startswith("refused: ")] == [9, 9, 9]
    for r in g.session_rows():
        if r[3] == 0:
            json.loads(r[4])


@pytest.mark.skipif(not (NODE and BUNDLE), reason="node + the yjs bundle are needed to regenerate")
def test_fixture_regenerates(tmp_path):
    from tools import json_overflow_fixture
    out = str(tmp_path / "o.json.gz")
    json_overflow_fixture.build(out)
    assert json_overflow_fixture.text(out) == json_overflow_fixture.text(FIX)


@pytest.fixture(scope="module")
def jsondev(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("jsondev") / "jsondev")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "snapdev", "jsondev.cpp")], check=True, timeout=300)
    return exe


@pytest.mark.parametrize("flags", ["1", "0"])
def test_kernel_code_on_host_vs_every_row(jsondev, tmp_path, flags):
    """The twin gives the golden status and bytes for every row; among the by-construction documents it takes the
    second run exactly where delta > 0 and the document is not refused or asked by an absent name -- delta 0 fits,
    delta +1 does not; a late refusal leaves the first run with its refusal, not with the internal status."""
    rows = g.built_rows() + g.session_rows()
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    jf.write_asks(a, [(r[1], r[2]) for r in rows])
    subprocess.run([jsondev, a, b, flags], check=True, timeout=600)
    got = jf.read_jsondev(b)
    assert len(got) == len(rows)
    bad = [(r[0], r[2], r[3], x[0], x[2][:60]) for r, x in zip(rows, got) if not jf.matches(r, x[0], x[2])]
    assert not bad, (len(bad), bad[:5])
    assert jf.ST_MORE not in {x[0] for x in got}
    reran = {(r[1], r[2]): bool(x[1]) for r, x in zip(rows, got)}
    for d in g.unique():
        assert reran[(d.u, d.ask)] == d.rerun, (d.name, d.delta)
        assert d.rerun == (d.delta > 0 and d.status == 0 and d.ask != g.ABSENT), d.name
        assert not reran[(d.u, g.ABSENT)], d.name
    assert not any(x[1] for r, x in zip(rows, got) if r[0] in {e["note"] for e in g.load()["sessions"]})

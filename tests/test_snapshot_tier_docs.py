"""CPU check of the corpus the GPU tests feed the snapshot cascade (snapshot_tier_docs.py) and of its yjs fixture
(tests/golden/snapshot_tier_edges_v135.json.gz): the fixture is what the committed tooling writes; the general kernel's
code host-compiled (tools/snapdev) equals yjs on every row, in both delete-set orders and for gc: false documents; the
flat-text code host-compiled (tools/snapdev/snaptext.cpp) with the workspaces of the two launches -- and the 4 KiB one of
YGM_SNAP_TEXT=4 -- takes exactly the rows labelled so and equals yjs on them."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

import snapshot_tier_docs as g
from devrun import same
from snapshot_tier_docs import FIX, expected, rows
from twins import BUNDLE, NODE, NOGC, _resolve_pending, build_twin, read_res, run_snaptext, write_in

GXX = pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
CENSUS = {"first": 242, "second": 15, "general": 41, "pending": 11, "throws": 27}


def test_caps_restate_the_layout():
    assert (g.CAP_FIRST, g.CAP_SECOND, g.CAP_4K) == (207, 865, 134)


def test_fixture_matches_the_corpus():
    docs = g.unique()
    r = rows()
    assert list(r) == [d.name for d in docs]
    for d in docs:
        u, (st, e), (st2, x) = r[d.name]
        assert u == d.u and st == st2, d.name
        assert (st != 0) == (d.tier == "throws"), (d.name, st)
        assert st or (e and x), d.name
    assert os.path.getsize(FIX) < 819131
    assert g.census() == CENSUS
    assert all(g.get(n).tier == "general" and r[n][1][0] == 0 for n in g.UNSUPPORTED)
    assert sum(e != x for _, e, x in r.values()) >= 100      # gc: false keeps deleted content: other bytes


@pytest.mark.skipif(not (NODE and BUNDLE), reason="node + the yjs bundle are needed to regenerate")
def test_fixture_regenerates():
    from tools import snap_fixture
    assert snap_fixture.tier_rows() == json.load(gzip.open(FIX, "rt"))["rows"]


def test_families_cover_the_named_edges():
    a = g.families()["A"]
    for c in (134, 207, 865):
        for kind in ("structs", "ranges", "origins"):
            assert sorted(d.parts for d in a if d.name.startswith("A cap %d %s " % (c, kind))) == list(range(c - 2, c + 3))
    assert {g.tier_at(d, 134) for d in a} == {"first", "second", "general"}
    assert len(g.C_DROPPED) * 20 <= len(g.C_SEEDS) and len(g.families()["C"]) == len(g.C_SEEDS) - len(g.C_DROPPED)
    orders = [d.name.split()[-1] for d in g.families()["C"]]
    assert {o: orders.count(o) for o in set(orders)} == {"ascending": 50, "descending": 50, "shuffled": 50}
    assert {int(d.name.split()[3]) for d in g.families()["C"]} >= {2, 3, 4, 8, 16}
    # D: each document starts at every residue, four of each tier and a truncated one; and once as the arena's last
    names = g.d_names()
    res = g.start_residues(g.family_d())
    assert all(res[n] == set(range(16)) for n in names)
    assert [g.get(n).tier for n in names] == ["first"] * 4 + ["second"] * 4 + ["general"] * 4 + ["throws"]
    assert [b[-1].name for b in g.family_d_last()] == names
    # E: a & 15 and b - a16 of the second group of 16
    seen = set()
    for r, t, docs in g.family_e()[:-1]:
        a, b = sum(len(d.u) for d in docs[:16]), sum(len(d.u) for d in docs)
        assert len(docs) == 32 and a & 15 == r and b - (a & ~15) == t
        assert {d.tier for d in docs[16:]} == {"first", "general"}
        seen.add((r, t - 40960))
    assert seen == {(r, x) for r in (0, 1, 8, 15) for x in (-16, -1, 0, 1, 16)}
    big = g.family_e()[-1][2]
    assert len(big) == 32 and sorted(len(d.u) for d in big[:16])[-2:] == [26, 41000]
    f = g.families()["F"]
    assert len(f) == 7 and f[0].u == b"" and len(f[1].u) == 11 and [d.tier for d in f[:2]] == ["throws", "pending"]
    assert [d.name for d in g.family_f(9, 5)] == [f[k % 7].name for k in range(5, 14)]


@GXX
@pytest.mark.parametrize("flags", [1, 0, 1 | NOGC, NOGC])
def test_general_kernel_code_on_host_equals_yjs(tmp_path, flags):
    """tools/snapdev over every row: 13.5 order and the default (golden.ds_to_desc), garbage-collecting and gc: false; a
    document it leaves pending (status 64) is one labelled so, its three updates merged by the oracle as the engine's
    merge kernels do."""
    exe = build_twin(tmp_path, "snapdev")
    docs = g.unique()
    a, b = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_in(a, [d.u for d in docs])
    subprocess.run([exe, a, b, str(flags)], check=True, timeout=300)
    got = read_res(b)
    assert len(got) == len(docs)
    for d, (st, body) in zip(docs, got):
        assert (st == 64) == (d.tier == "pending"), (d.name, st)
        res = _resolve_pending(st, body if st in (0, 64) else b"", bool(flags & 1))
        exp = expected(d, bool(flags & 1), bool(flags & NOGC))
        assert same(exp, res), (d.name, flags, exp[0], res[0])


@GXX
@pytest.mark.parametrize("flags", [1, 0, 1 | NOGC])
def test_flat_text_code_on_host_takes_what_the_labels_say(tmp_path, flags):
    """tools/snapdev/snaptext.cpp with 6 144, 24 576 and 4 096 bytes of workspace: the rows it takes are those labelled
    'first' / 'first' or 'second' / family A's at the 134-part cap, and on every row it takes its bytes are yjs's."""
    exe = build_twin(tmp_path, "snaptext")
    docs = g.unique()
    us = [d.u for d in docs]
    for budget, want in ((6144, {k for k, d in enumerate(docs) if d.tier == "first"}),
                         (24576, {k for k, d in enumerate(docs) if d.tier in ("first", "second")}),
                         (4096, None)):
        taken, _, got = run_snaptext(exe, tmp_path, us, flags, budget)
        taken = set(taken)
        if want is None:      # family C's documents hold up to 200 parts: 134 decides family A and the small ones
            small = {k for k, d in enumerate(docs) if d.tier == "first" and d.parts is None and not d.name.startswith("C ")}
            want = {k for k, d in enumerate(docs) if d.parts is not None and g.tier_at(d, g.CAP_4K) == "first"} | small
            taken -= {k for k, d in enumerate(docs) if d.name.startswith("C ")}
        assert taken == want, (budget, [docs[k].name for k in sorted(taken ^ want)][:8])
        for k in taken:
            assert got[k] == expected(docs[k], bool(flags & 1), bool(flags & NOGC)), (budget, docs[k].name)

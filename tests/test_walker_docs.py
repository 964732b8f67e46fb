"""The walker corpus (walker_docs.py) checked on the CPU: it is deterministic, every family has the items and the labels
its construction says, every item that is meant to be valid is one yjs answers, the placement families really sit at
the residues they name, and the label predicate agrees with labels written by hand."""
import collections

import walker_docs as g
from walker_docs import expected, flat


def counts(batches):
    c = collections.Counter()
    for it in flat(batches):
        c[it[3][0] + it[4][0]] += 1          # "ww": walker in both modes, "we": SV walker / diff exact, ...
    return len(batches), len(flat(batches)), c["ww"], c["we"], c["ew"], c["ee"]


# (batches, items, walker in both modes, walker in SV only, walker in diff only, exact in both)
PINNED = {"A": (12, 2706, 2706, 0, 0, 0), "B": (3, 304, 100, 2, 0, 202), "C": (2, 215, 215, 0, 0, 0), "D": (2, 66, 31, 35, 0, 0),
          "E": (1, 34, 31, 0, 0, 3), "F": (4, 411, 252, 81, 0, 78), "G": (2, 144, 9, 19, 0, 116), "H": (22, 7044, 6265, 0, 0, 779)}


def test_the_corpus_is_deterministic():
    a, b = g.families(), g.families()
    assert a == b
    assert g.family_i() == g.family_i()


def test_item_and_label_counts():
    f = g.families()
    assert {k: counts(v) for k, v in f.items()} == PINNED
    states, ask, items = g.family_i()
    c = collections.Counter(it[4] for it in items)
    assert (len(states), len(ask), c[g.WALKER], c[g.EXACT]) == (12, 778, 744, 34)
    assert sorted(collections.Counter(ask).values()) == sorted(n for n in g.I_ASKS * 2 if n)
    assert ask == sorted(ask)


def test_families_that_split_have_both_labels():
    f = g.families()
    for k in "BDEFGH":
        c = counts(f[k])
        assert c[2] and (c[3] or c[5]), k
    assert counts(f["D"])[3] and counts(f["F"])[3]           # diff alone defers: the state vector, the non-minimal varuints
    labels = {it[4] for it in g.family_i()[2]}
    assert labels == {g.WALKER, g.EXACT}


def test_batches_stay_small():
    for k, bs in g.families().items():
        for b in bs:
            assert len(b) <= 2800 and sum(len(it[1]) for it in b) <= 300000, k
            assert max(len(it[1]) for it in b) <= (40000 if k == "E" else 5100), k


def test_valid_items_are_answered_by_yjs():
    items = flat(sum(g.families().values(), [])) + g.family_i()[2]
    seen = set()
    for it in items:
        if not it[5]:                              # yjs throws on at least one of the two operations
            assert expected(it, "sv")[0] or expected(it, "diff")[0], it[0]
        if not it[5] or (it[1], it[2]) in seen:
            continue
        seen.add((it[1], it[2]))
        assert expected(it, "sv")[0] == 0, it[0]
        assert expected(it, "diff")[0] == 0, it[0]
    assert len(seen) > 1200


def test_placement_probes_sit_at_their_residues():
    a = g.family_a()
    res, off = a[0], g.offsets(a[0])
    names = [p[0] for p in g.probes()]
    seen = collections.defaultdict(set)
    for k, it in enumerate(res):
        if "@" in it[0]:
            name, r = it[0].rsplit(" @", 1)
            assert off[k] % 128 == int(r), it[0]
            seen[name].add(off[k] % 128)
    assert sorted(seen) == sorted(names) and all(v == set(range(128)) for v in seen.values())
    for b, p in zip(a[1:11], g.probes()):
        assert b[-1] == p and len(b) == 2
    sweep, off = a[11], g.offsets(a[11])
    ends = {off[k + 1] % 64 for k, it in enumerate(sweep) if it[0].startswith("A end residue") and off[k] % 64 == 0}
    assert ends == set(range(64))


def test_patterns_sit_at_their_stream_residues():
    f = g.family_f()
    for batch, pat, word in ((f[1], b"\x81\x00", "81 00"), (f[2], b"\xc4\x85\x80\x80\x80\x0f", "C4"), (f[3], b"\x80\x80\x80\x80\x80\x01", "6-byte")):
        off = g.offsets(batch)
        seen = set()
        for k, it in enumerate(batch):
            if word in it[0]:
                at = g.pattern_at(it[1], pat)
                assert len(at) == 1, it[0]
                r = (off[k] + at[0]) % 64
                assert it[0].endswith("residue %d" % r), (it[0], r)
                seen.add(r)
        assert seen == set(range(64)), word
    # the two-byte characters over a chunk seam: first byte at residue 63
    b2 = g.family_b()[1]
    off = g.offsets(b2)
    n = 0
    for k, it in enumerate(b2):
        if "over seam" in it[0]:
            at = g.pattern_at(it[1], "é".encode())
            assert len(at) == 1 and (off[k] + at[0]) % 64 == 63, it[0]
            assert off[k] + at[0] + 1 == int(it[0].rsplit(" ", 1)[1]) + off[k]
            n += 1
    assert n >= 40
    # the state vectors at every residue of their arena
    d = g.family_d()[1]
    off = g.offsets(d, 2)
    assert {off[k] % 16 for k, it in enumerate(d) if "@" in it[0]} == set(range(16))
    assert all(off[k] % 16 == int(it[0].rsplit("@", 1)[1]) for k, it in enumerate(d) if "@" in it[0])


BY_HAND = {  # name: (SV, diff)
    "A 00 00 @0": ("walker", "walker"),
    "B string 5000": ("walker", "walker"),
    "B string 64, two-byte character at 0": ("exact", "exact"),
    "B binary with a 6-run": ("exact", "exact"),
    "B binary with 80 00": ("walker", "exact"),
    "B y-key, content at 59": ("walker", "walker"),
    "B y-key, content at 60": ("exact", "exact"),
    "B type 3 name ends at 64, content at 57": ("walker", "walker"),
    "B type 3 name ends at 65, content at 57": ("exact", "exact"),
    "B type ref 7": ("exact", "exact"),
    "C cut string 1000, origin+right 5-byte ids, offset 257": ("walker", "walker"),
    "D 16 entries": ("walker", "walker"),
    "D 17 entries": ("walker", "exact"),
    "D 160 bytes": ("walker", "walker"),
    "D 161 bytes": ("walker", "exact"),
    "D 16 distinct and a repeat": ("walker", "exact"),
    "D clock 2^32 - 1": ("walker", "walker"),
    "D clock 2^32": ("walker", "exact"),
    "D one trailing byte": ("walker", "exact"),
    "E equal clients": ("exact", "exact"),
    "E a block of 0 structs": ("exact", "exact"),
    "F non-minimal origin clock": ("walker", "exact"),
    "F C4 and a 5-byte client at residue 63": ("walker", "walker"),
    "F 6-byte varuint at residue 61": ("exact", "exact"),
    "F clock + len = 2^32 - 1": ("walker", "walker"),
    "F clock + len = 2^32": ("exact", "exact"),
    "F info 0xA4": ("exact", "exact"),
    "F content any": ("exact", "exact"),
    "G two clients equal": ("walker", "exact"),
    "G a client without ranges": ("walker", "exact"),
    "G 200 ranges": ("walker", "walker"),
}


def test_the_predicate_agrees_with_labels_written_by_hand():
    by_name = {}
    for it in flat(sum(g.families().values(), [])):
        by_name.setdefault(it[0], it)
    for name, want in BY_HAND.items():
        it = by_name[name]
        assert (it[3], it[4]) == want, name

"""CPU check of the corpus the GPU tests feed the wave and workgroup merge tiers (general_tier_docs.py): every
document holds exactly the counts its family names, sits in the tier its label says by the caps restated in
`expected_tier`, is refused by the lean kernels for a stated reason, and is a valid input wherever the family says so."""
import pytest

import oracle
import general_tier_docs as g
from lean_docs import upd
from v1util import encode_ds, rd_vu


def _tiered():
    return [(f, d) for f in g.TIERED for batch in g.families()[f] for d in batch]


def _of(family):
    return [d for batch in g.families()[family] for d in batch]


def test_census_counts_every_record():
    ds = encode_ds([(5, [(0, 1), (0, 1), (3, 0)]), (2 ** 32 - 1, [(7, 2)]), (5, [(1, 1)])])
    us = [upd(9, 4, [g.gc(2), g.skip(3), g.ch(), g.skip(0)], ds=ds), g.update([g.block(9, 0, [g.ch()]), g.block(4, 0, [g.gc(1)])]), g.EMPTY]
    assert g.census(us) == dict(k=3, nbytes=sum(map(len, us)), largest=len(us[0]), S=4, D=5, struct_clients=2, ds_clients=2, defer=False)
    assert g.expected_tier(us) == "wave"
    for bad in ([upd(9, 0, [g.gc(0)]), g.EMPTY],                                           # a zero-length struct
                [upd(2 ** 32, 0, [g.gc(1)]), g.EMPTY],                                      # a client of 33 bits
                [upd(9, 2 ** 32 - 1, [g.gc(1)]), g.EMPTY],                                  # a struct ending at 2^32
                [b"\x00" + encode_ds([(1, [(2 ** 32 - 1, 1)])]), g.EMPTY],                  # a range ending at 2^32
                [g.update([g.block(4, 0, [g.gc(1)]), g.block(9, 0, [g.ch()])]), g.EMPTY],  # clients ascending
                [g.update([g.block(4, 3, [g.gc(1)]), g.block(4, 0, [g.ch()])]), g.EMPTY]):  # clocks descending
        assert g.census(bad)["defer"] and g.expected_tier(bad) == "large", bad


def test_every_document_is_what_its_family_says():
    for fam, d in _tiered():
        if len(d.us) < 2:        # the fillers in front of the residue documents
            assert d.tier is None and fam == "C" and len(d.us[0]) == d.want["nbytes"] < 16
            continue
        c = g.census(d.us)
        for key, v in d.want.items():
            assert c[key] == v, (d.name, key, v, c[key])
        assert g.expected_tier(d.us) == d.tier, (d.name, d.tier, c)
        assert d.valid and oracle.merge_updates(d.us)[0] == 0, d.name


def _lean_refusal(us):
    c = g.census(us)
    kinds = {s[2] for u in us for s in g.walk(u)[0]}
    return bool(kinds & {"gc", "skip"}) or c["struct_clients"] >= 9 or c["largest"] > 64 or c["D"] > 64


def test_the_lean_kernels_refuse_every_document():
    for fam, d in _tiered():
        if len(d.us) >= 2:
            assert _lean_refusal(d.us), d.name
    for d in _of("F noncanon"):
        assert _lean_refusal(d.us), d.name
    for d in _of("B invalid"):     # (the GC stands in one of the first two updates, the one that is not broken)
        assert any(s[2] == "gc" for u in d.us[:2] if oracle.merge_updates([u, g.EMPTY])[0] == 0 for s in g.walk(u)[0]), d.name


def _values(family, key, **where):
    return sorted({d.want[key] for d in _of(family) if key in d.want and all(d.want.get(k) == v for k, v in where.items())})


def test_the_families_cover_the_named_sizes():
    assert _values("A", "S") == [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 511, 512, 513]
    assert set(_values("A", "struct_clients")) >= {1, 8, 9, 63, 64, 65}
    for S in _values("A", "S"):
        assert {d.name.split()[-1] for d in _of("A") if d.want["S"] == S} == {"log", "reversed", "shuffled"}
    ids = {s[0] for d in _of("A") for u in d.us for s in g.walk(u)[0]}
    assert 0 in ids and 2 ** 32 - 1 in ids and any(127 < i < 2 ** 28 for i in ids)
    assert _values("B", "k") == [2, 63, 64, 65, 255, 256, 257]
    assert _values("C", "nbytes")[-6:] == [8175, 8176, 8177, 16383, 16384, 16385] and _values("C", "largest") == [1023, 1024]
    res = g.residues(g.families()["C"][1])
    assert res == {8176: set(range(16)), 8177: set(range(16))}
    assert set(_values("G", "D")) >= {1, 64, 65, 127, 128, 129, 255, 256, 257}
    assert set(_values("G", "ds_clients")) >= {1, 63, 64, 65}
    assert any(d.want.get("S") == 0 for d in _of("G")) and any(d.want.get("S") != 0 for d in _of("G"))
    labels = {f: {d.tier for d in _of(f)} for f in g.TIERED}
    assert all(labels[f] >= {"wave", "workgroup"} for f in "ACDFG") and all("large" in labels[f] for f in "ABCEFG")


def test_invalid_updates_throw_and_sit_where_the_family_says():
    for d in _of("B invalid"):
        assert len(d.us) == 256 and oracle.merge_updates(d.us)[0] in (1, 2), d.name
    at = {int(d.name.split()[-1]) for d in _of("B invalid") if " and " not in d.name}
    assert at == {0, 63, 64, 255}
    assert {st for st in (oracle.merge_updates(d.us)[0] for d in _of("B invalid"))} == {1, 2}


def test_gc_runs_sit_on_the_lane_block_edges():
    """Sorted positions of the GCs of each family-D run document (one client: sorted position = struct index in clock
    order): runs of every length 2-6 cross 4l - 1 | 4l for l = 1, 16, 32, 63 and 255 | 256, and all 32 boundary
    patterns of the six-GC run are there."""
    crossings = set()
    for d in _of("D"):
        if not (d.name.startswith("D run ") and d.name.split()[2].isdigit()):
            continue
        structs = sorted(s for u in d.us for s in g.walk(u)[0] if s[2] != "skip")
        pos = [i for i, s in enumerate(structs) if s[2] == "gc"]
        n = int(d.name.split()[2])
        assert len(pos) == n and pos == list(range(pos[0], pos[0] + n)), d.name
        crossings |= {(n, p) for p in pos[1:] if p % 4 == 0}
    for n in range(2, 7):
        assert {p for m, p in crossings if m == n} >= {4, 64, 128, 252, 256}, n
    six = [d for d in _of("D") if d.name.startswith("D run 6 pattern") and "reversed" not in d.name]
    assert len({tuple(len(g.walk(u)[0]) for u in d.us) for d in six}) == 32
    changes = sorted(len(g.walk(d.us[0])[0]) for d in _of("D") if d.name.startswith("D 256 GCs") and "reversed" not in d.name)
    assert changes == [1, 3, 4, 5, 63, 64, 127, 128, 200, 255]


def test_skip_lengths_take_one_to_five_bytes():
    outs = {}
    for d in _of("E"):
        if d.name.startswith("E gap ") and "reversed" not in d.name and d.tier == "wave":
            st, out = oracle.merge_updates(d.us)
            gap = int(d.name.split()[2])
            assert st == 0 and b"\x0a" + g.vu(gap) in out, d.name
            outs.setdefault(len(g.vu(gap)), []).append(gap)
    assert {n: len(v) for n, v in outs.items()} == {1: 2, 2: 2, 3: 2, 4: 2, 5: 2}
    last = g.find("E", "E gap %d" % (2 ** 32 - 4))
    assert max(s[1] + s[3] for u in last.us for s in g.walk(u)[0]) == 2 ** 32 - 1
    over = g.find("E", "E gap ends at 2^32")
    assert max(s[1] + s[3] for u in over.us for s in g.walk(u)[0]) == 2 ** 32 and over.tier == "large"


def test_odd_structs_keep_the_clocks_contiguous():
    """The clock lengths the corpus gives its odd structs are the oracle's: the merged document of every family-F
    document has one block per client and no Skip (its state vector ends at the sum of the lengths)."""
    for d in _of("F"):
        st, out = oracle.merge_updates(d.us)
        total = sum(s[3] for u in d.us for s in g.walk(u)[0] if s[0] == g.HI)
        st2, sv = oracle.encode_state_vector_from_update(out)
        assert st == 0 and st2 == 0, d.name
        n, p = rd_vu(sv, 0)
        clocks = {}
        for _ in range(n):
            c, p = rd_vu(sv, p)
            clocks[c], p = rd_vu(sv, p)
        assert clocks[g.HI] == total, (d.name, clocks, total)
        assert sum(1 for s in g.walk(out)[0] if s[2] == "skip") == 0, d.name
    names = {d.name.split(" at ")[0] for d in _of("F")}
    assert len(names) == len(g.ODD) + 2
    refs = {o[1][0] & 31 for o in g.ODD}
    assert refs >= set(range(1, 10))


def test_delete_set_order_differs_under_compat135():
    multi = [d for d in _of("G") if d.want["ds_clients"] > 1]
    differ = sum(1 for d in multi if oracle.merge_updates(d.us) != oracle.merge_updates(d.us, compat135=True))
    assert len(multi) >= 12 and 3 * differ >= len(multi), (differ, len(multi))


def test_reuse_batches_alternate_full_and_empty():
    wave, work = g.reuse_batches()
    assert all(d.tier in ("wave", None) for d in wave) and all(d.tier == "workgroup" for d in work)
    cw = [g.census(d.us) for d in wave if d.valid]
    assert max(c["S"] for c in cw) == 256 and min(c["S"] for c in cw) == 0
    assert max(c["D"] for c in cw) == 128 and max(c["struct_clients"] for c in cw) == 64
    assert max(c["nbytes"] for c in cw) == 8176 and 40 in [c["nbytes"] for c in cw]
    assert any(not d.valid for d in wave)
    ck = [g.census(d.us) for d in work]
    assert max(c["S"] for c in ck) == 512 and max(c["D"] for c in ck) == 256 and max(c["nbytes"] for c in ck) == 16384


@pytest.mark.parametrize("family", g.PARITY_ONLY)
def test_parity_only_families_carry_no_tier(family):
    assert all(d.tier is None and not d.valid for d in _of(family))

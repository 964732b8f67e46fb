"""CPU check of the corpus the GPU tests feed the large-document merge tier (large_tier_docs.py): every document reaches
the tier by its size, a byte-level walker re-finds each placed struct where its name says (U0 offset, byte length, clock
length, block struct count, tile and chunk offsets), the census of the log gives the labelled outcome by the caps
restated in `expected_outcome`, and every labelled document is a valid input."""
import pytest

import oracle
import large_tier_docs as g


def _tiered():
    return [(f, d) for f in g.TIERED for batch in g.families()[f] for d in batch]


def _of(family):
    return [d for batch in g.families()[family] for d in batch]


def _multi(family):
    return [d for d in _of(family) if len(d.us) >= 2]


def _structs(d):
    u = d.us[g.pick_u0(d.us)]
    blocks, ds0, ds = g.layout(u)
    return u, blocks, {s["off"]: (s, B) for B in blocks for s in B["structs"]}


def test_census_and_outcome_rules():
    u0 = g.base_u0()
    assert len(u0) == 1100 and g.pick_u0([b"\x00\x00", u0, u0]) == 1
    c = g.census([g.upd(g.LOGC, 0, [g.ch(), g.gc(2)], ds=g.encode_ds([(5, [(0, 1), (3, 1)])])), u0, b"\x00\x00"])
    assert (c["u0"], c["n0"], c["S"], c["D"], c["log_updates"], c["nb"], c["ds_clients"], c["reasons"]) == (1, 1100, 2, 2, 2, 1, 1, [])
    assert g.scan_contrib([u0, b"\x00\x00"]) == dict(positions=1120, tasks=1, slow_queue=0)
    assert g.scan_contrib([g.one_block([g.FILL], total=4097)[0]])["tasks"] == 2
    for n, out in ((256, ("mid", False)), (257, ("mid_to_wide", False)), (1024, ("mid_to_wide", False)), (1025, ("seq", True))):
        assert g.expected_outcome([u0] + g.chars(g.LOGC, 0, n)) == out
        assert g.expected_outcome([u0] + g.ds_only(g.LOGC, 0, n)) == out
    # a log the tier refuses stays with the mid size (it defers before it counts the caps)
    assert g.expected_outcome([u0] + g.chars(g.LOGC, 0, 300) + [g.upd(9, 0, [g.skip(2), g.ch()])]) == ("seq", False)
    assert g.expected_outcome([u0, g.upd(g.C0, 5, [g.ch()])]) == ("seq", False)          # overlap
    assert g.expected_outcome([u0], compat135=True) == ("mid", False)
    assert g.expected_outcome([g.base_u0(ds=g.encode_ds([(1, [(0, 1)]), (0, [(0, 1)])])), b"\x00\x00"], compat135=True) == ("seq", False)


def test_every_document_reaches_the_tier_and_is_what_its_label_says():
    for fam, d in _tiered():
        if len(d.us) < 2:         # the fillers in front of the residue documents
            assert d.outcome is None and fam == "W" and len(d.us[0]) == d.want["nbytes"] < 16
            continue
        assert d.outcome in g.OUTCOMES, d.name                      # (a condition: no tiered document without a label)
        assert max(len(u) for u in d.us) >= g.ROUTE, d.name
        assert d.valid and oracle.merge_updates(d.us)[0] == 0, d.name
        assert g.expected_outcome(d.us, noncanon=d.want.get("noncanon", False)) == (d.outcome, d.via_wide), d.name
        if d.seq135:
            assert g.expected_outcome(d.us, compat135=True)[0] == "seq", d.name
        c = g.census(d.us)
        for key in ("n0", "S", "D", "log_updates", "log_bytes", "nb", "u0"):
            if key in d.want:
                assert c[key] == d.want[key], (d.name, key, c[key], d.want[key])


def test_placed_structs_are_where_their_names_say():
    seen = 0
    for fam, d in _tiered():
        if not d.placed:
            continue
        u, blocks, at = _structs(d)
        for name, r in d.placed.items():
            s, B = at[r["off"]]
            seen += 1
            assert (s["nbytes"], s["clock"], s["clen"]) == (r["nbytes"], r["clock"], r["clen"]), (d.name, name, s, r)
            assert B is blocks[r["block"]] and B["structs"][r["index"]] is s, (d.name, name)
        for key in ("off", "nbytes", "clen"):
            for name, v in d.want.get(key, {}).items():
                assert d.placed[name][key] == v, (d.name, name, key, d.placed[name][key], v)
        for name in d.want.get("last_in_block", []):
            r = d.placed[name]
            assert r["index"] == blocks[r["block"]]["nst"] - 1, (d.name, name)
        for name in d.placed:
            if name.startswith("mid "):
                r = d.placed[name]
                assert 0 < r["index"] < blocks[r["block"]]["nst"] - 1, (d.name, name)
    assert seen > 100


def test_scan_family_covers_the_named_edges():
    S = _of("S")
    assert sorted(d.want["n0"] for d in S if d.name.startswith("S n0=")) == [4095, 4096, 4097, 8191, 8192, 8193]
    starts = sorted(d.placed["x"]["off"] for d in S if d.name.startswith("S struct starts at"))
    assert [(a % g.SCAN_CH) % g.WCH for a in starts] == [g.WCH - 1, 0, g.WCH - 1, 0] and starts[2] // g.SCAN_CH == 1
    over = {}
    for d in S:
        if d.name.startswith("S string from") and "past the stage" in d.name:
            r = d.placed["x"]
            w0 = r["off"] // g.WCH * g.WCH
            assert g.WCH - 24 <= r["off"] - w0 < g.WCH and len(d.us[0]) > w0 + g.WCH + g.MARGIN      # (the stage ends before n0)
            over.setdefault(w0, []).append(r["off"] + r["nbytes"] - (w0 + g.WCH + g.MARGIN))
    assert over == {0: [0, 1, 300], g.SCAN_CH + g.WCH: [0, 1, 300]}
    for d in S:
        if d.name.endswith("ends at n0 - 1"):
            r = d.placed["x"]
            assert r["off"] + r["nbytes"] == len(d.us[0]) - 1 and len(d.us[0]) < r["off"] // g.WCH * g.WCH + g.WCH + g.MARGIN
    sizes = {}
    for d in S:
        if "63 / 64 / 65" in d.name:
            u, blocks, at = _structs(d)
            for name, r in d.placed.items():
                info = at[r["off"]][0]["info"]
                sizes.setdefault((g.first_class(info), info & 31, name.split()[0]), set()).add(r["nbytes"])
    want = {g.VCAP - 1, g.VCAP, g.VCAP + 1}
    assert sizes[(True, 4, "string")] == want
    for ref in (2, 3, 4, 5, 6, 7, 8):
        assert sizes[(False, ref, "mid")] == want and sizes[(False, ref, "last")] == want, ref
    # the queued structs are counted by the slow queue's lower bound; the last of a block is followed by a header
    for kind in g.SECOND_CLASS:
        d = g.find("S", "S second class %s 63 / 64 / 65" % kind)
        low = g.scan_contrib(d.us)["slow_queue"]
        assert low == (0 if kind == "json9" else 2), (kind, low)          # (the two mid-block ones of at most VCAP bytes)
        u = d.us[0]
        for name in d.want["last_in_block"]:
            r = d.placed[name]
            assert not g.big_cand(u[r["off"] + r["nbytes"]]), (kind, name)
    assert {d.placed["x"]["nbytes"] for d in S if d.name.startswith("S struct of")} == {g.LEN15 - 1, g.LEN15}
    clens = sorted(d.placed["gc"]["clen"] for d in S if d.name.startswith("S clock length"))
    assert clens == [g.V16_MAX, g.V16_MAX + 1, g.V16_MAX + 2] == [65534, 65535, 65536]
    d = g.find("S", "S ASCII strings of 1-17 bytes")
    assert sorted(r["clen"] for r in d.placed.values()) == list(range(1, 18))
    d = g.find("S", "S UTF-8 strings")
    u, blocks, at = _structs(d)
    differ = [r for r in d.placed.values() if r["clen"] != r["nbytes"] - (3 if at[r["off"]][0]["info"] & 0x80 else 4) - 1]
    assert len(differ) == len(d.placed)          # UTF-16 length differs from the byte length in every one
    for n in (0, 1, 2):
        d = g.find("S", "S parentInfo %d" % n)
        assert d.us[0][d.placed["x"]["off"]] == 4 and d.us[0][d.placed["x"]["off"] + 1] == n
    assert all(not d.valid and d.outcome is None and oracle.merge_updates(d.us)[0] != 0 for d in _of("S oracle decides"))


def test_pick_family_covers_the_named_edges():
    P = g.families()["P"]
    assert [len(b) for b in P[:4]] == [g.PICK - 1, g.PICK, g.PICK + 1, 2 * g.PICK + 1]
    lists = [{("wide" if len(d.us[g.pick_u0(d.us)]) > g.MID_U0 else "mid") for d in b} for b in P]
    assert {"wide", "mid"} in lists and {"wide"} in lists and {"mid"} in lists
    big = g.big_docs()
    assert [len(d.us[0]) for d in big[:2]] == [g.MID_U0, g.MID_U0 + 1] == [524288, 524289]
    for d in big[2:]:
        u = d.us[0]
        nb = g.rd_vu(u, 0)[0]
        assert len(u) > g.MID_U0 and (nb * 256 > len(u)) == d.want["use_bh"], d.name
    assert sum(1 for f in g.TIERED for d in _of(f) if max(map(len, d.us)) > 100000) <= 8       # (the four, in three batches)
    eq = P[6]
    for d in eq:
        sizes = [len(u) for u in d.us]
        assert sizes.count(max(sizes)) == 2 and g.pick_u0(d.us) == d.want["u0"] == sizes.index(max(sizes))
    assert {d.outcome for d in eq} == {"mid", "mid_to_wide"}


def test_log_family_covers_the_named_edges():
    L = _of("L")
    assert sorted(d.want["S"] for d in L if d.name.endswith("log structs")) == [256, 257, 1024, 1025]
    assert sorted(d.want["D"] for d in L if d.name.endswith("log ranges")) == [256, 257, 1024, 1025]
    assert sorted(d.want["log_updates"] for d in L if d.name.endswith("log updates")) == [g.LG_LIST, g.LG_LIST + 1]
    assert (g.LG_CAP_M, g.LG_CAP_W) == (9296, 49232)
    by = sorted(d.want["log_bytes"] for d in L if d.name.startswith("L log of"))
    assert by == [g.LG_CAP_M, g.LG_CAP_M + 1, g.LG_CAP_W, g.LG_CAP_W + 1]
    one = sorted(max(len(u) for u in d.us[1:]) for d in L if d.name.startswith("L one log update"))
    assert one == [g.LG_CAP_M - 1, g.LG_CAP_M, g.LG_CAP_M + 1, g.LG_CAP_W - 1, g.LG_CAP_W, g.LG_CAP_W + 1]
    assert {d.outcome for d in L} == {"mid", "mid_to_wide", "seq"}


def test_walk_family_covers_the_named_edges():
    W = g.families()["W"]
    assert g.residues(W[1]) == set(range(16))
    for ch_ in (g.TILE_M, g.TILE_W):       # the first tile holds U0 positions [1, 1 + CH): its last byte is position CH
        d = g.find("W", "W client varuint across the last byte of the %d tile" % ch_)
        blocks = g.layout(d.us[0])[0]
        h0 = blocks[1]["h0"]
        assert h0 == ch_ - 1 and len(g.vu(blocks[1]["client"])) == 5 and h0 + 1 <= ch_ < h0 + 6
        for name in ("W struct starts on the last byte of the %d tile", "W 0xA8 struct on the last byte of the %d tile"):
            d = g.find("W", name % ch_)
            assert d.placed["x"]["off"] == ch_ and g.layout(d.us[0])[0][0]["h0"] == 1
        assert (d.outcome == "mid") == (ch_ == g.TILE_M)       # the wide size's tile is walked after a hand-on
    for name in ("W blocks of 1-129 structs", "W blocks of 1-129 structs, block table"):
        d = g.find("W", name)
        blocks = g.layout(d.us[0])[0]
        assert [B["nst"] for B in blocks] == d.want["nst"] and d.want["nst"][:7] == [1, 63, 64, 65, 127, 128, 129]
        assert (len(blocks) * 256 > len(d.us[0])) == d.want["use_bh"]
    for d in W[0]:
        if d.name.startswith("W 8 blocks of"):
            assert (g.census(d.us)["nb"] * 256 > len(d.us[0])) == d.want["use_bh"] and len(d.us[0]) in (8 * 255, 8 * 257)
    d = g.find("W", "W 400 empty client blocks")
    assert g.census(d.us)["nb"] > len(d.us[0]) // 4 + 1
    d = g.find("W", "W 0xA8 structs at bits 31, 0 and 1")
    assert sorted(r["off"] % 32 for r in d.placed.values()) == [0, 0, 1, 1, 31, 31]
    assert all(d.us[0][r["off"]] == 0xA8 for r in d.placed.values())
    assert {x.outcome for x in W[0]} == set(g.OUTCOMES) - {"wide_first"}
    one, two, two_u0 = g.ds_pair()
    assert not one.seq135 and two.seq135 and two_u0.seq135
    assert oracle.merge_updates(two.us) != oracle.merge_updates(two.us, compat135=True)


def test_reuse_sequences():
    seqs = g.reuse_sequences()
    rich, one, plain, again = seqs["stale pbits"]
    for a, b, c in zip(rich, plain, one):
        assert [len(u) for u in a.us] == [len(u) for u in b.us] == [len(u) for u in c.us]
        ua, ub, uc = a.us[0], b.us[0], c.us[0]
        at = [s["off"] for B in g.layout(ua)[0] for s in B["structs"] if s["info"] == 0xA8]
        assert len(at) >= 40 and all(ub[p] == 0x28 for p in at)
        assert sum(1 for p in at if uc[p] == 0xA8) == 1 and sum(1 for p in at if uc[p] == 0x28) == len(at) - 1
    grow = seqs["grow-only scratch"]
    assert sum(len(u) for d in grow[0] for u in d.us) > 50 * sum(len(u) for d in grow[1] for u in d.us)
    lists = [{len(d.us[g.pick_u0(d.us)]) > g.MID_U0 for d in b} for b in seqs["stream reuse"]]
    assert lists == [{True, False}, {False}, {True}, {False}]
    for batches in seqs.values():
        for b in batches:
            for d in b:
                assert d.outcome in g.OUTCOMES and g.expected_outcome(d.us) == (d.outcome, d.via_wide), d.name


@pytest.mark.parametrize("family", g.PARITY_ONLY)
def test_parity_only_families_carry_no_outcome(family):
    assert all(d.outcome is None and not d.valid for d in _of(family))
    assert all(max(len(u) for u in d.us) >= g.ROUTE and len(d.us) >= 2 for d in _of(family))       # (they reach the tier)

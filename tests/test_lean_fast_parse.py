"""The narrow lean merge kernel on the single-Item debounce shape and around it: row edges of the lane-per-update
parse, one odd update inside a row of plain ones, every varuint length, clock gaps / overlaps at the places a
per-block contiguity check can miss, and more documents than the persistent grid.  Every document is compared
with the CPU oracle; the tests describe behaviour (what is finished by the lean kernel, what is exact), not how
the kernel parses."""
import random

import pytest

from devrun import Memo, engine_fixture, run_merge, same
from lean_docs import CLIENTS, Log, fast_doc, item, text, upd
from v1util import vu

pytestmark = pytest.mark.gpu

eng = engine_fixture()
MEMO = Memo()
expect = MEMO.expect


def check(eng, key, docs, form, lean=None):
    exp = expect(key, docs)
    res, took = run_merge(eng, docs, form)
    bad = [d for d in range(len(docs)) if not same(exp[d], res[d])]
    assert not bad, (key, form, len(bad), bad[:5], [u.hex() for u in docs[bad[0]]][:8])
    if lean is not None:
        assert took == lean, (key, form, took, lean)
    return took


# ---- row edges
ROW_K = [2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 254, 255]


def _row_edge_docs():
    docs = []
    for ncl in (1, 2, 4, 5, 8):
        for k in ROW_K:
            docs.append(fast_doc(k, CLIENTS[:ncl], seed=k * 10 + ncl))
    return docs


@pytest.mark.parametrize("form", ["off", "lens"])
def test_row_edges_all_fast(eng, form):
    docs = _row_edge_docs()
    assert all(st == 0 for st, _ in expect("rows", docs))
    check(eng, "rows", docs, form, lean=len(docs))


# ---- one intruder in a row of fast updates
INTRUDER_AT = [0, 1, 63, 64, 65, 127, 128, 129]
A, B = 5, 9     # one-byte client ids: room for the long shapes inside 32 bytes


def _intruder_doc(i, shape):
    """130 updates of clients A / B (alternating); update i has the named shape."""
    g = Log([A, B], [5, 5], seed=i)
    for j in range(130):
        c = (A, B)[j % 2]
        if j != i:
            g.plain(c)
            continue
        o = g.last or (B, 1)
        if shape == "ykey":
            g.put(c, [item(4, text("q"))], 1)
        elif shape == "ykey_sub":
            g.put(c, [item(4, text("q"), sub=b"key")], 1)
        elif shape == "parent_id":
            g.put(c, [item(4, text("q"), parent=b"\x00" + vu(B) + vu(2))], 1)
        elif shape == "deleted":
            g.put(c, [item(1, vu(3), origin=o)], 3)
        elif shape in ("structs2", "structs3"):
            n = int(shape[-1])
            ck = g.clock[c]
            g.put(c, [item(4, text("q"), origin=o)] + [item(4, text("r"), origin=(c, ck + s)) for s in range(n - 1)], n)
        elif shape in ("str2", "str5", "str20"):
            n = int(shape[3:])
            g.put(c, [item(4, text("abcdefghijklmnopqrst"[:n]), origin=o)], n)
        elif shape == "insert_ds":
            g.put(c, [item(4, text("q"), origin=o)], 1, ds=b"\x01" + vu(B) + b"\x01" + vu(1) + vu(1))
        elif shape == "ds_only":
            g.raw(b"\x00\x01" + vu(A) + b"\x01" + vu(6) + vu(1))
        # ---- shapes outside the envelope
        elif shape == "nonmin_client":
            g.put(c, [item(4, text("q"), origin=o)], 1, client_bytes=bytes([c | 0x80, 0]))
        elif shape == "nonmin_clock":
            g.put(c, [item(4, text("q"), origin=o)], 1, clock_bytes=bytes([g.clock[c] | 0x80, 0]))
        elif shape == "nonmin_origin":
            g.put(c, [item(4, text("q"), origin=vu(o[0]) + bytes([o[1] | 0x80, 0]))], 1)
        elif shape == "non_ascii":
            g.put(c, [item(4, text("é"), origin=o)], 1)
        elif shape == "client_2_32":
            g.clock[2 ** 32 + 1] = 0
            g.put(2 ** 32 + 1, [item(4, text("q"), origin=o)], 1)
        elif shape == "flag20_origin":
            g.put(c, [item(4, text("q"), origin=o, flag20=True)], 1)
        elif shape == "bytes33":
            s = item(4, text("a" * 24), origin=o)
            g.put(c, [s], 24)
            assert len(g.ups[-1]) == 33
        elif shape == "trailing":
            g.put(c, [item(4, text("q"), origin=o)], 1, tail=b"\x07\x07")
        elif shape == "gap":
            g.put(c, [item(4, text("q"), origin=o)], 1, shift=1)
        elif shape == "overlap":
            g.put(c, [item(4, text("q"), origin=o)], 1, shift=-1)
        else:
            raise ValueError(shape)
    assert all(len(u) <= 32 for u in g.ups) or shape == "bytes33"
    return g.ups


LEAN_SHAPES = ["ykey", "ykey_sub", "parent_id", "deleted", "structs2", "structs3", "str2", "str5", "str20", "insert_ds", "ds_only"]
DEFER_SHAPES = ["nonmin_client", "nonmin_clock", "nonmin_origin", "non_ascii", "client_2_32", "flag20_origin", "bytes33",
                "trailing", "gap", "overlap"]


def test_intruder_inside_the_envelope_stays_lean(eng):
    docs = [_intruder_doc(i, s) for s in LEAN_SHAPES for i in INTRUDER_AT]
    assert all(st == 0 for st, _ in expect("intr_lean", docs))
    check(eng, "intr_lean", docs, "lens", lean=len(docs))
    check(eng, "intr_lean", docs, "off", lean=len(docs))


def test_intruder_outside_the_envelope_is_exact(eng):
    docs = [_intruder_doc(i, s) for s in DEFER_SHAPES for i in INTRUDER_AT]
    check(eng, "intr_defer", docs, "lens")
    check(eng, "intr_defer", docs, "off")


# ---- every varuint length inside the fast shape
VU_CLIENTS = [1, 127, 128, 2 ** 14, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 32 - 1]


def _varuint_docs():
    docs = [fast_doc(40, VU_CLIENTS, seed=1)]                                  # all eight in one document
    docs += [fast_doc(12, [c], seed=c & 0xFFFF) for c in VU_CLIENTS]           # each alone
    # document clocks and origin clocks crossing 127 -> 128 and 16 383 -> 16 384
    docs.append(fast_doc(30, [77, 2 ** 28], [120, 16376], seed=2))
    docs.append(fast_doc(200, [2 ** 32 - 1], [16300], seed=3))
    docs.append(fast_doc(24, [128, 127, 2 ** 21], [2 ** 21 - 4, 2 ** 28 - 9, 2 ** 14 - 3], seed=4))
    # updates of exactly 31 and 32 bytes: 5-byte clients, clock / origin clock / right-origin clock of 4 + 3 + 3
    # and 4 + 4 + 3 bytes
    for n, (ock, rck) in ((31, (2 ** 14 + 9, 2 ** 14 + 3)), (32, (2 ** 21 + 9, 2 ** 14 + 3))):
        c, ck = 2 ** 32 - 1, 2 ** 21 + 5
        ups = [upd(c, ck, [item(4, text("a"))])]
        for j in range(1, 70):
            ups.append(upd(c, ck + j, [item(4, text("b"), origin=(2 ** 31, ock), right=(2 ** 30, rck))]))
            assert len(ups[-1]) == n, len(ups[-1])
        docs.append(ups)
    return docs


def test_varuint_lengths_in_the_fast_shape(eng):
    docs = _varuint_docs()
    assert all(st == 0 for st, _ in expect("vu", docs))
    check(eng, "vu", docs, "lens", lean=len(docs))
    check(eng, "vu", docs, "off", lean=len(docs))


# ---- contiguity: gaps and overlaps where a check by sorted neighbours or by log neighbours can go wrong
def _contig_doc(ncl, where, shift, seed):
    """Client 0 of CLIENTS[:ncl] sorted descending (the first block) writes updates 0..69, the other clients follow
    round robin, four updates each.  `where`: 'second' (the second record of the last block), 'row' (record 64 of the
    first block: update 64 of the log), 'first_last' (the first record of the last block gets the clock one past /
    short of the END of the block sorted before it -- contiguous with nothing, which is no gap), None (clean)."""
    cl = sorted(CLIENTS[:ncl], reverse=True)
    g = Log(cl, [7] * ncl, seed)
    lastc = cl[-1]
    seen_last = 0
    n_first = 70 if ncl > 1 else 74
    for j in range(n_first + 4 * (ncl - 1)):
        c = cl[0] if j < n_first else cl[1 + (j - n_first) % (ncl - 1)]
        sh = 0
        if c == lastc:
            if where == "second" and seen_last == 1:
                sh = shift
            if where == "first_last" and seen_last == 0 and ncl > 1:
                sh = 7 + 4 + shift - g.clock[c]     # (every client but the first starts at 7 and writes four characters)
            seen_last += 1
        if where == "row" and j == 64:
            sh = shift
        if sh:   # this update's clock, and the client's later ones, shifted
            g.put(c, [item(4, text("z"), origin=g.last)], 1, shift=sh)
        else:
            g.plain(c)
    return g.ups


@pytest.mark.parametrize("ncl", [1, 4, 5, 8])
def test_contiguity_gaps_and_overlaps(eng, ncl):
    docs, broken = [], []
    for where in ("second", "row", "first_last"):
        for shift in (1, -1):
            if where == "first_last" and ncl == 1:
                continue
            docs.append(_contig_doc(ncl, None, 0, seed=len(docs)))          # a clean neighbour on each side
            docs.append(_contig_doc(ncl, where, shift, seed=len(docs)))
            broken.append(where != "first_last")
    docs.append(_contig_doc(ncl, None, 0, seed=99))
    key = "contig%d" % ncl
    n_lean = len(docs) - sum(broken)    # the neighbours, and the documents whose odd clock starts a block
    for form in ("lens", "off"):
        check(eng, key, docs, form, lean=n_lean)


# ---- more documents than the persistent grid: every wave takes a second document
def test_more_documents_than_the_grid(eng):
    rng = random.Random(12)
    docs = [fast_doc(2 + d % 4, [rng.randrange(1, 2 ** 32) for _ in range(1 + d % 3)], seed=d) for d in range(4500)]
    check(eng, "grid", docs, "lens", lean=len(docs))
    check(eng, "grid", docs, "off", lean=len(docs))

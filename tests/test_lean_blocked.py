"""The lean merge kernels with four updates per lane in a blocked layout (lane l owns updates 4l .. 4l+3): every
document length, one odd update at the lane and DPP-row boundaries, the first-seen delete-set order of yjs 13.5 across
those boundaries, and the sequencing of a wave's documents of every kind.  Every document is compared with the CPU
oracle, and every test asserts how many documents the lean kernels finished, so none passes by deferring."""
import pytest

import oracle
from devrun import Memo, engine_fixture, run_merge, same
from lean_docs import CLIENTS, Log, _ds, fast_doc, item, text, upd
from v1util import vu

pytestmark = pytest.mark.gpu

FORMS = ["off", "lens"]


eng = engine_fixture()
eng135 = engine_fixture(compat135=True)
MEMO = Memo()
expect = MEMO.expect


def check(e, exp, docs, form, lean, wide=None):
    w0 = e.stats().docs_lean_wide
    res, took = run_merge(e, docs, form)
    bad = [d for d in range(len(docs)) if not same(exp[d], res[d])]
    assert not bad, (form, len(bad), bad[:5], [u.hex() for u in docs[bad[0]]][:8])
    assert took == lean, (form, took, lean)
    if wide is not None:
        assert e.stats().docs_lean_wide - w0 == wide, (form, e.stats().docs_lean_wide - w0, wide)


# ---- 1. every document length
def _length_docs():
    return [fast_doc(k, CLIENTS[:ncl], seed=k * 10 + ncl) for ncl in (1, 3, 8) for k in range(2, 256)]


@pytest.mark.parametrize("form", FORMS)
def test_every_document_length_finishes_lean(eng, form):
    docs = _length_docs()
    exp = expect("lengths", docs)
    assert all(st == 0 for st, _ in exp)
    check(eng, exp, docs, form, lean=len(docs))


# ---- 2. one odd update at the lane boundaries (multiples of 4) and the DPP row boundaries (64 / 128 / 192)
ODD_AT = list(range(0, 9)) + [63, 64, 65, 127, 128, 129, 191, 192, 193, 251, 252, 253, 254]
A, B = 5, 9     # one-byte client ids: the long shapes fit in 32 bytes, the document in the staged bytes
ODD_K = 255


def _odd_doc(i, shape):
    """255 updates of clients A / B (alternating); update i has the named shape."""
    g = Log([A, B], [5, 5], seed=i)
    for j in range(ODD_K):
        c = (A, B)[j % 2]
        if j != i:
            g.plain(c)
            continue
        o = g.last or (B, 1)
        if shape == "deleted":
            g.put(c, [item(1, vu(3), origin=o)], 3)
        elif shape == "structs3":
            ck = g.clock[c]
            g.put(c, [item(4, text("q"), origin=o)] + [item(4, text("r"), origin=(c, ck + s)) for s in range(2)], 3)
        elif shape == "str20":
            g.put(c, [item(4, text("abcdefghijklmnopqrst"), origin=o)], 20)
        elif shape == "insert_ds":
            g.put(c, [item(4, text("q"), origin=o)], 1, ds=b"\x01" + vu(B) + b"\x01" + vu(1) + vu(1))
        elif shape == "ds_only":
            g.raw(b"\x00\x01" + vu(A) + b"\x01" + vu(6) + vu(1))
        elif shape == "bytes33":
            # one byte past the narrow kernel's 32-byte window (clock and origin lengths vary with the position)
            m = next(m for m in range(1, 32) if len(upd(c, g.clock[c], [item(4, text("a" * m), origin=o)])) == 33)
            g.put(c, [item(4, text("a" * m), origin=o)], m)
            assert len(g.ups[-1]) == 33, len(g.ups[-1])
        elif shape == "gap":
            g.put(c, [item(4, text("q"), origin=o)], 1, shift=1)
        elif shape == "overlap":
            g.put(c, [item(4, text("q"), origin=o)], 1, shift=-1)
        else:
            raise ValueError(shape)
    assert all(len(u) <= 32 for u in g.ups) or shape == "bytes33"
    assert sum(len(u) for u in g.ups) + 16 <= 5120     # staged whole by the narrow kernel (and under the wide one's 7 168)
    return g.ups


@pytest.mark.parametrize("shape", ["deleted", "structs3", "str20", "insert_ds", "ds_only"])
def test_odd_update_at_the_boundaries_stays_lean(eng, shape):
    docs = [_odd_doc(i, shape) for i in ODD_AT]
    exp = expect("odd_" + shape, docs)
    assert all(st == 0 for st, _ in exp)
    for form in FORMS:
        check(eng, exp, docs, form, lean=len(docs), wide=0)


@pytest.mark.parametrize("shape", ["gap", "overlap"])
def test_odd_clock_at_the_boundaries_is_exact(eng, shape):
    docs = [_odd_doc(i, shape) for i in ODD_AT]
    exp = expect("odd_" + shape, docs)
    # updates 0 and 1 are their clients' first: a shifted first clock is contiguous with nothing, so those two
    # documents stay lean; every later position breaks its client's contiguity and leaves the lean kernels
    n_lean = sum(1 for i in ODD_AT if i < 2)
    for form in FORMS:
        check(eng, exp, docs, form, lean=n_lean)


def test_long_update_at_the_boundaries_takes_the_wide_kernel(eng):
    docs = [_odd_doc(i, "bytes33") for i in ODD_AT]
    exp = expect("odd_bytes33", docs)
    assert all(st == 0 for st, _ in exp)
    for form in FORMS:
        check(eng, exp, docs, form, lean=len(docs), wide=len(docs))


# ---- 3. delete-set order under yjs 13.5 semantics: clients in first-seen order, by (update, position in its delete set)
def _ds_doc(k, at, seed):
    """k updates of clients A / B; the updates at the positions `at` carry delete sets.  Delete-set clients are first
    seen in ascending order of their ids (the sorted order is descending), two new ones per update, the second update
    on repeating the client seen two updates before (adjacent range: merged; its rank stays its first sighting's)."""
    g = Log([A, B], [5, 5], seed=seed)
    nxt, seen, n_ranges = 20, [], 0
    for j in range(k):
        c = (A, B)[j % 2]
        if j not in at:
            g.plain(c)
            continue
        n = at.index(j)
        ent = [(nxt, [(3 + n, 2)]), (nxt + 1, [(40, 1), (50 + n, 3)])]
        if len(seen) >= 2:
            ent.insert(1, (seen[-2], [(3 + n, 2)]))
        seen.append(nxt)
        nxt += 2
        n_ranges += sum(len(rs) for _, rs in ent)
        d = _ds(ent)
        if n % 3 == 2 or g.last is None:
            g.raw(b"\x00" + d)                                     # a deletion: no structs
        else:
            g.put(c, [item(4, text("q"), origin=g.last)], 1, ds=d)
    assert all(len(u) <= 32 for u in g.ups), max(len(u) for u in g.ups)
    assert 10 <= n_ranges <= 64, n_ranges
    return g.ups


def _ds_docs():
    docs = []
    for n, ln in enumerate((0, 1, 2, 14, 15, 16, 30, 47, 62)):
        b = 4 * ln + 3                                             # updates 4l+3 | 4l+4: the last of lane l, the first of lane l+1
        at = sorted({b - 1, b, b + 1, b + 2, 62, 63, 64, 65} | ({1, 2} if n % 2 else set()))
        docs.append(_ds_doc(min(255, 70 + 4 * ln + n), at, seed=n))
    # the delete sets on the far sides of the boundaries only, in reverse proximity: a rank by lane alone, or by slot
    # alone, orders these differently
    docs.append(_ds_doc(200, [3, 4, 63, 64, 67, 68, 128, 131, 132, 191, 192, 196], seed=50))
    docs.append(_ds_doc(133, [0, 7, 8, 60, 61, 66, 127, 128, 129, 130], seed=51))
    return docs


@pytest.mark.parametrize("form", FORMS)
def test_delete_set_first_seen_order_across_lane_boundaries(eng135, form):
    docs = _ds_docs()
    exp = expect("ds135", docs, compat135=True)
    assert all(st == 0 for st, _ in exp)
    # (the first-seen order of these documents is not the sorted one: the default semantics give other bytes)
    assert any(exp[d] != oracle.merge_updates(us) for d, us in enumerate(docs))
    check(eng135, exp, docs, form, lean=len(docs))


# ---- 4. store sequencing: a wave's documents of every kind follow each other in every order
N_SEQ = 8300     # the persistent grid holds 4 096 waves and 4 096 % 5 = 1: wave w's documents are of kinds w % 5, (w + 1) % 5, ...


def _seq_doc(d):
    kind = d % 5
    cl = 1 + d % 100
    if kind == 0:
        return fast_doc(3, [cl], seed=d)
    if kind == 1:
        return fast_doc(1, [cl], seed=d)
    if kind == 2:
        return []
    g = Log([cl], [d % 50], seed=d)
    g.plain(cl)
    g.plain(cl)
    if kind == 3:
        g.put(cl, [item(4, text("g"), origin=g.last)], 1, shift=1)     # a clock gap: deferred to the general kernels
    else:
        g.put(cl, [item(4, text("d"), origin=g.last)], 1, ds=_ds([(cl, [(g.clock[cl] - 2, 1)])]))
    return g.ups


def _seq_corpus():
    docs = MEMO.get("seq_docs", lambda: [_seq_doc(d) for d in range(N_SEQ)])
    return docs, expect("seq", docs)


@pytest.mark.parametrize("n", [N_SEQ, 1, 2, 4095, 4096, 4097])
def test_documents_of_every_kind_in_sequence(eng, n):
    docs, exp = _seq_corpus()
    docs, exp = docs[:n], exp[:n]
    n_lean = sum(1 for d in range(n) if d % 5 != 3)
    for form in FORMS:
        check(eng, exp, docs, form, lean=n_lean)

"""The narrow lean merge kernel's two placements: documents made only of single-character inserts and deletions, with
at most four clients, are placed in log order (a record's index and byte offset inside its client block come from
scans where the record is); every other document goes through the sorted domain.  The tests sit on the borders
between the two and on what the log-order placement has to prove by itself: client counts and orders, document
lengths at the lane and row edges, clock faults at every kind of position, first clocks of every varuint length,
slow rows and deletions among fast rows, the largest block byte totals, and batches that alternate the two
placements inside one persistent wave.  Every document is compared bit-exact with the CPU oracle in both input
forms, and the documents inside the envelope must be finished by the lean kernel."""
import pytest

import oracle
from devrun import Memo, engine_fixture, run_merge, same
from lean_docs import A, B, C, Log, _deletion_doc, _deletion_docs, _longest, fast_doc, item, text1
from v1util import vu

pytestmark = pytest.mark.gpu

FORMS = ["off", "lens"]
SMALL = [5, 9, 200, 70, 3, 127, 128, 90, 33]      # one- and two-byte client ids: 255 updates stay under the staged bytes
BIG = [3000000001, 77, 2 ** 31 + 5, 12345, 999, 4000000000, 2, 65536, 424242]
LN_IN, LN_OUT = 5120, 4096                       # the narrow kernel's staged input / output bytes


eng = engine_fixture()
eng135 = engine_fixture(compat135=True)
MEMO = Memo()
expect = MEMO.expect


def check(e, exp, docs, lean=None, wide=None):
    """Both input forms: exact against exp; `lean` documents finished by the lean kernels, `wide` of them by the wide one."""
    for form in FORMS:
        w0 = e.stats().docs_lean_wide
        res, took = run_merge(e, docs, form)
        bad = [d for d in range(len(docs)) if not same(exp[d], res[d])]
        assert not bad, (form, len(bad), bad[:5], [u.hex() for u in docs[bad[0]]][:8])
        if lean is not None:
            assert took == lean, (form, took, lean)
        if wide is not None:
            assert e.stats().docs_lean_wide - w0 == wide, (form, e.stats().docs_lean_wide - w0, wide)


def narrow(us):
    """The document is staged whole by the narrow kernel wherever the batch puts it."""
    return 2 <= len(us) <= 255 and all(len(u) <= 32 for u in us) and sum(len(u) for u in us) + 15 <= LN_IN


# ---- client count: 1 - 4 (log order; one byte scan up to two clients, two above), 5 and 8 (sorted domain), 9 (deferred)
@pytest.mark.parametrize("ids", [SMALL, BIG], ids=["small", "big"])
def test_client_counts(eng, ids):
    docs = [fast_doc(k, ids[:ncl], seed=10 * k + ncl) for ncl in (1, 2, 3, 4, 5, 8) for k in (ncl, 2 * ncl + 1, 61, 120) if k >= 2]
    assert all(narrow(us) for us in docs)
    exp = expect("ncl" + str(ids[0]), docs)
    assert all(st == 0 for st, _ in exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


def test_nine_clients_defer_and_are_exact(eng):
    docs = [fast_doc(k, ids[:9], seed=k) for ids in (SMALL, BIG) for k in (9, 40, 130)]
    exp = expect("ncl9", docs)
    assert all(st == 0 for st, _ in exp)
    check(eng, exp, docs, lean=0)


# ---- client order
def _order_docs():
    docs = []
    for ncl in (2, 3, 4):
        for ids in (SMALL[:ncl], BIG[:ncl], sorted(BIG[:ncl]), sorted(BIG[:ncl], reverse=True), [77, 3000000001, 12345, 2 ** 31 + 5][:ncl]):
            k = 97
            docs.append(fast_doc(k, ids, seed=ncl))                                          # strictly alternating
            docs.append(fast_doc(k, ids, seed=ncl + 1, order=lambda i: (i // 10) % ncl))         # runs of ten
            docs.append(fast_doc(k, ids, seed=ncl + 2, order=lambda i: (i // 4) % ncl))          # runs of one lane
            docs.append(fast_doc(k, ids, seed=ncl + 3, order=lambda i: (i // 3 + i // 7) % ncl))   # runs across lanes
            # a client whose only record is the last update (and one whose only record is the first)
            docs.append(fast_doc(k, ids, seed=ncl + 4, order=lambda i: ncl - 1 if i == k - 1 else i % (ncl - 1)))
            docs.append(fast_doc(k, ids, seed=ncl + 5, order=lambda i: 0 if i == 0 else 1 + i % (ncl - 1)))
    return docs


def test_client_orders(eng):
    docs = _order_docs()
    assert all(narrow(us) for us in docs)
    exp = expect("order", docs)
    assert all(st == 0 for st, _ in exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


# ---- k at the lane and row edges
EDGE_K = [2, 3, 4, 5, 8, 9, 63, 64, 65, 199, 200, 252, 253, 254, 255]


@pytest.mark.parametrize("ncl", [1, 2, 3, 4])
def test_document_lengths_at_the_edges(eng, ncl):
    docs = [fast_doc(k, SMALL[:ncl], seed=k + ncl) for k in EDGE_K]
    docs += [fast_doc(k, SMALL[:ncl], seed=k, order=lambda i: (i // 5) % ncl) for k in EDGE_K]
    assert all(narrow(us) for us in docs)
    exp = expect("edge%d" % ncl, docs)
    assert all(st == 0 for st, _ in exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


# ---- clock faults: a gap (+1), an overlap (-2: a clock two records back) and a repeated clock (-1) inside one client
FAULT_K = 130
FAULT_AT = [1, 2, 3, 4, 7, 64, 67, 124, 127, FAULT_K - 1]     # the first place a fault can be, updates 4l and 4l + 3, the last


def _fault_doc(ncl, at, shift, seed):
    """FAULT_K updates, round robin over ncl clients; update `at` has its client's clock shifted (the client's later
    updates follow on from the shifted clock: one fault)."""
    ids = SMALL[:ncl]
    g = Log(ids, [9] * ncl, seed)
    for j in range(FAULT_K):
        c = ids[j % ncl]
        if j == at:
            g.put(c, [item(4, text1("z"), origin=g.last)], 1, shift=shift)
        else:
            g.plain(c)
    return g.ups


@pytest.mark.parametrize("ncl", [1, 2, 3, 4])
def test_clock_faults_defer_and_are_exact(eng, ncl):
    docs, n_lean = [], 0
    for shift in (1, -2, -1):
        for at in FAULT_AT:
            if at < ncl:
                continue       # (a client's first record: below)
            docs.append(_fault_doc(ncl, at, shift, seed=at))
            docs.append(_fault_doc(ncl, None, 0, seed=at + 1))     # a clean neighbour: the next document of the batch
            n_lean += 1
    # a shifted first record of a client is contiguous with nothing: the block starts there, the document stays lean
    for at in range(ncl):
        docs.append(_fault_doc(ncl, at, 3, seed=50 + at))
        n_lean += 1
    assert all(narrow(us) for us in docs)
    check(eng, expect("fault%d" % ncl, docs), docs, lean=n_lean)


# ---- first clocks of every varuint length; the last record's clock at the largest one the kernel takes
def _first_clock_docs():
    docs = []
    top = 0xFFFFFFFE
    for ncl in (1, 2, 3, 4):
        k = 41
        per = [len(range(c, k, ncl)) for c in range(ncl)]          # records per client (round robin)
        for clocks in ([0] * ncl, [0, 120, 16380, 2 ** 21 - 5][:ncl], [2 ** 14, 2 ** 21, 2 ** 28, 2 ** 28 - 3][:ncl],
                       [2 ** 21 + 7] * ncl, [2 ** 28 + 1] * ncl, [2 ** 31] * ncl, [top - (n - 1) for n in per]):
            docs.append(fast_doc(k, SMALL[:ncl], clocks, seed=ncl))
            docs.append(fast_doc(k, [77, 12345, 999, 2][:ncl], clocks, seed=ncl + 7))
    return docs


def test_first_clocks(eng):
    docs = _first_clock_docs()
    assert all(narrow(us) for us in docs)
    exp = expect("fc", docs)
    assert all(st == 0 for st, _ in exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


def test_clock_past_the_largest_defers_and_is_exact(eng):
    # the last record's clock at 0xFFFFFFFF: clock + 1 is no uint32 -- the lean kernel does not take it
    docs = [fast_doc(9, SMALL[:ncl], [0xFFFFFFFF - (len(range(c, 9, ncl)) - 1) for c in range(ncl)], seed=ncl) for ncl in (1, 2, 3)]
    check(eng, expect("fcmax", docs), docs)


# ---- rows and lanes: one slow row among fast ones; deletions between inserts; lanes holding only deletions
def _slow_row_doc(ncl, at, shape, seed):
    ids = [A, B, C][:ncl]
    g = Log(ids, [5] * ncl, seed)
    for j in range(90):
        c = ids[j % ncl]
        o = g.last or (B, 1)
        if j != at:
            g.plain(c)
        elif shape == "str3":
            g.put(c, [item(4, b"\x03abc", origin=o)], 3)
        elif shape == "structs2":
            g.put(c, [item(4, text1("q"), origin=o), item(4, text1("r"), origin=(c, g.clock[c]))], 2)
        elif shape == "deleted":
            g.put(c, [item(1, vu(3), origin=o)], 3)
    return g.ups


@pytest.mark.parametrize("shape", ["str3", "structs2", "deleted"])
def test_one_slow_row_takes_the_sorted_domain(eng, shape):
    docs = []
    for ncl in (1, 2, 3):
        for at in (0, 1, 3, 4, 5, 6, 7, 63, 64, 88, 89):       # every slot of a lane, the row edge, the last update
            docs.append(_slow_row_doc(ncl, at, shape, seed=at))
            docs.append(fast_doc(30, [A, B, C][:ncl], seed=at))     # a log-order neighbour
    assert all(narrow(us) for us in docs)
    exp = expect("slow_" + shape, docs)
    assert all(st == 0 for st, _ in exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


def test_deletions_between_inserts(eng):
    docs = _deletion_docs()
    assert all(narrow(us) for us in docs)
    exp = expect("dels", docs)
    assert all(st == 0 for st, _ in exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


def test_deletions_first_seen_order_under_compat135(eng135):
    docs = _deletion_docs() + [fast_doc(50, BIG[:ncl], seed=ncl) for ncl in (1, 2, 3, 4, 5)]
    exp = expect("dels135", docs, compat135=True)
    assert all(st == 0 for st, _ in exp)
    # (first-seen order is not the sorted one in these documents: the default semantics give other bytes)
    assert any(exp[d] != oracle.merge_updates(us) for d, us in enumerate(docs[:8]))
    check(eng135, exp, docs, lean=len(docs), wide=0)


# ---- block byte totals: the longest fast shape (a 32-byte update: parent key, one character)
def _longest_doc(per_client, ncl):
    return [_longest([A, B][j % ncl], 3 + j // ncl) for j in range(per_client * ncl)]


def test_block_byte_totals(eng):
    # 255 records of the longest shape per client: the 16-bit byte fields' largest values.  (Such a document is past the
    # kernels' staged bytes, or past their 255 updates with two clients: deferred before any placement.)
    big = [_longest_doc(255, 1), _longest_doc(255, 2)]
    check(eng, expect("bytes_big", big), big, lean=0)
    # the largest documents the narrow kernel stages: their output is past LN_OUT, which the size test has to see
    # with the whole byte total (the wide kernel, with more output bytes, finishes them) ...
    over = [_longest_doc(159, 1), _longest_doc(79, 2), [_longest(A, 3 + j) for j in range(100)] + [_longest(B, 3 + j) for j in range(59)]]
    assert all(sum(len(u) for u in us) + 15 <= LN_IN for us in over)
    exp = expect("bytes_over", over)
    assert all(st == 0 and len(b) > LN_OUT for st, b in exp)
    check(eng, exp, over, lean=len(over), wide=len(over))
    # ... and the largest ones whose output fits: finished by the narrow kernel
    fit = [_longest_doc(150, 1), _longest_doc(75, 2), [_longest(A, 3 + j) for j in range(148)] + [_longest(B, 3), _longest(B, 4)]]
    exp = expect("bytes_fit", fit)
    assert all(st == 0 and LN_OUT - 80 < len(b) <= LN_OUT for st, b in exp), [len(b) for _, b in exp]
    check(eng, exp, fit, lean=len(fit), wide=0)


# ---- batches alternating the two placements inside a persistent wave
N_MIX = 8200     # the grid holds 4 096 waves and 4 096 % 7 = 1: wave w's documents are of kinds w % 7, (w + 1) % 7, ...


def _mix_doc(d):
    kind = d % 7
    k = 2 + d % 11
    if kind == 0:
        return fast_doc(k, [1 + d % 100], seed=d)                                   # log order, one byte scan
    if kind == 1:
        return fast_doc(k + 3, SMALL[:5 + d % 4], seed=d)                           # sorted domain: 5 - 8 clients
    if kind == 2:
        return fast_doc(k + 2, BIG[d % 3:d % 3 + 3 + d % 2], seed=d)                # log order, two byte scans
    if kind == 3:
        return _slow_row_doc(1 + d % 3, d % 5, ("str3", "structs2", "deleted")[d % 3], seed=d)[:6 + d % 9]   # sorted domain: a slow row
    if kind == 4:
        return _deletion_doc(1 + d % 4, k + 2, {1, k}, d % 2 == 0, seed=d)           # log order with deletions
    if kind == 5:
        g = Log([A, B], [d % 50, 3], seed=d)                                        # log order, a clock gap: deferred
        for j in range(k + 2):
            if j == k:
                g.put(A, [item(4, text1("g"), origin=g.last)], 1, shift=1)
            else:
                g.plain((A, B)[j % 2] if j < k else A)
        return g.ups
    return fast_doc(k, SMALL[1:3], [d, 2 * d], seed=d)                              # log order, two clients


def _mix_corpus():
    docs = MEMO.get("mix_docs", lambda: [_mix_doc(d) for d in range(N_MIX)])
    return docs, expect("mix", docs)


@pytest.mark.parametrize("n", [N_MIX, 1, 2, 4095, 4096, 4097])
def test_batches_mixing_both_placements(eng, n):
    docs, exp = _mix_corpus()
    docs, exp = docs[:n], exp[:n]
    n_lean = sum(1 for d in range(n) if d % 7 != 5)
    check(eng, exp, docs, lean=n_lean, wide=0)

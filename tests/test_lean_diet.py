"""The narrow lean merge kernel where its vote and its fast parse were put on a diet: clients of an all-single-Item
document are found in the order their first records appear in the log and ranked afterwards (a fifth client sends
the document to the descending vote), the parent-key shape is looked at only in a row that holds an insert without
origins, and the shape of an update is decided from where its varuints end.  The tests sit on those borders: every
order of first sight, client ids of every varuint length, a block's first record at every kind of position, no-origin
inserts in every slot, malformed and near-miss updates of each shape, and batches in which one persistent wave takes
the three kinds of document one after another.  Every document is compared bit-exact with the CPU oracle in both
input forms; where stated, with the count of documents the narrow kernel finished.  They describe behaviour, not
the kernel.  (Documents have 2 to 40 updates, except those that need a record in lane 49: 200.)"""
import itertools

import pytest

import oracle
from devrun import Memo, engine_fixture, run_merge, same
from lean_docs import Log, _deletion_docs, _ds, _longest, fast_doc, item, overlong, upd
from v1util import vu

pytestmark = pytest.mark.gpu

FORMS = ["off", "lens"]
SMALL = [5, 9, 70, 200]
BIG = [3000000001, 77, 2 ** 31 + 5, 12345]


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


def all_ok(exp):
    return all(st == 0 for st, _ in exp)


# ======================================================================= the vote by first sight
def _order_docs():
    """Every order of first sight of 2, 3 and 4 clients: the clients list is the order (update i: client i mod n),
    then the same orders with runs of one lane and a half."""
    docs = []
    for ids in (SMALL, BIG):
        for ncl in (2, 3, 4):
            for perm in itertools.permutations(ids[:ncl]):
                docs.append(fast_doc(2 * ncl + 3, list(perm), seed=ncl))
                docs.append(fast_doc(40, list(perm), seed=ncl + 1, order=lambda i: (i // 6) % ncl))
    return docs


def test_every_order_of_first_sight(eng):
    docs = _order_docs()
    assert len(docs) == 2 * 2 * (2 + 6 + 24)
    exp = expect("order", docs)
    assert all_ok(exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


VU_IDS = [1, 127, 128, 2 ** 14 - 1, 2 ** 14, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 0xFFFFFFFF]
TOP_BYTE = [0x00ABCDEF, 0x10ABCDEF, 0x20ABCDEF, 0xF0ABCDEF]       # ids that differ only in the top byte


def _id_docs(with_zero):
    docs = []
    pool = ([0] if with_zero else []) + VU_IDS
    for j in range(len(pool)):
        ids = [pool[(j + 3 * t) % len(pool)] for t in range(4)]
        if with_zero and 0 not in ids:
            continue
        for ncl in (1, 2, 3, 4):
            docs.append(fast_doc(3 * ncl + 2, ids[:ncl], seed=j))
    if not with_zero:
        for perm in itertools.permutations(TOP_BYTE):
            docs.append(fast_doc(14, list(perm), seed=1))
    return docs


def test_client_ids_of_every_varuint_length(eng):
    docs = _id_docs(False)
    exp = expect("ids", docs)
    assert all_ok(exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


def test_client_id_zero_is_exact(eng):
    # (an origin of client 0 is a zero byte right after the info byte, which the lean kernel leaves to the general ones)
    docs = _id_docs(True)
    # client 0 seen last and only at the last update: no origin names it, and it ranks last among 2, 3 and 4 clients
    docs += [fast_doc(k, ids + [0], seed=k, order=lambda i: len(ids) if i == k - 1 else i % len(ids))
             for ids in ([7], [7, 9], [200, 9, 7]) for k in (len(ids) + 1, 23)]
    check(eng, expect("ids0", docs), docs)


def _seq_doc(seq, ids=SMALL, clocks=None, seed=0):
    """seq: per update a client index, 'x' (a deletion with one range) or 'e' (a deletion with an empty delete set)."""
    g = Log(ids, clocks or [3] * len(ids), seed)
    n = 0
    for s in seq:
        if s == "x":
            g.raw(b"\x00" + _ds([(ids[n % 2], [(40 + 2 * n, 1)])]))
            n += 1
        elif s == "e":
            g.raw(b"\x00\x00")
        else:
            g.plain(ids[s])
    return g.ups


def _position_docs():
    docs = []
    # the second (third, fourth) block's first record in slot 3 of lane 0, of lane 1, of lane 9 ...
    for at in (3, 7, 39):
        docs.append(_seq_doc([0] * at + [1] + [0, 1] * ((39 - at) // 2)))
        docs.append(_seq_doc([0] * at + [3] + [0, 3, 1] * ((39 - at) // 3), seed=1))
    # ... and in every slot of lane 49 (200 updates), the block ranking first (3), in the middle (1), last
    for at in (196, 197, 198, 199):
        docs.append(_seq_doc([0, 2] * (at // 2) + [0] * (at % 2) + [3] + [0] * (199 - at), seed=at))
        docs.append(_seq_doc([1, 2] * (at // 2) + [1] * (at % 2) + [0] + [1] * (199 - at), seed=at + 1))
        docs.append(_seq_doc([3] * at + [1] + [3] * (199 - at), seed=at + 2))
    # lanes that hold only deletions before a block's first record: before the second block, before every block
    docs.append(_seq_doc([0, 0, 0, 0] + ["x"] * 8 + [1, 0, 1, 2] + ["e"] * 5 + [3, 0]))
    docs.append(_seq_doc(["x"] * 8 + [2] + ["e"] * 7 + [3, 2, 0, 1], seed=2))
    docs.append(_seq_doc(["e"] * 4 + ["x"] * 3 + [1, 0] + ["x"] * 11 + [1, 0, 3], seed=3))
    docs.append(_seq_doc(["x"] * 39 + [2], seed=4))
    # a client seen at update 0 and next at the last update
    for ncl in (2, 3, 4):
        for k in (ncl + 1, 17, 40):
            docs.append(fast_doc(k, SMALL[:ncl], seed=k, order=lambda i: 0 if i in (0, k - 1) else 1 + i % (ncl - 1)))
            docs.append(fast_doc(k, BIG[:ncl], seed=k, order=lambda i: 0 if i in (0, k - 1) else 1 + i % (ncl - 1)))
    return docs


def test_first_records_at_every_kind_of_position(eng):
    docs = _position_docs()
    exp = expect("pos", docs)
    assert all_ok(exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


FIVE = [5, 9, 70, 200, 33]
NINE = [5, 9, 70, 200, 33, 3, 127, 128, 90]


def test_five_clients_take_the_descending_vote_and_stay_narrow(eng):
    docs = [fast_doc(k, list(perm) + [FIVE[4]], seed=k) for k in (5, 6, 23, 40) for perm in itertools.permutations(FIVE[:4])][::3]
    docs += [fast_doc(k, ids[:5], seed=k) for k in (5, 40) for ids in (BIG + [999], sorted(FIVE), sorted(FIVE, reverse=True))]
    exp = expect("five", docs)
    assert all_ok(exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


def test_nine_clients_defer_and_are_exact(eng):
    docs = [fast_doc(k, NINE, seed=k) for k in (9, 10, 40)]
    exp = expect("nine", docs)
    assert all_ok(exp)
    check(eng, exp, docs, lean=0)


def _fault_doc(ids, shift, at, k=24, seed=0):
    """Round robin over ids; update `at` has its client's clock shifted (later ones follow on: one fault)."""
    g = Log(ids, [9] * len(ids), seed)
    for j in range(k):
        c = ids[j % len(ids)]
        if j == at:
            g.put(c, [item(4, b"\x01z", origin=g.last)], 1, shift=shift)
        else:
            g.plain(c)
    return g.ups


def test_clock_faults_in_the_block_seen_second_that_ranks_first(eng):
    docs, n_lean = [], 0
    for ids in ([5, 200], [5, 200, 9], [77, 3000000001, 12345, 999]):     # ids[1] is seen second and is the largest
        n = len(ids)
        for shift in (1, -1):                                              # a gap, an overlap
            for at in (1 + n, 1 + 2 * n, 1 + n * ((24 - 2) // n)):         # its second record, its third, its last
                docs.append(_fault_doc(ids, shift, at, seed=at))
                docs.append(_fault_doc(ids, 0, None, seed=at + 1))         # a clean neighbour
                n_lean += 1
    check(eng, expect("fault", docs), docs, lean=n_lean)


def test_deletions_first_seen_order_under_compat135(eng135):
    docs = _deletion_docs() + [_seq_doc(["x"] * 5 + [1, 0, 3] + ["x"] * 4 + [2], seed=9)]
    exp = expect("dels135", docs, compat135=True)
    assert all_ok(exp)
    assert any(exp[d] != oracle.merge_updates(us) for d, us in enumerate(docs[:8]))
    check(eng135, exp, docs, lean=len(docs), wide=0)


# ======================================================================= the parent-key shape, row by row
A, B = 5, 9


def _keyed(at, k=40, key=None, seed=0):
    """k updates of A / B; the ones at the positions `at` (and update 0) are inserts under a parent key with no origin."""
    g = Log([A, B], [5, 5], seed)
    for j in range(k):
        c = (A, B)[j % 2]
        if j in at:
            kb = b"t" if key is None else key
            g.put(c, [item(4, b"\x01q", parent=b"\x01" + vu(len(kb)) + kb)], 1)
        else:
            g.plain(c)
    return g.ups


def test_no_origin_inserts_in_every_slot(eng):
    docs = [_keyed({at}, seed=at) for at in (0, 1, 2, 3, 20, 21, 22, 23)]       # lane 0 and lane 5, one document each
    docs += [_keyed({1, 22}), _keyed({2, 7, 39}), _keyed({1, 2, 3, 21, 23}), _keyed(set(range(40)))]   # two rows and more at once
    # rows whose only lane without origins is past the document's end (the kernel parks those lanes on update 0)
    docs += [_keyed(set(), k=k, seed=k) for k in (2, 3, 5, 6, 7, 38)]
    exp = expect("slots", docs)
    assert all_ok(exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


def test_parent_keys_of_every_length(eng):
    docs = []
    for at in (0, 2, 21):
        docs += [_keyed({at}, key=b""), _keyed({at}, key=b"k"), _keyed({at}, key=b"key-of-16-bytes!")]
    docs.append([_longest(A, 3 + j) for j in range(9)])                          # 32 bytes: the longest that fits
    docs.append(_keyed({0}, k=6)[:1] + [_longest(70, 3), _longest(70, 4)] + _keyed({0}, k=6)[1:])
    exp = expect("keys", docs)
    assert all_ok(exp)
    check(eng, exp, docs, lean=len(docs), wide=0)


def test_parent_keys_the_fast_parse_refuses_are_exact(eng):
    docs = []
    for at in (0, 3, 22):
        docs.append(_keyed({at}, key="é".encode()))          # a key byte of 0x80 or above
        docs.append(_keyed({at}, key=b"k" * 0x80))           # a key length of 0x80 or above
        docs.append(_keyed({at}, key=b"k" * 0x91))
    exp = expect("keys_refused", docs)
    assert all_ok(exp)
    check(eng, exp, docs)


# ======================================================================= the shape of an update
SHAPES = ["origin", "right", "both", "key"]
INFO = {"origin": 0x84, "right": 0x44, "both": 0xC4, "key": 0x04}
C5 = 0xFFFFFF01                      # a five-byte client id


def fields(shape, c, ck, o=(B, 2), r=(B, 1), key=b"t", s=b"\x01q", ds=b"\x00"):
    """The update as a list of fields, and the indexes of its varuint fields after the struct count."""
    f = [b"\x01", b"\x01", vu(c), vu(ck), bytes([INFO[shape]])]
    vus = [2, 3]
    if shape in ("origin", "both"):
        vus += [len(f), len(f) + 1]
        f += [vu(o[0]), vu(o[1])]
    if shape in ("right", "both"):
        vus += [len(f), len(f) + 1]
        f += [vu(r[0]), vu(r[1])]
    if shape == "key":
        vus += [len(f) + 1]
        f += [b"\x01", vu(len(key)), key]
    vus += [len(f), len(f) + 2]
    f += [s[:1], s[1:], ds]
    return f, vus


def wrap(c, ck, u, clen=1):
    """A document around the update u (client c, clock ck + 1): a first insert before it, two plain ones after."""
    first = upd(c, ck, [item(4, b"\x01a")])
    after = [upd(c, ck + 1 + clen + j, [item(4, b"\x01b", origin=(c, ck + clen + j))]) for j in range(2)]
    return [first, u] + after


def _sized(shape, n):
    """The shape at exactly n bytes: varuints of up to five bytes where the shape has room for it, else id varuints of
    seven to nine bytes (which no kernel's fast path takes)."""
    ck = 2 ** 28 + 7                                       # five clock bytes
    if shape == "key":
        f, _ = fields(shape, C5, ck + 1, key=b"k" * (n - 18))
    elif shape == "both":
        ock, rck = {31: (2 ** 7, 2 ** 14 + 1), 32: (2 ** 14, 2 ** 14 + 1), 33: (2 ** 14, 2 ** 21 + 1)}[n]
        f, _ = fields(shape, C5, ck + 1, o=(2 ** 32 - 3, ock), r=(2 ** 32 - 2, rck))
    else:
        f, v = fields(shape, C5, ck + 1)
        f[v[2]] = vu(2 ** 49 + 5)                          # eight bytes
        f[v[3]] = vu(2 ** (7 * (n - 25)) + 3)              # seven, eight, nine bytes
    u = b"".join(f)
    assert len(u) == n, (shape, n, len(u))
    return wrap(C5, ck, u)


def _variants(shape):
    c, ck = A, 11
    docs = [_sized(shape, n) for n in (31, 32, 33)]

    def doc(f, clen=1):
        return wrap(c, ck, b"".join(f), clen)
    f, v = fields(shape, c, ck + 1)
    docs.append(doc(f))                                                        # the shape itself
    docs.append(doc(f[:5] + [b"\x07"] + f[5:]))                                # an extra varuint after the info byte
    docs.append(doc(f[:-3] + [b"\x07"] + f[-3:]))                              # ... before the string length
    docs.append(doc(f[:v[-3]] + f[v[-3] + 1:]))                                # the last id varuint (the key length) missing
    for big in (2 ** 35 + 1, 2 ** 49 + 1):                                     # a varuint of 6 and of 8 bytes
        for i in (v[2:-2] if shape != "key" else v[:1]):
            g = list(f)
            g[i] = vu(big)
            docs.append(doc(g))
    for i in v:                                                                # the overlong pair at each varuint in turn
        g = list(f)
        g[i] = overlong(g[i])
        docs.append(doc(g))
    docs.append(doc(fields(shape, c, ck + 1, s=b"\x02qr")[0], clen=2))         # string length 2
    docs.append(doc(fields(shape, c, ck + 1, s=b"\x02" + "é".encode())[0]))    # a character of 0x80 or above
    docs.append(doc(fields(shape, c, ck + 1, ds=b"\x01" + vu(c) + b"\x01" + vu(2) + vu(1))[0]))   # a delete set
    # as many terminators before byte n - 4 as the shape has, but byte n - 4 is a continuation byte
    g = list(f)
    g[v[-3]] = b"\x05" + bytes([g[v[-3]][-1] | 0x80]) if shape != "key" else bytes([g[v[-3]][-1] | 0x80])
    docs.append(doc(g))
    g = list(f)
    g[v[-3] - (0 if shape == "key" else 1)] = b"\x85"
    docs.append(doc(g))
    return docs


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_and_their_near_misses(eng, shape):
    docs = _variants(shape)
    exp = expect("shape_" + shape, docs)
    assert exp[3][0] == 0 and (shape not in ("both", "key") or all_ok(exp[:2]))
    check(eng, exp, docs)
    # the shape itself, and its 31- and 32-byte forms where plain varuints reach them, are the narrow kernel's
    mine = [docs[3]] + (docs[:2] if shape in ("both", "key") else [])
    check(eng, [exp[3]] + (exp[:2] if shape in ("both", "key") else []), mine, lean=len(mine), wide=0)


# ======================================================================= one wave, every kind after every other
GRID = 4096                      # the narrow kernel's waves: wave w takes documents w, w + GRID, ...
POOL = 24


def _kind_doc(kind, j):
    k = 2 + j % 7
    if kind == 0:
        return fast_doc(k + 2, [SMALL, BIG][j % 2][:1 + j % 4], seed=j)          # voted by first sight
    if kind == 1:
        return fast_doc(k + 5, FIVE, seed=j)                                      # five clients: the descending vote
    return _fault_doc([5, 200], 1, 3 + j % 4, k=8 + j % 5, seed=j)                # a clock gap: deferred


def _loop_corpus(n):
    """Document d of wave w = d % GRID, round r = d // GRID is of kind (w + (0, 1, 0)[r]) % 3: over three rounds every wave
    steps one kind up and one kind down, and the waves between them start at every kind."""
    pool = MEMO.get("pool", lambda: [[_kind_doc(kind, j) for j in range(POOL)] for kind in range(3)])
    pool_exp = MEMO.get("pool_exp", lambda: [[oracle.merge_updates(us) for us in row] for row in pool])
    docs, exp, lean = [], [], 0
    for d in range(n):
        kind = (d % GRID + (0, 1, 0)[(d // GRID) % 3]) % 3
        docs.append(pool[kind][d % POOL])
        exp.append(pool_exp[kind][d % POOL])
        lean += kind != 2
    return docs, exp, lean


@pytest.mark.parametrize("n", [1, 2, GRID + 1, 3 * GRID])
def test_batches_alternating_the_three_kinds(eng, n):
    docs, exp, lean = _loop_corpus(n)
    assert all(st == 0 for st, _ in exp)
    check(eng, exp, docs, lean=lean, wide=0)

"""The corpora of test_lean_slowclass.py: the narrow lean merge kernel where its arithmetic runs in the VALU's fast
instruction class -- the value of a varuint (client, clock, delete-set fields) from dot products of its bytes, the byte
masks of the struct copies from shifts and a clamp, the guards of a fifth varuint byte without selects.  What can go
wrong there is a value built from the wrong bytes, a byte of a neighbouring struct overwritten or dropped, and a
document taken or deferred that was not before -- so the corpora are

  varuints   client and clock of every length at the values on both sides of each length, client 0, a fifth byte with
             a bit of 0x70, the byte after a varuint being 0x7F / 0x80 / 0xFF, and the same values as origin ids, in a
             multi-character insert (the generic parse) and as delete-set client, clock and length (one range: the
             fast path; more: the cursor walk);
  copies     structs of every length the narrow kernel takes (4 to 27 bytes) at every offset of an output dword and of a
             source dword, documents on both sides of the copy widths 20 | 21 and 24 | 25, short structs packed between
             long ones, append-shaped and mid-text inserts mixed;
  vote       1 to 5 clients in every order of first sight, ids that differ only in the top bit or only in the fifth
             byte, a client that only a delete set names, a block of 255 records, and a clock gap and an overlap in the
             block of every rank.

A document marked "lean" is never deferred, one marked "bad" is never taken.  (Documents have 2 to 40 updates, except
the block of 255 records.)  tests/test_lean_docs.py checks the corpora against the oracle on the CPU."""
import itertools
import random

from lean_docs import Log, _ds, fast_doc, item, text, upd
from v1util import vu


class Corpus:
    """Documents in arena order (packed back to back from arena byte 0); kind 'lean' (finished by a lean kernel),
    'bad' (never taken by one) or 'any' (exact, whoever finishes it: no corpus with such a document asserts the count)."""

    def __init__(self):
        self.docs, self.kind, self.b0, self.at = [], [], [], 0

    def add(self, us, kind="lean"):
        assert kind in ("lean", "bad", "any")
        self.docs.append(us)
        self.kind.append(kind)
        self.b0.append(self.at)
        self.at += sum(map(len, us))
        return len(self.docs) - 1

    def lean(self):
        return None if "any" in self.kind else sum(k == "lean" for k in self.kind)


# ======================================================================= varuints
# both sides of every varuint length, and the largest uint32
VALS = [127, 128, 2 ** 14 - 1, 2 ** 14, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 32 - 1]
A, B = 5, 200                     # a one- and a two-byte client id


def origin_doc(k, clients, clocks, order):
    """k updates of one character each: the first under the parent key, every later one with an origin alone (two
    five-byte varuints of the document and two of the origin fit the 32 bytes; a right origin beside them does not)."""
    g = Log(clients, clocks)
    for i in range(k):
        cl = clients[order(i)]
        g.put(cl, [item(4, text("abcdefgh"[i % 8]), origin=g.last)], 1)
    return g.ups


def _client_clock_corpus():
    """Client c and first clock k - 2 for every pair of VALS: six updates of c (and two of a small client between them)
    whose clocks run k - 2 .. k + 3, across the length's edge.  A clock of 2^32 - 1 and beyond is no lean document."""
    c = Corpus()
    turn = lambda i: 0 if i % 4 else 1
    for cl in VALS:
        for k in VALS:
            if k == 2 ** 32 - 1:
                c.add(origin_doc(8, [cl, A], [k - 7, 3], turn))           # clocks 2^32 - 8 .. 2^32 - 3
                c.add(origin_doc(8, [cl, A], [k - 3, 3], turn), "any")    # .. 2^32 + 2
            else:
                c.add(origin_doc(8, [cl, A], [k - 2, 3], turn))
    return c


def _next_byte_corpus():
    """The byte after the client varuint is the clock's first: 0x7F, 0x80 (128), 0xFF (255), and 0xFE / 0x00 beside
    them; the byte after the clock is the info byte: 0x84, 0x44, 0xC4 (Log.plain takes them in turn).  Every client
    length, the client's bytes all ones and all zeros below the top."""
    c = Corpus()
    for cl in (1, 127, 128, 2 ** 14 - 1, 2 ** 14, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 32 - 1):
        for k0 in (125, 253, 2 ** 14 - 3, 2 ** 21 - 3):
            c.add(fast_doc(9, [cl], [k0], seed=k0 & 0xFF))
    return c


def _fifth(b, bits):
    """The five-byte varuint b with `bits` (of 0x70) set in its fifth byte."""
    assert len(b) == 5
    return b[:4] + bytes([b[4] | bits])


def _fifth_byte_corpus():
    """A fifth byte with a bit of 0x70 (a value of 2^32 and more) in the client, in the clock, in a delete set's client:
    never a lean document.  Each beside its twin without the bit."""
    c = Corpus()
    big = vu(2 ** 32 - 1)
    for bits in (0x10, 0x20, 0x40, 0x70):
        for at in (0, 1, 4):
            g = Log([A], [9], seed=bits + at)
            for j in range(6):
                if j == at:
                    g.raw(upd(_fifth(big, bits), 7, [item(4, text("q"), origin=(A, 9))]))
                else:
                    g.plain(A)
            c.add(g.ups, "bad")
            g = Log([A], [9], seed=bits + at)
            for j in range(6):
                if j == at:
                    g.raw(upd(_fifth(big, bits), _fifth(vu(2 ** 28 + 1), 0), [item(4, text("q"), origin=(A, 9))]))
                else:
                    g.plain(A)
            c.add(g.ups, "bad")
        # the clock's fifth byte
        g = Log([A, B], [9, 2 ** 28 + 5], seed=bits)
        g.plain(A)
        g.plain(B)
        g.put(B, [item(4, text("q"), origin=g.last)], 1, clock_bytes=_fifth(vu(g.clock[B]), bits))
        g.plain(A)
        c.add(g.ups, "bad")
        c.add(fast_doc(4, [A, B], [9, 2 ** 28 + 5], seed=bits))
        # a delete set's client: one range (the fast path), two ranges (the cursor walk)
        for rs in ([(3, 1)], [(3, 1), (9, 2)]):
            g = Log([A], [9], seed=bits)
            g.plain(A)
            g.raw(b"\x00\x01" + _fifth(big, bits) + vu(len(rs)) + b"".join(vu(k) + vu(n) for k, n in rs))
            g.plain(A)
            c.add(g.ups, "bad")
            g = Log([A], [9], seed=bits)
            g.plain(A)
            g.raw(b"\x00" + _ds([(2 ** 32 - 1, rs)]))
            g.plain(A)
            c.add(g.ups)
    return c


def _client_zero_corpus():
    """Client 0 (an origin of client 0 is a zero byte right after the info byte: left to the general kernels)."""
    c = Corpus()
    for ids in ([0], [0, A], [A, 0], [2 ** 32 - 1, 0, 128]):
        c.add(fast_doc(3 * len(ids) + 2, ids, seed=len(ids)), "any")
    # client 0 seen last, at the last update only: no origin names it
    for ids in ([7], [7, 9], [200, 9, 7]):
        k = 11
        c.add(fast_doc(k, ids + [0], seed=k, order=lambda i: len(ids) if i == k - 1 else i % len(ids)), "any")
    return c


def _origin_corpus():
    """The values as origin and right-origin ids (copied byte for byte), and as the client and clock of a
    multi-character insert, which the generic parse reads."""
    c = Corpus()
    for i, v in enumerate(VALS):
        w = VALS[(i + 4) % len(VALS)]
        g = Log([A], [9], seed=i)
        g.plain(A)
        g.put(A, [item(4, text("q"), origin=(v, w), right=(w, v))], 1)
        g.put(A, [item(4, text("r"), origin=(v, v))], 1)
        g.put(A, [item(4, text("s"), right=(w, w))], 1)
        g.plain(A)
        c.add(g.ups)
    for cl in VALS:
        for k in VALS[:-1]:
            g = Log([cl, A], [k - 2, 3], seed=k & 0xFF)
            g.plain(A)
            g.put(cl, [item(4, text("abc"), origin=g.last)], 3)          # clocks k - 2 .. k
            g.put(cl, [item(4, text("de"), origin=g.last)], 2)           # k + 1, k + 2
            g.plain(A)
            g.put(cl, [item(1, vu(3), origin=g.last)], 3)                # a ContentDeleted of three
            c.add(g.ups)
    return c


DS_VALS = [127, 128, 2 ** 14 - 1, 2 ** 14, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1]     # clocks and lengths a lean delete set holds


def _ds_corpus():
    """Delete-set client (VALS), clock and length (DS_VALS; 2^28 and more: never lean): one client with one range (the
    fast path), with two ranges, and two clients (the cursor walk).  The byte after a clock is the length's first:
    0x7F, 0x80, 0xFF among them."""
    c = Corpus()
    for i, cl in enumerate(VALS):
        for j, k in enumerate(DS_VALS):
            n = DS_VALS[(i + j) % len(DS_VALS)]
            g = Log([A], [9], seed=i + j)
            g.plain(A)
            g.raw(b"\x00" + _ds([(cl, [(k, n)])]))
            g.plain(A)
            if j % 2:
                g.raw(b"\x00" + _ds([(cl, [(3, 255), (2 ** 21 + k, n)])]))
            else:
                g.raw(b"\x00" + _ds([(A, [(k, 127)]), (cl, [(n, k)])]))
            g.plain(A)
            c.add(g.ups)
    for big in (2 ** 28, 2 ** 32 - 1):
        for rs in ([(big, 1)], [(7, big)], [(3, 1), (big, 2)]):
            g = Log([A], [9], seed=1)
            g.plain(A)
            g.raw(b"\x00" + _ds([(B, rs)]))
            g.plain(A)
            c.add(g.ups, "bad")
    # an insert that carries a delete set of its own
    for cl in VALS:
        g = Log([A], [9], seed=2)
        g.plain(A)
        g.put(A, [item(4, text("q"), origin=g.last)], 1, ds=_ds([(cl, [(2 ** 14, 2 ** 21 - 1)])]))
        g.plain(A)
        c.add(g.ups)
    return c


# ======================================================================= copies
SB_MIN, SB_MAX = 4, 27            # struct bytes of one update the narrow kernel takes (a 32-byte update, one-byte ids)


def _wid(n):
    """A varuint value of n bytes."""
    return 3 if n == 1 else 2 ** (7 * (n - 1)) + 3


def sized_struct(sb, ch="q"):
    """One struct of exactly sb bytes (content length 1): a ContentDeleted with an origin (4), one character with an
    origin (5 .. 13), with both origins (14 .. 23), under a parent key (24 .. 27)."""
    if sb == 4:
        s = item(1, vu(1), origin=(3, 3))
    elif sb <= 13:
        oc = min(5, sb - 4)
        s = item(4, text(ch), origin=(_wid(oc), _wid(sb - 3 - oc)))
    elif sb <= 23:
        w = [1, 1, 1, 1]
        for _ in range(sb - 3 - 4):
            i = max(range(4), key=lambda j: 5 - w[j])
            w[i] += 1
        s = item(4, text(ch), origin=(_wid(w[0]), _wid(w[1])), right=(_wid(w[2]), _wid(w[3])))
    else:
        s = item(4, text(ch), parent=b"\x01" + vu(sb - 5) + b"k" * (sb - 5))
    assert len(s) == sb, (sb, len(s))
    return s


def struct_doc(seq, c=A, ck0=3):
    """One client's log: seq holds struct lengths, 'e' (a deletion with an empty delete set: two bytes) and 'x' (a
    deletion of one range of a two-byte client: seven bytes).  Returns the updates."""
    ups, ck = [], ck0
    for s in seq:
        if s == "e":
            ups.append(b"\x00\x00")
        elif s == "x":
            ups.append(b"\x00" + _ds([(B, [(len(ups), 1)])]))
        else:
            ups.append(upd(c, ck, [sized_struct(s, "abcdefgh"[len(ups) % 8])]))
            ck += 1
    return ups


def _ip(u):
    """Offset of the info byte of an update's first struct: after the two counts, the client and the clock."""
    p = 2
    for _ in range(2):
        while u[p] & 0x80:
            p += 1
        p += 1
    return p


def placements(us, b0):
    """(struct bytes, offset in its output dword, offset in its source dword) of every struct of a one-client document
    whose first byte lies at arena offset b0: the merged block is the header and the structs back to back; the kernel
    stages the document from its 16-byte granule."""
    recs, pos = [], b0 % 16
    for u in us:
        if u[0]:
            recs.append((len(u) - 1 - _ip(u), pos + _ip(u)))
        pos += len(u)
    first = next(u for u in us if u[0])
    # the document's block count, the block's struct count, its client and first clock (the first update's)
    out, t = [], 1 + len(vu(len(recs))) + _ip(first) - 2
    for sb, src in recs:
        out.append((sb, t & 3, src & 3))
        t += sb
    return out


def _every_length_corpus():
    """Per struct length documents of that length mixed with five-byte structs and deletions (which move the source
    by two and by seven bytes and the output not at all), seeds taken until the length has been at every pair of
    output and source offsets."""
    c, cover = Corpus(), {}
    for sb in range(SB_MIN, SB_MAX + 1):
        seen, seed = set(), 0
        while len(seen) < 16:
            rng = random.Random(sb * 100 + seed)
            seq = []
            while sum(1 for s in seq) < 36:
                r = rng.random()
                seq.append(sb if r < 0.6 else 5 if r < 0.75 else "e" if r < 0.9 else "x")
            us = struct_doc(seq)
            d = c.add(us)
            seen |= {(h, s) for n, h, s in placements(us, c.b0[d]) if n == sb}
            seed += 1
            assert seed < 12, (sb, sorted(seen))
        cover[sb] = seen
    return c, cover


def _width_corpus():
    """Documents whose widest run (offset in the output dword plus struct bytes) is 20, 21, 24 and 25 -- each side of
    the widths at which the copy takes another number of dwords -- with and without a five-byte struct among them (a
    least run of at most 8, or the widest struct's own)."""
    c, widest = Corpus(), set()
    for sb in range(14, 24):
        for short in (False, True):
            for k, ck0 in ((9, 3), (12, 300)):     # (a first clock of two bytes: the block's header is one byte longer)
                seq = [sb] * k
                if short:
                    seq[2:2] = [5]
                    seq[7:7] = [5, "e"]
                us = struct_doc(seq, ck0=ck0)
                d = c.add(us)
                pl = placements(us, c.b0[d])
                widest.add((max(h + n for n, h, _ in pl), min(h + n for n, h, _ in pl) <= 8))
    return c, widest


def _packed_corpus():
    """A short struct (4, 5, 6 bytes) between two long ones (17, 20, 23, 27 bytes), the short one at every offset of an
    output dword: a wrong tail mask of the long struct before it or a wrong head mask of the one after it lands in it."""
    c, heads = Corpus(), set()
    for long_ in (17, 20, 23, 27):
        for short in (4, 5, 6):
            for lead in ([], [5], [6], [7]):
                seq = lead + [long_, short, long_, short, short, long_, "e", short, long_ - 1, short, long_]
                us = struct_doc(seq)
                d = c.add(us)
                heads |= {(short, h) for n, h, _ in placements(us, c.b0[d]) if n == short}
    return c, heads


def _mixed_shape_corpus():
    """Appends (an origin alone: 7 to 10 struct bytes with these ids) and mid-text inserts (both origins: 13 to 17) of
    one to four clients, as a debounce log mixes them."""
    c = Corpus()
    for ncl in (1, 2, 3, 4):
        for k in (7, 23, 40):
            c.add(fast_doc(k, [3000000001, 77, 2 ** 31 + 5, 12345][:ncl], [100, 2 ** 14 - 9, 2 ** 21 - 5, 120][:ncl], seed=k + ncl))
            c.add(fast_doc(k, [B, A, 70000, 9][:ncl], seed=k))
    return c


# ======================================================================= vote and placement
SMALL = [5, 9, 70, 200, 33]
BIG = [3000000001, 77, 2 ** 31 + 5, 12345, 999]
TOP_BIT = [0x12345678, 0x92345678, 0x00000001, 0x80000001]           # pairs that differ only in bit 31
FIFTH = [0x00ABCDEF, 0x10ABCDEF, 0x20ABCDEF, 0xF0ABCDEF]             # ids that differ only in the fifth varuint byte


def _order_corpus():
    """Every order of first sight of one to five clients (the first n updates name them in that order), one- and
    two-byte ids and five-byte ones."""
    c = Corpus()
    for ids in (SMALL, BIG):
        for ncl in (1, 2, 3, 4, 5):
            for perm in itertools.permutations(ids[:ncl]):
                c.add(fast_doc(ncl + 3 + ncl % 2, list(perm), seed=ncl))
    return c


def _near_id_corpus():
    c = Corpus()
    for ids in (TOP_BIT, FIFTH):
        for perm in itertools.permutations(ids):
            c.add(fast_doc(14, list(perm), seed=1))
        for pair in itertools.permutations(ids, 2):
            c.add(fast_doc(7, list(pair), [2 ** 14 - 3, 125], seed=2))
    return c


def _deletion_client_corpus():
    """A client that only a delete set names (it has no structs in the document): one deletion, several, and as the
    only update beside one insert; ids above, between and below the struct clients'."""
    c = Corpus()
    for ghost in (3, 100, 2 ** 32 - 1):
        for ncl in (1, 2, 4):
            ids = [B, A, 70000, 9][:ncl]
            g = Log(ids, [7] * ncl, seed=ghost & 0xFF)
            for j in range(9):
                if j in (2, 6):
                    g.raw(b"\x00" + _ds([(ghost, [(4 + j, 2)])]))
                else:
                    g.plain(ids[j % ncl])
            c.add(g.ups)
        g = Log([A], [7], seed=1)
        g.plain(A)
        g.raw(b"\x00" + _ds([(ghost, [(1, 1)])]))
        c.add(g.ups)
    return c


def _block255_corpus():
    """A block of 255 records (the most a document holds), alone and beside nothing else: one- and two-byte ids keep
    255 updates inside the staged bytes."""
    c = Corpus()
    c.add(fast_doc(255, [A], seed=1))
    c.add(fast_doc(255, [B], [120], seed=2))
    return c


def _fault_doc(ids, who, shift, seed, k=24):
    """Round robin over ids; the third update of client `who` has its clock shifted by `shift` (the later ones follow
    on: one gap or one overlap).  who None: a clean document."""
    g = Log(ids, [9] * len(ids), seed)
    seen = 0
    for j in range(k):
        cl = ids[j % len(ids)]
        if cl == who:
            seen += 1
        if cl == who and seen == 3:
            g.put(cl, [item(4, text("z"), origin=g.last)], 1, shift=shift)
        else:
            g.plain(cl)
    return g.ups


def _fault_corpus():
    """One clock gap and one overlap in the block of every rank, of one to four blocks: deferred, beside a clean twin."""
    c = Corpus()
    for ids in (SMALL, BIG):
        for ncl in (1, 2, 3, 4):
            for who in ids[:ncl]:                       # (the ids are in no order: every rank is some client's)
                for shift in (1, -1):
                    c.add(_fault_doc(ids[:ncl], who, shift, seed=ncl), "bad")
            c.add(_fault_doc(ids[:ncl], None, 0, seed=ncl))
    return c


# ======================================================================= every corpus by its key
CORPORA = [("clck", _client_clock_corpus), ("next", _next_byte_corpus), ("fifth", _fifth_byte_corpus),
           ("zero", _client_zero_corpus), ("origin", _origin_corpus), ("ds", _ds_corpus),
           ("lengths", lambda: _every_length_corpus()[0]), ("widths", lambda: _width_corpus()[0]),
           ("packed", lambda: _packed_corpus()[0]), ("mixed", _mixed_shape_corpus), ("order", _order_corpus),
           ("near", _near_id_corpus), ("ghost", _deletion_client_corpus), ("b255", _block255_corpus),
           ("fault", _fault_corpus)]

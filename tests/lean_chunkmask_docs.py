"""The corpora of test_lean_chunkmask.py: the narrow lean merge kernel where its fast parse takes the two varuint byte masks (top bit set, zero byte) from bit
arrays made once per staged 16-byte chunk, and reads a 16-byte window.  What can go wrong there depends on where an
update lies in the staged document, so every corpus here is laid out in one arena with each document's residue (its
first byte's arena offset mod 16) chosen, by clean filler documents of the right length in front of it:

  alignment   clean all-fast documents at every residue, their updates starting at every bit offset of a mask dword;
  non-minimal a `0x80 0x00` varuint tail (and one run of seven continuation bytes) in the client, the clock, the origin
              clock and the right-origin clock, the pair at every offset of a chunk -- split across the chunk edge, and
              across staged bytes 1023 | 1024 -- each beside a clean twin;
  neighbours  a top-bit byte right before a clean document, 0x00 / 0x80 right after one, a delete-set-only update right
              after a top-bit byte;
  capacity    200 updates filling the staged buffer to its last chunk, its last halfword, one byte into its last chunk;
  widths      structs of 14 to 23 bytes at every offset of an output dword: both sides of each copy width;
  reuse       one wave per CU taking a long document, then a short one, then one with a slow row.

A clean document is never deferred, a document with a non-minimal varuint is never taken.  (Documents have 2 to 40
updates, except the 1023 | 1024 split, the capacity and the reuse documents.)  tests/test_lean_docs.py takes the
census of the corpora on the CPU."""
from lean_docs import Log, _ds, fast_doc, item, overlong, text, upd
from v1util import vu

A, B = 5, 200                     # a one- and a two-byte client id
C5 = 0xFFFFFF01                   # a five-byte one


# ======================================================================= the arena layout
def _fillers():
    """Clean all-fast documents by total length mod 16."""
    pool = {}
    for k in range(2, 16):
        for ids in ([A], [B], [70000], [3000000001], [A, B], [B, 70000]):
            us = fast_doc(k, ids, seed=k)
            pool.setdefault(sum(map(len, us)) % 16, us)
    assert set(pool) >= set(range(1, 16))
    return pool


FILL = _fillers()


class Corpus:
    """Documents in arena order; kind 'clean' / 'fill' (finished by the lean kernel) or 'bad' (never taken by it)."""

    def __init__(self):
        self.docs, self.kind, self.b0, self.at = [], [], [], 0

    def add(self, us, kind, residue=None):
        """Appends the document, at the arena residue asked for (a filler goes in front when needed); returns its index."""
        if residue is not None and (residue - self.at) % 16:
            self.add(FILL[(residue - self.at) % 16], "fill")
        assert residue is None or self.at % 16 == residue
        self.docs.append(us)
        self.kind.append(kind)
        self.b0.append(self.at)
        self.at += sum(map(len, us))
        return len(self.docs) - 1

    def staged(self, d):
        """Staged positions of document d's updates: the kernel stages it from its 16-byte granule."""
        p, out = self.b0[d] % 16, []
        for u in self.docs[d]:
            out.append(p)
            p += len(u)
        return out

    def lean(self):
        return sum(k != "bad" for k in self.kind)

    def bit_offsets(self):
        return {s & 31 for d in range(len(self.docs)) if self.kind[d] != "bad" for s in self.staged(d)}


# ======================================================================= alignment
ALIGN_IDS = [[A], [B, A], [3000000001, 77], [2 ** 31 + 5, 12345, 9], [70000], [C5, A, B, 999]]


def _align_corpus():
    c = Corpus()
    for r in range(16):
        c.add(fast_doc(24 + r, ALIGN_IDS[r % len(ALIGN_IDS)], [100 + r] * 4, seed=r), "clean", residue=r)
    return c


# ======================================================================= non-minimal varuints
FIELDS = ["client", "clock", "origin", "right"]
_PART = {"client": 1, "clock": 2, "origin": 5, "right": 7}


def shaped(c, ck, o, r, over=None, long_run=False):
    """One character with both origins.  over: that field's varuint is non-minimal; long_run: the origin clock is an
    eight-byte varuint.  Returns the update and the offset in it of the first byte of the pair / the run."""
    p = [b"\x01\x01", vu(c), vu(ck), b"\xC4", vu(o[0]), vu(2 ** 49 + 5 if long_run else o[1]), vu(r[0]), vu(r[1]), b"\x01q", b"\x00"]
    off = None
    if over:
        i = _PART[over]
        p[i] = overlong(p[i])
        off = len(b"".join(p[:i])) + len(p[i]) - 2
    if long_run:
        off = len(b"".join(p[:5]))
    return b"".join(p), off


def nonmin_doc(k, at, over=None, long_run=False, ids=(A, B), seed=0):
    """k updates of two clients, alternating; update `at` is `shaped`.  Returns the document and the offset in it of
    the pair's first byte (None for the clean twin, whose update `at` is the same with minimal varuints)."""
    g = Log(list(ids), [90, 120], seed)
    off = None
    for j in range(k):
        c = ids[j % 2]
        if j != at:
            g.plain(c)
            continue
        u, o = shaped(c, g.clock[c], g.last, (ids[0], 3), over, long_run)
        if o is not None:
            off = sum(map(len, g.ups)) + o
        g.raw(u)
        g.last = (c, g.clock[c])
        g.clock[c] += 1
    assert all(len(u) <= 32 for u in g.ups)
    return g.ups, off


def _nonmin_corpus():
    """Per field and residue r a document with the pair at staged position r + off (off is the same for every r: the
    pair visits every offset of a chunk) and its clean twin; then the 1023 | 1024 split; then the eight-byte run."""
    c, pos = Corpus(), {f: [] for f in FIELDS + ["run"]}
    for i, f in enumerate(FIELDS):
        ids = (A, B) if i % 2 else (B, 3000000001)
        for r in range(16):
            us, off = nonmin_doc(7, 4 + i % 2, over=f, ids=ids, seed=i)
            c.add(us, "bad", residue=r)
            pos[f].append(r + off)
            c.add(nonmin_doc(7, 4 + i % 2, ids=ids, seed=i)[0], "clean")
    for f in FIELDS:        # the pair's first byte at staged byte 1023: the last byte of lane 63's first chunk
        for at in range(40, 120):
            us, off = nonmin_doc(at + 3, at, over=f, seed=at)
            if 1008 <= off <= 1023:
                break
        c.add(us, "bad", residue=1023 - off)
        pos[f].append(1023)
        c.add(nonmin_doc(at + 3, at, seed=at)[0], "clean", residue=1023 - off)
    for r in range(16):
        us, off = nonmin_doc(6, 3, long_run=True, seed=r)
        c.add(us, "bad", residue=r)
        pos["run"].append(r + off)
        c.add(nonmin_doc(6, 3, seed=r)[0], "clean")
    return c, pos


# ======================================================================= neighbours
def _clean(k, seed, ids=(A, B)):
    return fast_doc(k, list(ids), [40, 50], seed=seed)


def _neighbour_corpus():
    c = Corpus()
    for r in range(16):
        # a document that ends in a top-bit byte (its last delete set's count is cut off), the clean one right after it
        pred = _clean(3, r)
        pred[-1] = pred[-1][:-1] + bytes([0x80 | r])
        c.add(pred, "bad", residue=(r - sum(map(len, pred))) % 16)
        d = c.add(_clean(5 + r, r + 1), "clean")
        assert c.b0[d] % 16 == r
        # ... and right after the clean one a document that starts with 0x00 (a deletion with an empty delete set: clean
        # itself) or with 0x80 | 1, 0x00 (a non-minimal block count)
        g = Log([A, B], [7, 7], r)
        g.raw(b"\x00\x00")
        for j in range(3):
            g.plain((A, B)[j % 2])
        if r % 2:
            c.add(g.ups, "clean")
        else:
            c.add([b"\x81\x00" + _clean(2, r)[0][1:]] + _clean(2, r)[1:], "bad")
    for r in range(16):
        # a delete-set-only update right after an update whose last byte has the top bit (its delete set's last varuint
        # is cut off: the document is malformed), at every residue; the same with the whole delete set is clean
        for last, kind in ((bytes([0x80 | (r + 1)]), "bad"), (b"\x01", "clean")):
            g = Log([A, B], [7, 7], r)
            g.plain(A)
            g.put(B, [item(4, text("q"), origin=g.last)], 1, ds=b"\x01" + vu(A) + b"\x01" + vu(4) + last)
            g.raw(b"\x00" + _ds([(A, [(2, 1)])]))
            g.plain(A)
            c.add(g.ups, kind, residue=r if kind == "bad" else None)
    return c


# ======================================================================= capacity
STAGED = 5120                      # the narrow kernel's staged bytes
K_CAP = 200


def _sized(c, ck, n):
    """One character of client c (five id bytes) at clock ck (four bytes) in exactly n bytes, 17 <= n <= 32."""
    m = n - 15                     # bytes of the origin ids: (client, clock), once or twice
    width = lambda w: 3 if w == 1 else 2 ** (7 * (w - 1)) + 3
    if m <= 9:
        oc = min(5, m - 1)
        u = upd(c, ck, [item(4, text("q"), origin=(width(oc), width(m - oc)))])
    else:
        w = [1, 1, 1, 1]
        lim = [5, 4, 5, 4]
        for _ in range(m - 4):
            i = max(range(4), key=lambda j: lim[j] - w[j])
            w[i] += 1
        u = upd(c, ck, [item(4, text("q"), origin=(width(w[0]), width(w[1])), right=(width(w[2]), width(w[3])))])
    assert len(u) == n, (n, len(u))
    return u


def _cap_doc(nbytes):
    ck = 2 ** 21 + 5
    us = [upd(C5, ck, [item(4, text("a"))])]
    rest = nbytes - len(us[0])
    base, extra = divmod(rest, K_CAP - 1)
    for j in range(1, K_CAP):
        us.append(_sized(C5, ck + j, base + (1 if j <= extra else 0)))
    assert sum(map(len, us)) == nbytes and len(us) == K_CAP
    return us


CAP_FILL = [5120, 5119, 5105]      # the last chunk whole, the last halfword short of one bit, one byte in the last chunk


def _cap_corpus():
    c = Corpus()
    for fill in CAP_FILL:
        for r in (0, 9, 15):
            c.add(_cap_doc(fill - r), "clean", residue=r)
    return c


# ======================================================================= struct widths around the copy classes
def _width_doc(sb, k, c=A):
    """k one-character Items of client c whose structs are sb bytes each (both origins; 14 <= sb <= 23): in the merged
    block they lie back to back, so with an odd sb they start at every offset of an output dword."""
    w, lim = [1, 1, 1, 1], [5, 5, 5, 5]
    for _ in range(sb - 3 - 4):
        i = max(range(4), key=lambda j: lim[j] - w[j])
        w[i] += 1
    val = lambda n: 3 if n == 1 else 2 ** (7 * (n - 1)) + 3
    us = [upd(c, 0, [item(4, text("a"))])]
    for j in range(1, k):
        us.append(upd(c, j, [item(4, text("q"), origin=(val(w[0]), val(w[1])), right=(val(w[2]), val(w[3])))]))
        assert len(us[-1]) == 2 + len(vu(c)) + 1 + sb + 1
    return us


def _width_corpus():
    """A struct's run in the output is its offset in the dword plus its bytes: 14 to 26 here, on both sides of the
    widths at which the copy takes another number of dwords (20 | 21, 24 | 25)."""
    c = Corpus()
    for sb in range(14, 24):
        c.add(_width_doc(sb, 9 + sb % 4), "clean")
        c.add(_width_doc(sb, 40, c=B) + _width_doc(14, 3, c=A), "clean")
    return c


# ======================================================================= reuse: one wave, document after document
POOL = 8


def _reuse_pool():
    """Per kind POOL documents and whether the lean kernel finishes them: long (200 updates of large ids: many top-bit
    bytes, and zero bytes in the origin clocks), short, and one with a slow row (a longer string, a ContentDeleted --
    both the lean kernel's -- or a non-minimal clock, which is not)."""
    long_ = [fast_doc(200, [3000000001 + j, 2 ** 31 + 128 * j], [2 ** 14 - 100, 2 ** 21 - 100], seed=j) for j in range(POOL)]
    assert all(4000 < sum(map(len, us)) <= STAGED - 16 for us in long_)
    short = [fast_doc(2 + j % 5, [[A], [B, A], [3000000001, 77]][j % 3], seed=j) for j in range(POOL)]
    slow, lean = [], []
    for j in range(POOL):
        g = Log([A, B], [5, 5], j)
        for i in range(9 + j):
            c = (A, B)[i % 2]
            if i != 5:
                g.plain(c)
            elif j % 3 == 0:
                g.put(c, [item(4, text("abcde"), origin=g.last)], 5)
            elif j % 3 == 1:
                g.put(c, [item(1, vu(3), origin=g.last)], 3)
            else:
                g.put(c, [item(4, text("q"), origin=g.last)], 1, clock_bytes=overlong(vu(g.clock[c])))
        slow.append(g.ups)
        lean.append(j % 3 != 2)
    return [long_, short, slow], [[True] * POOL, [True] * POOL, lean]

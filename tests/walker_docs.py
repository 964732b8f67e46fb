"""Hand-built update-V1 documents and state vectors for the SV / diff ring walker (dw_walk<MODE, GATHER> in
ygm_walk.hip, k_sv_table before it): every item sits on an edge of the walker's envelope, of its 64-byte window, of its
256-byte ring, of its re-encoded headers, or on plumbing that exists only on the GPU (the arena residue of a document,
the batch split, the shared-state plan).

An item is `(name, update, sv, label_sv, label_diff, valid)`.  A label says who finishes the document: "walker", or
"exact" (the walker appends it to defer_list and k_doc answers).  The labels come from `label()`, a restatement in
Python of the envelope documented in the header of ygm_doc_walk.hpp and above k_sv_table; nothing is read from the
library.  `valid` says that yjs answers both operations (the tests ask the oracle for the bytes either way).

`families()` maps a family letter to a list of batches, a batch being a list of items packed one after the other the
way Engine._pack does (`offsets`).  Pure Python, deterministic: no library, no torch (`expected` alone asks the oracle)."""
import random

from v1util import encode_ds, vu

WALKER, EXACT = "walker", "exact"
SV_MAX_ENTRIES, SV_MAX_BYTES = 16, 160
SV0 = b"\x00"


# ---------------------------------------------------------------- the envelope, as a predicate over the bytes
class _Defer(Exception):
    pass


def _term(b, p, lim):
    """Position of the first byte >= p with its top bit clear, below lim; else the walker sees no end: defer."""
    while p < lim:
        if b[p] < 0x80:
            return p
        p += 1
    raise _Defer


def _val(b, p, lim):
    """A varuint of <= 5 bytes below 2^32 at p -> (value, position after); anything else defers."""
    e = _term(b, p, min(lim, p + 5))
    v = 0
    for k in range(p, e + 1):
        v |= (b[k] & 0x7F) << (7 * (k - p))
    if v >> 32:
        raise _Defer
    return v, e + 1


def _skip(b, p, lim):
    """A varuint the walker copies without reading its value (origin ids, parent ids, delete ranges)."""
    return _term(b, p, lim) + 1


def _ascii_str(b, q, p, n):
    """A y-key, parentSub or type-name string at struct-relative p: ASCII, ending inside the struct's 64-byte window."""
    ln, s = _val(b, q + p, min(n, q + 64))
    f = s - q + ln
    if f > 64 or q + f > n or any(x >= 0x80 for x in b[s:s + ln]):
        raise _Defer
    return f


def sv_table(sv):
    """k_sv_table: {client: clock} (a repeated client's last entry wins), or None for a vector left to the exact kernel:
    empty bytes, more than 160 bytes, a count above 16, a value of more than 5 bytes or >= 2^32, truncated, trailing."""
    n = len(sv)
    if n == 0 or n > SV_MAX_BYTES:
        return None
    try:
        cnt, p = _val(sv, 0, n)
        if cnt > SV_MAX_ENTRIES:
            return None
        t = {}
        for _ in range(cnt):
            c, p = _val(sv, p, n)
            k, p = _val(sv, p, n)
            t[c] = k
    except _Defer:
        return None
    return t if p == n else None


def label(u, sv, mode):
    """Who finishes `u` in mode "sv" / "diff" (diff: against state vector `sv`)."""
    u = bytes(u)
    n = len(u)
    diff = mode == "diff"
    run = 0
    for i, x in enumerate(u):                      # byte patterns, anywhere in the document
        run = run + 1 if x & 0x80 else 0
        if run >= 6:
            return EXACT
        if diff and x == 0 and i and u[i - 1] & 0x80:
            return EXACT
    tbl = sv_table(sv) if diff else {}
    if tbl is None or n == 0 or n >> 30:
        return EXACT
    try:
        nb, p = _val(u, 0, n)
        prevc = None
        for _ in range(nb):
            nst, p = _val(u, p, n)
            cl, p = _val(u, p, n)
            clock, p = _val(u, p, n)
            if nst == 0 or (prevc is not None and cl >= prevc):
                raise _Defer
            prevc = cl
            for _ in range(nst):
                q = p
                if q >= n:
                    raise _Defer
                info = u[q]
                if (info & 31) == 0 or info == 10:            # GC / Skip
                    if info not in (0, 10):
                        raise _Defer
                    ln, p = _val(u, q + 1, n)
                    if ln == 0:
                        raise _Defer
                else:
                    ref = info & 31
                    if (info & 0xC0) and (info & 0x20):
                        raise _Defer
                    lim = min(n, q + 64)
                    if info & 0xC0:
                        c = q + 1
                        for _ in range(4 if (info & 0xC0) == 0xC0 else 2):
                            c = _skip(u, c, lim)
                        cs = c - q
                    else:
                        pi, c = _val(u, q + 1, lim)
                        if pi > 1:
                            raise _Defer
                        if pi == 1:
                            cs = _ascii_str(u, q, c - q, n)
                        else:
                            cs = _skip(u, _skip(u, c, lim), lim) - q
                        if info & 0x20:
                            if cs >= 64:
                                raise _Defer
                            cs = _ascii_str(u, q, cs, n)
                    if cs >= 60:                              # the content starts at or past byte 60 of the struct
                        raise _Defer
                    v, c = _val(u, q + cs, lim)
                    if ref == 1:
                        ln, p = v, c
                    elif ref in (3, 4):
                        ln, p = (v if ref == 4 else 1), c + v
                        if p > n or (ref == 4 and any(x >= 0x80 for x in u[c:p])):
                            raise _Defer
                    elif ref == 7:
                        if v > 6:
                            raise _Defer
                        ln, p = 1, c
                        if v in (3, 5):
                            p = q + _ascii_str(u, q, c - q, n)
                    else:
                        raise _Defer
                    if ln == 0:
                        raise _Defer
                if clock + ln >= 1 << 32 or p > n:
                    raise _Defer
                clock += ln
        if diff:                                              # the delete set, copied verbatim
            nc, p = _val(u, p, n)
            prevc = None
            for _ in range(nc):
                c, p = _val(u, p, n)
                k, p = _val(u, p, n)
                if k == 0 or (prevc is not None and c >= prevc):
                    raise _Defer
                prevc = c
                for _ in range(k):
                    p = _skip(u, _skip(u, p, n), n)
    except _Defer:
        return EXACT
    return WALKER


def mk(name, u, sv=SV0, valid=True):
    u, sv = bytes(u), bytes(sv)
    return (name, u, sv, label(u, sv, "sv"), label(u, sv, "diff"), valid)


def offsets(batch, what=1):
    """Arena offsets of a batch's updates (what = 1) or state vectors (2), packed back to back."""
    o, out = 0, []
    for it in batch:
        out.append(o)
        o += len(it[what])
    return out + [o]


# ---------------------------------------------------------------- building blocks
ROOT = b"\x01\x01t"


def item(ref, content, origin=None, right=None, parent=ROOT, sub=None, info_or=0):
    info = ref | (0x80 if origin else 0) | (0x40 if right else 0) | (0x20 if sub is not None else 0) | info_or
    b = bytes([info])
    for o in (origin, right):
        if o:
            b += o if isinstance(o, bytes) else vu(o[0]) + vu(o[1])
    if not origin and not right:
        b += parent
        if sub is not None:
            b += vu(len(sub)) + sub
    return b + content


def s(txt, **kw):
    raw = txt.encode() if isinstance(txt, str) else bytes(txt)
    return item(4, vu(len(raw)) + raw, **kw)


def dl(n, **kw):
    return item(1, vu(n), **kw)


def binary(raw, **kw):
    return item(3, vu(len(raw)) + bytes(raw), **kw)


def ytype(ref, name=None, **kw):
    return item(7, vu(ref) + (vu(len(name)) + name if name is not None else b""), **kw)


def gc(n):
    return b"\x00" + vu(n)


def skip(n):
    return b"\x0a" + vu(n)


def block(client, clock, structs, nst=None):
    cl = client if isinstance(client, bytes) else vu(client)
    ck = clock if isinstance(clock, bytes) else vu(clock)
    return (nst if isinstance(nst, bytes) else vu(len(structs) if nst is None else nst)) + cl + ck + b"".join(structs)


def update(blocks, ds=()):
    return vu(len(blocks)) + b"".join(blocks) + (ds if isinstance(ds, bytes) else encode_ds(list(ds)))


def svec(entries):
    return vu(len(entries)) + b"".join(vu(c) + vu(k) for c, k in entries)


def text(n, salt=0):
    return bytes(97 + (i + salt) % 26 for i in range(n))


def filler(size):
    """A one-string document of exactly `size` bytes, 11 .. 400."""
    for hdr in (10, 11):
        u = update([block(5, 0, [s(text(size - hdr))])])
        if len(u) == size:
            return u
    raise ValueError(size)


def chain(client, k, width=2, first_clock=0):
    """k strings typed one after the other: the first under the root, the others fast-shaped (origin, <= 32 bytes)."""
    out, ck = [], first_clock
    for i in range(k):
        t = text(width, i)
        out.append(s(t, origin=(client, ck - 1)) if ck else s(t))
        ck += width
    return out


def aligned(items, mod=128):
    """The items with a filler in front of each, so that each starts at a multiple of `mod` of the arena."""
    out, o = [], 0
    for it in items:
        pad = (-o) % mod
        if pad:
            pad += mod * ((11 - pad + mod - 1) // mod) if pad < 11 else 0
            out.append(mk("filler %d" % pad, filler(pad)))
            o += pad
        out.append(it)
        o += len(it[1])
    return out


# ---------------------------------------------------------------- A: placement
def probes():
    ds300 = [(9, [(200 + 7 * k, 3) for k in range(100)])]
    cutdoc = update([block(5, 0, [s(text(20)), s(text(20, 3), origin=(5, 19)), dl(9, origin=(5, 39))])], [(5, [(3, 2)])])
    p = [mk("A three fast Items", update([block(5, 1, chain(5, 3, first_clock=1))])),
         mk("A 300-byte string", update([block(5, 0, [s(text(300))])])),
         mk("A cut", cutdoc, svec([(5, 27)])),
         mk("A 300-byte delete set", update([block(5, 0, [s("ab")])], ds300)),
         mk("A 64 bytes", filler(64)), mk("A 128 bytes", filler(128)),
         mk("A 00 00", b"\x00\x00"),
         mk("A deleted and gc", update([block(7, 3, [dl(5, origin=(7, 2)), gc(4), dl(70000, origin=(7, 11))])]), svec([(7, 10)])),
         mk("A two clients", update([block(300, 0, chain(300, 4)), block(5, 0, chain(5, 2))], [(300, [(1, 1)])]), svec([(5, 1), (300, 3)])),
         mk("A binary 80", update([block(5, 0, [binary(text(80))])]))]
    assert len(encode_ds(ds300)) >= 300
    return p


def family_a():
    ps = probes()
    res, o = [], 0
    for r in range(128):
        for pr in ps:
            pad = (r - o) % 128
            if pad < 11:
                pad += 128
            res.append(mk("A filler", filler(pad)))
            res.append((pr[0] + " @%d" % r,) + pr[1:])
            o += pad + len(pr[1])
    last = [[mk("A filler", filler(11 + 13 * k)), pr] for k, pr in enumerate(ps)]
    sweep = aligned([mk("A end residue %d" % (L % 64), filler(L)) for L in range(140, 204)], 64)
    return [res] + last + [sweep]


# ---------------------------------------------------------------- B: strings, keys and the ring
STR_LENS = list(range(55, 67)) + [127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 1000, 5000]


def two_byte(n, i):
    """n bytes of text with a two-byte UTF-8 character at bytes i, i + 1."""
    return text(i) + "é".encode() + text(n - i - 2, 5)


def family_b():
    b1 = []
    for ln in (27, 28, 29):
        u = update([block(5, 0, [s("ab"), s(text(ln), origin=(5, 1))])])
        b1.append(mk("B fast struct of %d bytes" % (4 + ln), u, svec([(5, 1)])))
    for n in STR_LENS:
        b1.append(mk("B string %d" % n, update([block(5, 0, [s(text(n))])])))
    # one two-byte character: doc header 4 bytes (blocks, structs, client, clock), struct header 4, the length's varuint
    utf = []
    for n in STR_LENS:
        head = 4 + len(vu(n))                      # struct-relative start of the string's bytes
        at = {0, 1, n - 2}
        at |= {r - head for r in (62, 63, 64, 65) if 0 <= r - head <= n - 2}
        for i in sorted(at):
            utf.append(mk("B string %d, two-byte character at %d" % (n, i), update([block(5, 0, [s(two_byte(n, i))])])))
    seam = []
    for n in STR_LENS:
        head = 4 + 4 + len(vu(n))                  # arena-relative, the document 64-aligned
        for k in (63, 127, 255, 319):
            if 0 <= k - head <= n - 2:
                seam.append(mk("B string %d, two-byte character over seam %d" % (n, k + 1), update([block(5, 0, [s(two_byte(n, k - head))])])))
    b2 = aligned(seam, 64) + utf
    b3 = [mk("B binary %d" % n, update([block(5, 0, [binary(text(n))])])) for n in (0, 3, 80, 300)]
    b3.append(mk("B binary with a 6-run", update([block(5, 0, [binary(text(20) + b"\xff" * 6 + text(20))])])))
    b3.append(mk("B binary with 80 00", update([block(5, 0, [binary(text(20) + b"\x80\x00" + text(20))])])))
    b3.append(mk("B binary 300 with 80 00 late", update([block(5, 0, [binary(text(280) + b"\x80\x00" + text(18))])])))
    for cs in (55, 56, 57, 58, 59, 60):            # info, parent info 1, key length, key: cs = 3 + key
        key = text(cs - 3)
        b3.append(mk("B y-key, content at %d" % cs, update([block(5, 0, [s("xyz", parent=b"\x01" + vu(len(key)) + key)])])))
        b3.append(mk("B y-key, deleted at %d" % cs, update([block(5, 0, [dl(7, parent=b"\x01" + vu(len(key)) + key)])])))
    for end in (63, 64, 65):
        for cs in (40, 57):                        # type ref at cs, the name's length at cs + 1
            key = text(cs - 3)
            name = text(end - cs - 2, 7)
            for ref in (3, 5):
                b3.append(mk("B type %d name ends at %d, content at %d" % (ref, end, cs),
                             update([block(5, 0, [ytype(ref, name, parent=b"\x01" + vu(len(key)) + key), s("q", origin=(5, 0))])])))
        sub = text(end - 7 - 1, 3)                 # info, parent id (0, client 5-byte, clock) = 1 + 5 + 1 = 7, then the length
        b3.append(mk("B parentSub ends at %d" % end, update([block(5, 0, [s("v", parent=b"\x00" + vu(0xFFFFFFF0) + b"\x00", sub=sub)])])))
        key = text(end - 3, 2)
        b3.append(mk("B y-key ends at %d" % end, update([block(5, 0, [s("v", parent=b"\x01" + vu(len(key)) + key)])])))
    key = text(53) + b"\x00"                       # info, parent info, key length, 54 key bytes: the parentSub's length at 57
    b3.append(mk("B parentSub length at 57 after a key ending in 00", update([block(9, 0, [s("v", parent=b"\x01" + vu(54) + key, sub=b"k")])])))
    for k in (50, 51, 52, 53):                     # parent id, then a parentSub whose length byte is at 55 .. 58
        par = b"\x00" + vu(0xFFFFFFF0) + vu(7)     # 7 bytes: the parentSub length at struct byte 8
        b3.append(mk("B parentSub of %d, content at %d" % (k, 9 + k), update([block(5, 0, [s("v", parent=par, sub=text(k))])])))
    for tr in range(8):
        b3.append(mk("B type ref %d" % tr, update([block(5, 0, [ytype(tr, b"p" if tr in (3, 5) else None)])]), valid=tr < 7))
    return [b1, b2, b3]


# ---------------------------------------------------------------- C: cuts
def family_c():
    out = []
    shapes = {"origin": dict(origin=(5, 0)), "origin+right": dict(origin=(5, 0), right=(3, 1)),
              "origin+right 5-byte ids": dict(origin=(0xF0000005, 0x10000000), right=(0xF0000003, 0x10000001)),
              "y-key parent": dict(parent=b"\x01\x04root"), "parent id": dict(parent=b"\x00" + vu(3) + vu(1)),
              "parentSub": dict(parent=b"\x01\x01t", sub=b"key")}
    kinds = {"short string": (lambda kw: s(text(9), **kw), 9), "string 300": (lambda kw: s(text(300), **kw), 300),
             "string 1000": (lambda kw: s(text(1000), **kw), 1000), "deleted 2": (lambda kw: dl(2, **kw), 2),
             "deleted 70000": (lambda kw: dl(70000, **kw), 70000)}
    for kn, (mkst, ln) in kinds.items():
        offs = [1, ln - 1] + ([63, 64, 65, 255, 256, 257] if ln >= 300 else [])
        for sn, kw in shapes.items():
            u = update([block(5, 1, [mkst(kw), s("zz", origin=(5, ln))])])
            for off in sorted(set(offs)):
                if 0 < off < ln:
                    out.append(mk("C cut %s, %s, offset %d" % (kn, sn, off), u, svec([(5, 1 + off)])))
    for ln in (2, 70000):
        u = update([block(5, 4, [gc(ln), s("zz", origin=(5, 3 + ln))])])
        for off in (1, ln - 1):
            out.append(mk("C cut gc %d, offset %d" % (ln, off), u, svec([(5, 4 + off)])))
    c1 = out
    # the state vector's clock against the struct boundaries of one block (first clock 10, three strings of 5)
    c2 = []
    b3 = [s(text(5), origin=(5, 9)), s(text(5, 1), origin=(5, 14)), s(text(5, 2), origin=(5, 19))]
    u = update([block(9, 0, chain(9, 2)), block(5, 10, b3), block(2, 0, chain(2, 2))], [(5, [(11, 2)])])
    for k in (0, 9, 10, 11, 14, 15, 16, 19, 20, 21, 24, 25, 28):
        c2.append(mk("C clock %d in a block of 10 .. 25" % k, u, svec([(5, k), (9, 2)])))
    for where, structs in (("before", [skip(4)] + b3[1:]), ("at", [b3[0], skip(5), b3[2]]), ("after", b3[:2] + [skip(5)])):
        us = update([block(5, 10, [s(text(5), origin=(5, 9))] + structs if where == "before" else structs)], [])
        for k in (10, 12, 15, 17, 20, 22, 25):
            c2.append(mk("C skip %s the cut, clock %d" % (where, k), us, svec([(5, k)])))
    # varuint-length edges of the re-encoded header
    for left in (127, 128):
        st = [s(text(4), origin=(5, 0))] + [s("x", origin=(5, 4 + i)) for i in range(left)]
        c2.append(mk("C %d structs left after the cut one's" % left, update([block(5, 1, st)]), svec([(5, 3)])))
    for edge in (127, 128, 16383, 16384, 1 << 28):
        for d in (0, 1):                            # header clock = edge (d = 0), origin clock = clock + off - 1 = edge (d = 1)
            first = max(edge - 3, 0)
            u = update([block(5, first, [s(text(9), origin=(5, first - 1)) if first else s(text(9)), s("y", origin=(5, first + 8))])])
            c2.append(mk("C header clock %d" % (edge + d), u, svec([(5, edge + d)])))
    big = 0xF1234567
    u = update([block(big, 0, [s(text(9)), dl(5, origin=(big, 8), right=(big - 1, 0x0FFFFFFF))])])
    for k in (4, 9, 11):
        c2.append(mk("C 5-byte client, clock %d" % k, u, svec([(big, k)])))
    return [c1, c2]


# ---------------------------------------------------------------- D: state vectors
def family_d():
    doc = update([block(c, 0, chain(c, 3)) for c in range(40, 20, -1)], [(30, [(0, 1)])])
    out = []

    def add(name, sv, valid=True):
        out.append(mk("D " + name, doc, sv, valid))

    ents = [(c, 1 + c % 5) for c in range(21, 41)]
    for n in (0, 1, 8, 9, 16, 17):
        add("%d entries" % n, svec(ents[:n]))
    wide = [(0xF0000000 + c, 0x10000000 + c) for c in range(16)]      # 10 bytes an entry
    sv160 = vu(16) + b"".join(vu(c) + vu(k) for c, k in wide[:15]) + vu(0xF0000F0F) + vu(0x7FFFFFF)
    assert len(sv160) == 160
    add("160 bytes", sv160)
    add("161 bytes", vu(16) + b"".join(vu(c) + vu(k) for c, k in wide))
    add("a repeated client", svec([(30, 1), (25, 2), (30, 4)]))
    add("16 distinct and a repeat", svec(ents[:16] + [ents[3]]))
    add("ascending", svec(ents[:12]))
    add("descending", svec(ents[:12][::-1]))
    sh = ents[:12]
    random.Random(5).shuffle(sh)
    add("shuffled", svec(sh))
    add("clients the document lacks", svec([(1000, 5), (30, 2), (7, 1)]))
    add("few of the document's clients", svec([(40, 6), (21, 3)]))
    add("clock 2^32 - 1", svec([(30, 0xFFFFFFFF)]))
    add("clock 2^32", svec([(30, 1 << 32)]))
    add("client 2^32", svec([(1 << 32, 1)]))
    add("a 6-byte varuint", b"\x01\x1e\x80\x80\x80\x80\x80\x01")
    add("a non-minimal clock", b"\x01\x1e\x82\x00")
    full = svec([(30, 2), (0xF0000001, 300), (25, 4)])
    for k in range(len(full)):
        add("truncated at %d" % k, full[:k], valid=False)
    add("one trailing byte", full + b"\x00")
    add("00", b"\x00")
    # every residue mod 16 of the sv arena: sixteen 5-entry vectors behind vectors of odd lengths
    res, o = [], 0
    for r in range(16):
        pad = (r - o) % 16 or 16
        res.append(mk("D sv filler", doc, vu(pad - 1 >> 1) + b"".join(vu(50 + j) + vu(1) for j in range(pad - 1 >> 1)) + (b"" if pad % 2 else b"\x00"), True))
        res.append(mk("D sv @%d" % r, doc, svec(ents[r:r + 5])))
        o += len(res[-2][2]) + len(res[-1][2])
    return [out, res]


# ---------------------------------------------------------------- E: headers, counts, the SV accumulator
def family_e():
    e1 = []
    for n in (1, 2, 15, 16, 17, 127, 128, 129, 300):
        u = update([block(1000 - c, 0, [s("a")]) for c in range(n)])
        e1.append(mk("E %d client blocks" % n, u))
    # entries of 1 .. 5 bytes a number, the first entry varied: the accumulator's fill passes every residue
    sizes = [0x50, 0x2000, 0x100000, 0x8000000, 0xF0000000]
    for lead in range(16):
        cls, bl = [], []
        base = 0xFFFFFF00
        seq = [sizes[(lead + j) % 5] for j in range(12)]
        for j, v in enumerate(seq):
            cl = base - j if v == sizes[4] else v + 200 - j
            cls.append(cl)
        cls = sorted(set(cls), reverse=True)
        for j, cl in enumerate(cls):
            ck = [1, 200, 20000, 3000000, 0x10000000][(lead + 2 * j) % 5]
            bl.append(block(cl, ck, [dl([1, 130, 17000, 2100000][(lead + j) % 4], origin=(cl, ck - 1))]))
        e1.append(mk("E accumulator, lead %d" % lead, update(bl)))
    e1.append(mk("E blocks ascending", update([block(3, 0, [s("a")]), block(4, 0, [s("a")])])))
    e1.append(mk("E equal clients", update([block(4, 0, [s("a")]), block(4, 1, [s("b", origin=(4, 0))])])))
    e1.append(mk("E a block of 0 structs", update([block(4, 0, []), block(3, 0, [s("a")])])))
    for n in (127, 128, 16383, 16384):
        st = [gc(1)] * n                            # (two bytes a struct: the 16 384-struct document stays at 32 KB)
        e1.append(mk("E %d structs" % n, update([block(5, 0, st)]), svec([(5, n - 2)])))
    for ck in (127, 128):
        e1.append(mk("E block clock %d" % ck, update([block(5, ck, [s("ab", origin=(5, ck - 1))])]), svec([(5, ck + 1)])))
    return [e1]


# ---------------------------------------------------------------- F: byte patterns and values
def family_f():
    f1 = []
    NM = b"\x81\x00"                               # 1, non-minimal
    nm = {"blocks": NM + block(5, 0, [s("a")]) + b"\x00",
          "structs": update([block(5, 0, [s("a")], nst=NM)]),
          "client": update([block(b"\x85\x00", 0, [s("a")])]),
          "block clock": update([block(5, NM, [s("a", origin=(5, 0))])]),
          "origin client": update([block(5, 1, [s("a", origin=b"\x85\x00\x00")])]),
          "origin clock": update([block(5, 1, [s("a", origin=b"\x05\x80\x00")])]),
          "parent info": update([block(5, 0, [s("a", parent=b"\x81\x00\x01t")])]),
          "key length": update([block(5, 0, [s("a", parent=b"\x01\x81\x00t")])]),
          "string length": update([block(5, 0, [item(4, NM + b"a")])]),
          "deleted length": update([block(5, 0, [item(1, NM)])]),
          "gc length": update([block(5, 0, [b"\x00" + NM])]),
          "type ref": update([block(5, 0, [item(7, NM)])]),
          "ds clients": update([block(5, 0, [s("a")])], NM + b"\x05\x01\x00\x01"),
          "ds client": update([block(5, 0, [s("a")])], b"\x01\x85\x00\x01\x00\x01"),
          "ds ranges": update([block(5, 0, [s("a")])], b"\x01\x05" + NM + b"\x00\x01"),
          "ds clock": update([block(5, 0, [s("a")])], b"\x01\x05\x01\x80\x00\x01"),
          "ds length": update([block(5, 0, [s("a")])], b"\x01\x05\x01\x00" + NM)}
    for k, u in nm.items():
        f1.append(mk("F non-minimal %s" % k, u))
    f1.append(mk("F clock + len = 2^32 - 1", update([block(5, 0xFFFFFFF0, [dl(15, origin=(5, 0xFFFFFFEF))])])))
    f1.append(mk("F clock + len = 2^32", update([block(5, 0xFFFFFFF0, [dl(16, origin=(5, 0xFFFFFFEF))])])))
    f1.append(mk("F fast, clock + len = 2^32", update([block(5, 0xFFFFFFF0, [dl(3, origin=(5, 0xFFFFFFEF)), dl(13, origin=(5, 0xFFFFFFF2))])])))
    f1.append(mk("F fifth byte 0x70, block clock", update([block(5, b"\x80\x80\x80\x80\x10", [dl(1, origin=(5, 9))])])))
    f1.append(mk("F fifth byte 0x70, client", update([block(b"\x85\x80\x80\x80\x70", 3, [dl(1, origin=(5, 2))])])))
    f1.append(mk("F fifth byte 0x70, deleted length", update([block(5, 3, [item(1, b"\x80\x80\x80\x80\x10", origin=(5, 2))])])))
    f1.append(mk("F fifth byte 0x0F, client", update([block(b"\x85\x80\x80\x80\x0f", 3, [dl(1, origin=(5, 2))])])))
    f1.append(mk("F gc info 0x20", update([block(5, 0, [b"\x20\x03"])])))
    f1.append(mk("F info 0xA4", update([block(5, 1, [s("ab", origin=(5, 0), info_or=0x20)])])))
    f1.append(mk("F parent info 2", update([block(5, 0, [s("a", parent=b"\x02\x01t")])])))
    f1.append(mk("F type ref 7", update([block(5, 0, [ytype(7)])]), valid=False))
    f1.append(mk("F content json", update([block(5, 0, [item(2, b"\x01\x011")])])))
    f1.append(mk("F content embed", update([block(5, 0, [item(5, b"\x011")])])))
    f1.append(mk("F content format", update([block(5, 0, [item(6, b"\x01b\x04true")])])))
    f1.append(mk("F content any", update([block(5, 0, [item(8, b"\x02\x7d\x05\x78")])])))
    f1.append(mk("F content doc", update([block(5, 0, [item(9, b"\x01g\x76\x00")])])))
    # patterns at every stream residue: the document 64-aligned, a string in front moves the pattern
    f2, f3, f4 = [], [], []
    big = 0xF0000005
    for r in range(64):
        def at(prefix, second, client=5, r=r):
            """Two structs; the first one's string length puts byte `prefix` of the second at arena residue r."""
            hdr = 2 + len(vu(client)) + 1                       # blocks, structs, client, clock
            n = (r - prefix - hdr - 6) % 64 + 192               # 192 .. 255: two-byte varuints for n and n - 1
            return update([block(client, 0, [s(text(n)), second(n)])])
        f2.append(mk("F 81 00 at residue %d" % r, at(4, lambda n: item(4, b"\x81\x00a", origin=(5, n - 1)))))
        f3.append(mk("F C4 and a 5-byte client at residue %d" % r, at(0, lambda n: s("a", origin=(big, n - 1), right=(3, 0)), client=big)))
        f4.append(mk("F 6-byte varuint at residue %d" % r, at(4, lambda n: item(1, b"\x80\x80\x80\x80\x80\x01", origin=(5, n - 1)))))
    return [f1, aligned(f2, 64), aligned(f3, 64), aligned(f4, 64)]


def pattern_at(u, pat):
    """Offsets of `pat` in u."""
    out, i = [], u.find(pat)
    while i >= 0:
        out.append(i)
        i = u.find(pat, i + 1)
    return out


# ---------------------------------------------------------------- G: delete sets and truncation
def family_g():
    base = [block(9, 0, chain(9, 3)), block(5, 0, chain(5, 2))]
    g1 = []

    def add(name, ds, valid=True, sv=SV0):
        g1.append(mk("G " + name, update(base, ds), sv, valid))

    add("no clients", [])
    add("one client", [(9, [(1, 2)])])
    add("two clients descending", [(9, [(1, 2)]), (5, [(0, 1)])])
    add("two clients equal", [(9, [(1, 2)]), (9, [(4, 1)])])
    add("two clients ascending", [(5, [(0, 1)]), (9, [(1, 2)])])
    add("a client without ranges", [(9, []), (5, [(0, 1)])])
    add("60 ranges", [(9, [(3 * k, 2) for k in range(60)])])
    add("200 ranges", [(9, [(300 * k, 200) for k in range(200)])], sv=svec([(9, 6)]))
    add("5-byte clocks and lengths", [(9, [(0x10000000 + 0x11000000 * k, 0x10000001) for k in range(5)])])
    add("one trailing byte", encode_ds([(9, [(1, 2)])]) + b"\x07")
    g1.append(mk("G one trailing byte, cut", update(base, encode_ds([(9, [(1, 2)])]) + b"\x07"), svec([(9, 3)])))
    doc = update([block(0xF0000009, 0, [s(text(40)), dl(300, origin=(0xF0000009, 39)), gc(5), s(text(20, 4), origin=(0xF0000009, 344), right=(5, 1))]),
                  block(5, 2, chain(5, 3, first_clock=2))], [(0xF0000009, [(3, 4), (50, 200)]), (5, [(2, 1)])])
    assert 110 <= len(doc) <= 135, len(doc)
    g2 = [mk("G truncated at %d" % k, doc[:k], svec([(0xF0000009, 10 + k % 40), (5, k % 9)]), valid=False) for k in range(len(doc))]
    g2.append(mk("G whole", doc, svec([(0xF0000009, 17), (5, 3)])))
    return [g1, g2]


# ---------------------------------------------------------------- H: scheduling
H_COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)


def family_h():
    tiny = [mk("H fast", update([block(5, 1, chain(5, 3, first_clock=1))]), svec([(5, 3)])),
            mk("H cut", update([block(5, 0, [s(text(9)), dl(4, origin=(5, 8))])]), svec([(5, 4)])),
            mk("H two clients", update([block(9, 0, chain(9, 2)), block(5, 0, chain(5, 2))], [(9, [(0, 1)])]), svec([(9, 2)])),
            mk("H exact", update([block(5, 0, [s("hé")])])),
            mk("H string 70", update([block(5, 0, [s(text(70))])])),
            mk("H invalid", update([block(5, 0, [s(text(9))])])[:9], valid=False),
            mk("H 00 00", b"\x00\x00"),
            mk("H gc", update([block(5, 2, [gc(3), dl(2, origin=(5, 4))])]), svec([(5, 3)])),
            mk("H binary", update([block(5, 0, [binary(b"\x01\x02\x03")])]))]
    long = mk("H 5 000-byte document", update([block(5, 0, [s(text(5000)), dl(9, origin=(5, 4999))])]), svec([(5, 2500)]))
    same = [mk("H same size %d" % j, update([block(5, 1, [s(text(6, j), origin=(5, 0)), s(text(4, j), origin=(5, 6))])]), svec([(5, 2 + j % 9)]))
            for j in range(13)]
    assert len({len(x[1]) for x in same}) == 1
    mixed, ties = [], []
    for n in H_COUNTS:
        b = [tiny[k % 9] for k in range(n)]
        b[n // 2] = long
        mixed.append(b)
        ties.append([same[k % 13] for k in range(n)])
    return mixed + ties


# ---------------------------------------------------------------- I: shared states
I_ASKS = (0, 1, 2, 64, 65, 257)


def family_i():
    """-> (states, ask_state, items): one item per ask (its update the state's bytes)."""
    a, b, c = family_a(), family_b(), family_c()
    pool = [a[1][1], a[2][1], a[3][1], b[0][0], b[0][20], c[0][0], c[0][40], c[1][3], c[1][20], c[1][-1], a[8][1], b[2][0]]
    states, ask, items = [], [], []
    rng = random.Random(11)
    seventeen = svec([(100 + j, 1) for j in range(17)])
    for k, it in enumerate(pool):
        states.append(it[1])
        n = I_ASKS[k % len(I_ASKS)]
        top = max(len(it[1]), 2)
        cl = [5, 9, 7, 300, 0xF1234567, 3]
        for j in range(n):
            sv = seventeen if j % 23 == 5 else svec([(cl[(j + i) % 6], rng.randrange(top)) for i in range(j % 4)]) if j % 7 else it[2]
            ask.append(k)
            items.append(mk("I state %d (%s), ask %d" % (k, it[0], j), it[1], sv, it[5]))
    return states, ask, items


def families():
    return {"A": family_a(), "B": family_b(), "C": family_c(), "D": family_d(), "E": family_e(), "F": family_f(),
            "G": family_g(), "H": family_h()}


def flat(batches):
    return [it for b in batches for it in b]


_EXP = {}


def expected(it, mode, compat135=False):
    """yjs's answer for an item, (status, bytes | None), computed once per distinct (update, sv)."""
    import oracle
    key = (it[1], it[2] if mode == "diff" else None, compat135)
    if key not in _EXP:
        r = oracle.diff_update(it[1], it[2], compat135=compat135) if mode == "diff" else oracle.encode_state_vector_from_update(it[1], compat135=compat135)
        _EXP[key] = (r[0], r[1] if r[0] == 0 else None)
    return _EXP[key]

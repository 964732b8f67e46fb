"""Hand-built update-V1 documents for the snapshot cascade (snapshot_dev): k_snap_text with a 6 KiB workspace, then
with 24 KiB, then k_snap_count / scan / k_snap, then the pending merge.  Every document sits on a cap of the flat-text
tier, on an edge of its envelope, or on byte-level plumbing that exists only on the GPU (the dword shift of the input,
the staging copy, the scanned workspace offsets).

A `Doc` carries its name, its bytes, the tier that finishes it with the default workspaces -- 'first', 'second',
'general', 'pending' (k_snap leaves it to the three-way merge) or 'throws' (yjs throws reading it) -- and a one-line
reason.  The caps are restated here from the documented layout of the workspace (a client table of 16 records of 20
bytes and 16 order bytes, then 26 + 2 bytes a part), not read from the library.  The expectations are yjs's
(tests/golden/snapshot_tier_edges_v135.json.gz, written by tools/snap_fixture.py --tiers from `unique()`).

`unique()` lists every distinct document once; the families D, E and F are batches of names over it."""
import gzip
import json
import os
import random

from golden import ds_to_desc
from v1util import encode_ds, vu

TIERS = ("first", "second", "general", "pending", "throws")


def cap(lb):
    """Parts a workspace of lb bytes holds: (lb - (16 * sizeof(CT) + 16)) // (sizeof(P) + 2)."""
    return (lb - (16 * 20 + 16)) // 28


CAP_FIRST, CAP_SECOND, CAP_4K = cap(6144), cap(24576), cap(4096)


class Doc:
    """u: the update; tier: see TIERS; why: the reason; parts: the flat-text parts the document needs (family A)."""

    def __init__(self, name, u, tier, why, parts=None):
        assert tier in TIERS, tier
        self.name, self.u, self.tier, self.why, self.parts = name, bytes(u), tier, why, parts


def tier_at(d, first_cap, second_cap=CAP_SECOND):
    """The tier of a family-A document when the first launch holds first_cap parts."""
    return "first" if d.parts <= first_cap else "second" if d.parts <= second_cap else "general"


# ---------------------------------------------------------------- building blocks
ROOT = b"\x01\x01t"


def item(ref, content, origin=None, right=None, parent=ROOT, sub=None):
    """One struct: info byte, origin / right origin ids ((client, clock) or raw bytes), else the parent, content."""
    info = ref | (0x80 if origin else 0) | (0x40 if right else 0) | (0x20 if sub is not None else 0)
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
    """ContentString (clock length: UTF-16 units)."""
    raw = txt.encode() if isinstance(txt, str) else txt
    return item(4, vu(len(raw)) + raw, **kw)


def dl(n, **kw):
    """ContentDeleted of n clocks."""
    return item(1, vu(n), **kw)


def block(client, clock, structs, nst=None):
    cl = client if isinstance(client, bytes) else vu(client)
    ck = clock if isinstance(clock, bytes) else vu(clock)
    return vu(len(structs) if nst is None else nst) + cl + ck + b"".join(structs)


def update(blocks, ds=()):
    return vu(len(blocks)) + b"".join(blocks) + (ds if isinstance(ds, bytes) else encode_ds(list(ds)))


def filler(size):
    """A one-string document of exactly `size` bytes (11 .. 130): flat text, one part."""
    assert 11 <= size <= 130
    return update([block(5, 0, [s("f" * (size - 10))])])


def sized(n, general=False):
    """A document of exactly n bytes: one client, three long strings typed one after the other; general: the second
    string starts with a two-byte character, which the flat-text tier refuses."""
    a = n // 3
    for c in range(n - 2 * a, 0, -1):
        second = ("é" + "b" * (a - 2)) if general else "b" * a
        la, lb = a, len(second)
        u = update([block(5, 0, [s("a" * a), s(second, origin=(5, la - 1)), s("c" * c, origin=(5, la + lb - 1))])])
        if len(u) == n:
            return u
        if len(u) < n:
            break
    raise ValueError(n)


# ---------------------------------------------------------------- A: workspace caps
def chain(client, K, L=6):
    """K strings of L letters by one client, each typed after the one before: K parts."""
    out, ck = [], 0
    for i in range(K):
        txt = chr(97 + i % 26) * L
        out.append(s(txt, origin=(client, ck - 1)) if ck else s(txt))
        ck += L
    return out


def a_structs(parts):
    """Input structs alone: parse refuses the struct past the cap."""
    return update([block(7, 0, chain(7, parts))])


def a_ranges(parts):
    """Fewer structs than the cap; delete ranges inside a string (two splits) or over its second half (one) bring the
    parts to `parts`: split refuses after the document was integrated and earlier ranges were applied."""
    K = parts - parts // 3
    extra = parts - K
    mids, ends = extra // 2, extra % 2
    rs = [(6 * i + 1, 4) for i in range(mids)] + [(6 * (mids + i) + 3, 3) for i in range(ends)]
    return update([block(7, 0, chain(7, K))], [(7, rs)])


def a_origins(parts, hi):
    """A second client types one letter into the middle of each of the first m strings (origin (7, 6j + 2): one split
    each), every third without a right origin; integration refuses the split past the cap with earlier parts linked.
    hi: the second client's id is above / below the first one's (it is integrated first / last)."""
    m = parts // 4
    KA = parts - 2 * m
    other = 9 if hi else 3
    b = [s("X", origin=(7, 6 * j + 2), right=None if j % 3 == 2 else (7, 6 * j + 3)) for j in range(m)]
    blocks = [block(other, 0, b), block(7, 0, chain(7, KA))]
    return update(blocks if hi else blocks[::-1])


def family_a():
    docs = []
    for c in (CAP_4K, CAP_FIRST, CAP_SECOND):
        for parts in range(c - 2, c + 3):
            tier = "first" if parts <= CAP_FIRST else "second" if parts <= CAP_SECOND else "general"
            for kind, u in (("structs", a_structs(parts)), ("ranges", a_ranges(parts)), ("origins", a_origins(parts, parts % 2 == 0))):
                docs.append(Doc("A cap %d %s parts %d" % (c, kind, parts), u, tier, "%d parts against the caps %d / %d" %
                                (parts, CAP_FIRST, CAP_SECOND), parts=parts))
    return docs


# ---------------------------------------------------------------- B: envelope edges
GAP = bytes([1, 1, 5, 3, 0x04, 1, 1, 0x74, 1, 0x61, 0])      # client 5 starts at clock 3
ORPHAN = bytes([1, 1, 5, 0, 0x84, 9, 0, 1, 0x61, 0])          # origin (9, 0) is not in the update
SMALL = update([block(9, 0, [s("ab")]), block(5, 0, [s("c", origin=(9, 0), right=(9, 1))])], [(9, [(1, 1)])])


def family_b():
    D = []

    def add(name, u, tier, why):
        D.append(Doc("B " + name, u, tier, why))

    for nc in (15, 16, 17):
        ids = sorted((1000 + 37 * i for i in range(nc)), reverse=True)
        add("%d client blocks" % nc, update([block(c, 0, [s("xy")]) for c in ids]), "first" if nc <= 16 else "general",
            "the client table holds 16 blocks")
    add("a client block twice", update([block(7, 0, [s("ab")]), block(7, 2, [s("cd", origin=(7, 1))])]), "general",
        "a repeated client: outside the engine's envelope (yjs keeps the later block alone)")
    for tail in (5, 6):
        add("clock end %d" % (65530 + tail), update([block(9, 0, [dl(65530), s("q" * tail, origin=(9, 65529))])]),
            "first" if tail == 5 else "general", "clock + len <= 65535 in the 16-bit part records")
    head = block(9, 0, [dl(65530), s("abcde", origin=(9, 65529))])
    for ck in (65534, 65535, 65536):
        add("origin clock %d" % ck, update([block(12, 0, [s("z", origin=(9, ck))]), head]), "first" if ck == 65534 else "pending",
            "an origin past the client's state 65535 stays pending; 65536 does not fit the record")
        add("right origin clock %d" % ck, update([block(12, 0, [s("z", right=(9, ck))]), head]), "first" if ck == 65534 else "pending",
            "a right origin past the client's state 65535 stays pending; 65536 does not fit the record")
    for n in (65534, 65535, 65536):
        add("%d bytes" % n, sized(n), "first" if n == 65534 else "general", "inputs below 65535 bytes")
    # a two-byte character: first, last, and with its first byte at each residue of the document's bytes mod 4
    add("non-ASCII first", update([block(5, 0, [s("ébcdefgh")])]), "general", "ASCII strings only")
    add("non-ASCII last", update([block(5, 0, [s("abcdefgé")])]), "general", "ASCII strings only")
    for r in range(4):
        u = next(u for u in (update([block(5, 0, [s("a" * k + "é" + "z" * (11 - k))])]) for k in range(1, 9)) if u.index(b"\xc3") % 4 == r)
        add("non-ASCII at residue %d" % r, u, "general", "ASCII strings only, a dword at a time")
        name = ("n" * (r + 1) + "é").encode()
        u = update([block(5, 0, [s("abc", parent=b"\x01" + vu(len(name)) + name)])])
        add("non-ASCII root name, %d letters before" % (r + 1), u, "general", "an ASCII root name")
    add("two root names of equal length", update([block(5, 0, [s("ab", parent=b"\x01\x02t1"), s("cd", parent=b"\x01\x02t2")])]),
        "general", "one root type")
    add("two root names of unequal length", update([block(5, 0, [s("ab", parent=b"\x01\x02t1"), s("cd", parent=b"\x01\x03t12")])]),
        "general", "one root type")
    add("the same root name twice", update([block(5, 0, [s("ab", parent=b"\x01\x02t1"), s("cd", parent=b"\x01\x02t1")])]),
        "first", "one root type, named by both structs")
    add("parentSub", update([block(5, 0, [s("v", sub=b"key")])]), "general", "no map entries")
    add("parent by id", update([block(5, 0, [item(7, vu(0)), s("q", parent=b"\x00" + vu(5) + vu(0))])]), "general", "no nested types")
    for name, st in (("GC", b"\x00\x02"), ("ContentType", item(7, vu(0))), ("ContentEmbed", item(5, vu(7) + b'{"k":1}')),
                     ("ContentBinary", item(3, vu(3) + b"\x01\x02\xff")), ("ContentJSON", item(2, vu(1) + vu(1) + b"2")),
                     ("ContentFormat", item(6, vu(4) + b"bold" + vu(4) + b"true")), ("ContentAny", item(8, vu(1) + b"\x7d\x05"))):
        add("one " + name, update([block(5, 0, [s("ab"), st])]), "general", "ContentString and ContentDeleted only")
    add("one Skip", update([block(5, 0, [s("ab"), b"\x0a\x03", s("c", origin=(5, 1))])]), "pending",
        "a Skip: the structs after it wait for the gap")
    add("client id 2^32 - 1", update([block(2 ** 32 - 1, 0, [s("ab")]), block(2 ** 28, 0, [s("c", origin=(2 ** 32 - 1, 0))])],
                                     [(2 ** 32 - 1, [(1, 1)])]), "first", "five-byte client ids below 2^32")
    add("client id 2^32", update([block(2 ** 32, 0, [s("ab")])]), "general", "client ids below 2^32: outside the engine's envelope")
    add("origin client id 2^32 + 5", update([block(2 ** 32 + 5, 0, [s("ab")]), block(7, 0, [s("c", origin=(2 ** 32 + 5, 0))])]), "general",
        "client ids below 2^32: outside the engine's envelope")
    nm5 = b"\x85\x80\x80\x80\x00"       # 5 in five bytes
    nm6 = b"\x85\x80\x80\x80\x80\x00"   # 5 in six bytes
    add("non-minimal client id", update([block(nm5, 0, [s("ab")])]), "first", "varuints of up to five bytes, whatever their value")
    add("non-minimal client id, six bytes", update([block(nm6, 0, [s("ab")])]), "general", "varuints of up to five bytes")
    add("non-minimal origin", update([block(5, 0, [s("ab"), s("c", origin=nm5 + b"\x81\x00")])]), "first", "varuints of up to five bytes")
    add("non-minimal length", update([block(5, 0, [item(4, b"\x82\x80\x00ab")])]), "first", "varuints of up to five bytes")
    add("non-minimal length, six bytes", update([block(5, 0, [item(4, b"\x82\x80\x80\x80\x80\x00ab")])]), "general",
        "varuints of up to five bytes")
    add("non-minimal delete set", update([block(5, 0, [s("abcd")])], b"\x81\x00" + nm5 + b"\x81\x00" + b"\x81\x80\x00" + b"\x82\x00"), "first",
        "varuints of up to five bytes")
    add("non-minimal delete set, six bytes", update([block(5, 0, [s("abcd")])], b"\x01" + nm6 + b"\x01\x01\x02"), "general",
        "varuints of up to five bytes")
    add("zero-length string", update([block(5, 0, [s("ab"), s("", origin=(5, 1))])]), "general", "parts of at least one clock")
    add("origin on an absent client", ORPHAN, "pending", "the struct waits for client 9")
    add("first clock 3", GAP, "pending", "the struct waits for clocks 0 .. 2")
    add("delete range past the state", update([block(5, 0, [s("abc")])], [(5, [(1, 5)])]), "pending", "the range's rest waits")
    add("delete range up to the state", update([block(5, 0, [s("abc")])], [(5, [(1, 2)])]), "first", "the range ends at the state")
    add("delete set of an absent client", update([block(5, 0, [s("abc")])], [(9, [(0, 1)])]), "pending", "the range waits for client 9")
    add("delete range ending at 2^32 - 1", update([block(5, 0, [s("abc")])], [(5, [(1, 2 ** 32 - 2)])]), "pending", "the range's rest waits")
    add("delete range ending at 2^32", update([block(5, 0, [s("abc")])], [(5, [(1, 2 ** 32 - 1)])]), "general",
        "clock + len past 2^32 - 1: outside the engine's envelope")
    for k in range(len(SMALL)):
        add("truncated to %d of %d bytes" % (k, len(SMALL)), SMALL[:k], "throws", "yjs reads past the end")
    add("whole", SMALL, "first", "the document the truncations cut")
    add("trailing bytes", SMALL + b"\x07\xff\x00", "first", "bytes after the delete set are not read")
    return D


# Documents the general kernel refuses by contract (include/ygm.h: YGM_EUNSUPPORTED, the caller keeps its yjs path for
# them): the fixture records what yjs does, the engine's answer is the status alone.
UNSUPPORTED = {"B a client block twice", "B client id 2^32", "B origin client id 2^32 + 5", "B delete range ending at 2^32"}


# ---------------------------------------------------------------- C: integration shapes inside the envelope
C_SEEDS = range(150)
C_DROPPED = ()      # seeds on which the general kernel's code (tools/snapdev) and yjs 13.5.16 differ: none
ID_POOL = [1, 5, 77, 127, 128, 999, 12345, 65536, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 31 + 5, 3000000001, 4000000000,
           2 ** 32 - 1, 300, 4242, 70000, 2 ** 24]


def session(seed):
    """Two writers type a base text in turn (strings and deleted runs, each after the one before); then every client
    inserts one to three runs into that base without seeing the others -- most of them at the same position -- with
    the neighbours' ids as origin and right origin; then delete ranges over whole structs, touching and overlapping
    ones, and ones that cut a struct's first or last character.  Blocks ascending, descending or shuffled by id."""
    rng = random.Random(1000 + seed)
    nc = (2, 3, 4, 5, 8, 12, 16)[seed % 7] if seed % 5 else rng.randint(2, 16)
    ids = rng.sample(ID_POOL, nc)
    structs = {c: [] for c in ids}
    spans = {c: [] for c in ids}      # (clock, len, deleted) per struct
    clock = {c: 0 for c in ids}
    seq = []

    def put(c, L, deleted, origin, right):
        body = dl(L, origin=origin, right=right) if deleted else s("".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(L)),
                                                                     origin=origin, right=right)
        structs[c].append(body)
        spans[c].append((clock[c], L, deleted))
        ids_ = [(c, clock[c] + k) for k in range(L)]
        clock[c] += L
        return ids_

    for i in range(rng.randint(2, 8)):
        c = ids[i % 2]
        seq += put(c, rng.randint(1, 6), bool(seq) and rng.random() < 0.2, seq[-1] if seq else None, None)
    hot = rng.randrange(len(seq) + 1)
    for c in ids:
        for _ in range(rng.randint(1, 3)):
            if sum(len(v) for v in structs.values()) >= 48:      # (3 parts a struct at the most, and 25 ranges below)
                break
            pos = hot if rng.random() < 0.6 else rng.randrange(len(seq) + 1)
            origin = seq[pos - 1] if pos else None
            right = seq[pos] if pos < len(seq) and rng.random() < 0.8 else None
            if origin is None and right is None and pos < len(seq):
                right = seq[pos]
            mine = put(c, rng.randint(1, 4), rng.random() < 0.1 and (origin or right) is not None, origin, right)
            if rng.random() < 0.4:      # and goes on typing after its own run
                put(c, rng.randint(1, 3), False, mine[-1], right)
    ds = []
    for c in ids:
        rs = []
        for ck, L, deleted in spans[c]:
            kind = rng.randrange(8) if sum(len(r) for _, r in ds) + len(rs) < 23 else 7
            if kind == 0:
                rs.append((ck, L))                            # the whole struct
            elif kind == 1:
                rs.append((ck, 1))                            # its first character
            elif kind == 2:
                rs.append((ck + L - 1, 1))                    # its last character
            elif kind == 3 and L >= 2:
                rs += [(ck, 1), (ck + 1, L - 1)]              # two touching ranges
            elif kind == 4 and L >= 3:
                rs += [(ck, 2), (ck + 1, L - 1)]              # two overlapping ranges
            elif kind == 5 and ck + L < clock[c]:
                rs.append((ck + L - 1, 2))                    # across the boundary to the next struct
        if rs:
            ds.append((c, rs))
    order = seed % 3
    by = sorted(ids) if order == 0 else sorted(ids, reverse=True) if order == 1 else rng.sample(ids, nc)
    if order == 2:
        rng.shuffle(ds)
    nstructs = sum(len(v) for v in structs.values())
    nranges = sum(len(rs) for _, rs in ds)
    assert 3 * nstructs + 2 * nranges <= 200, (seed, nstructs, nranges)      # parts: a struct, two origin splits, two range splits
    return update([block(c, 0, structs[c]) for c in by], ds), nc, ("ascending", "descending", "shuffled")[order]


def family_c():
    docs = []
    for seed in C_SEEDS:
        if seed in C_DROPPED:
            continue
        u, nc, order = session(seed)
        docs.append(Doc("C seed %d, %d clients %s" % (seed, nc, order), u, "first", "flat text of at most 200 parts"))
    return docs


# ---------------------------------------------------------------- F: many small documents
def family_f_docs():
    return [
        Doc("F empty", b"", "throws", "an empty update: yjs throws reading it"),
        Doc("F gap", GAP, "pending", "the 11-byte document whose only struct waits"),
        Doc("F one letter", filler(11), "first", "flat text"),
        Doc("F two clients", update([block(9, 0, [s("ab")]), block(5, 0, [s("cd")])]), "first", "flat text"),
        Doc("F deleted middle", update([block(5, 0, [s("abcd")])], [(5, [(1, 2)])]), "first", "flat text"),
        Doc("F two-byte letter", update([block(5, 0, [s("é")])]), "general", "ASCII strings only"),
        Doc("F deleted run", update([block(5, 0, [dl(3)])]), "first", "flat text"),
    ]


# ---------------------------------------------------------------- the corpus
FILLERS = range(11, 43)
E_RESIDUES = (0, 1, 8, 15)
E_TARGETS = (40960 - 16, 40960 - 1, 40960, 40960 + 1, 40960 + 16)     # b - a16 against k_snap's staging limit
E_MID = 2560
_CORPUS = None


def _e_last(r, t):
    return t - r - 15 * E_MID


def _corpus():
    global _CORPUS
    if _CORPUS is None:
        fam = {"A": family_a(), "B": family_b(), "C": family_c(), "F": family_f_docs()}
        fam["filler"] = [Doc("filler %d" % n, filler(n), "first", "flat text, one part") for n in FILLERS]
        e = [Doc("E %d bytes" % E_MID, sized(E_MID), "first", "three long strings"),
             Doc("E %d bytes, two-byte letter" % E_MID, sized(E_MID, True), "general", "ASCII strings only"),
             Doc("E 41000 bytes", sized(41000), "first", "three long strings; alone past the staging limit")]
        for n in sorted({_e_last(r, t) for r in E_RESIDUES for t in E_TARGETS} - {E_MID}):
            e.append(Doc("E %d bytes" % n, sized(n), "first", "three long strings"))
        fam["E"] = e
        by_name = {}
        for docs in fam.values():
            for d in docs:
                assert d.name not in by_name, d.name
                by_name[d.name] = d
        _CORPUS = fam, by_name
    return _CORPUS


def families():
    """{'A' | 'B' | 'C' | 'E' | 'F' | 'filler': [Doc]} -- every distinct document."""
    return _corpus()[0]


def unique():
    """Every distinct document, in a fixed order (the fixture's rows)."""
    return [d for docs in _corpus()[0].values() for d in docs]


def get(name):
    return _corpus()[1][name]


def census(docs=None):
    """{tier: documents} of docs (default: every distinct document)."""
    out = dict.fromkeys(TIERS, 0)
    for d in unique() if docs is None else docs:
        out[d.tier] += 1
    return out


# ---------------------------------------------------------------- D: residues
D_NAMES = ["A cap 207 ranges parts 207", "A cap 134 origins parts 136", None, "B 16 client blocks",      # (None: the first of family C)
           "A cap 207 structs parts 208", "A cap 207 origins parts 209", "A cap 865 ranges parts 865", "A cap 865 structs parts 864",
           "A cap 865 ranges parts 866", "B 17 client blocks", "B one GC", "B non-ASCII last",
           "B truncated to %d of %d bytes" % (len(SMALL) - 1, len(SMALL))]      # and a thirteenth: cut inside its last varuint


def d_names():
    return [n or families()["C"][0].name for n in D_NAMES]


def _fill_to(at, r):
    """A filler that ends at residue r mod 16 when it starts at `at`."""
    size = 11 + (r - at - 11) % 16
    assert (at + size) % 16 == r
    return get("filler %d" % size)


def family_d():
    """One batch: each of the thirteen documents behind a filler, starting at every residue 0 .. 15 of the arena."""
    docs, at = [], 0
    for name in d_names():
        for r in range(16):
            f = _fill_to(at, r)
            docs += [f, get(name)]
            at += len(f.u) + len(get(name).u)
    return docs


def family_d_last():
    """Thirteen batches: three fillers, then the document as the last one of the arena (at residues that differ)."""
    out = []
    for k, name in enumerate(d_names()):
        fs = [get("filler %d" % (11 + (k + j) % 16)) for j in range(3)]
        out.append(fs + [get(name)])
    return out


def start_residues(docs):
    """{name: set of arena offsets mod 16} over a batch packed in order."""
    at, out = 0, {}
    for d in docs:
        out.setdefault(d.name, set()).add(at % 16)
        at += len(d.u)
    return out


# ---------------------------------------------------------------- E: staging
def family_e():
    """[(r, target, [32 Docs])]: the first 16 documents end at residue r mod 16 (a & 15 of the second group), the second
    16 hold target - r bytes, so that b - a16 is the target; documents at odd places of the second group are general.
    Then one batch whose first group holds a single 41000-byte document among fillers."""
    out = []
    for r in E_RESIDUES:
        for t in E_TARGETS:
            g1 = [get("filler 16")] * 15 + [get("filler %d" % (16 + r))]
            g2 = [get("E %d bytes, two-byte letter" % E_MID) if j % 2 else get("E %d bytes" % E_MID) for j in range(15)]
            g2.append(get("E %d bytes" % _e_last(r, t)))
            assert sum(len(d.u) for d in g1) % 16 == r and r + sum(len(d.u) for d in g2) == t
            out.append((r, t, g1 + g2))
    big = [get("filler %d" % (11 + j)) for j in range(16)]
    big[7] = get("E 41000 bytes")
    out.append((None, None, big + [get("filler %d" % (20 + j)) for j in range(16)]))
    return out


# ---------------------------------------------------------------- F: cycled
def family_f(n, shift=0):
    """n documents: the seven tiny ones in turn."""
    f = families()["F"]
    return [f[(k + shift) % len(f)] for k in range(n)]


# ---------------------------------------------------------------- the yjs fixture of the corpus
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snapshot_tier_edges_v135.json.gz")
_ROWS = None


def rows():
    """{name: (update, (yjs status, bytes), (status, bytes under gc: false))}, read once."""
    global _ROWS
    if _ROWS is None:
        d = json.load(gzip.open(FIX, "rt"))
        _ROWS = {n: (bytes.fromhex(u), (st, bytes.fromhex(e)), (st, bytes.fromhex(x) if x is not None else b"")) for n, u, st, e, x in d["rows"]}
        assert len(_ROWS) == len(d["rows"])
    return _ROWS


def expected(d, compat135=True, nogc=False):
    """What the engine answers: yjs's bytes (the delete set client-descending in the default mode), or the status of a
    documented refusal."""
    if d.name in UNSUPPORTED:
        return (9, b"")
    st, e = rows()[d.name][2 if nogc else 1]
    return (st, e) if compat135 or st else (st, bytes.fromhex(ds_to_desc(e.hex())))

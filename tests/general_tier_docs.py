"""Hand-built update-V1 documents for the two general merge tiers between the lean kernels and the large-document
tier: k_merge_wave (one wave per document) and k_merge_fast (one workgroup per document).  Every document sits on a
cap, a sort width, a lane-block edge of a scan or a rule of R-M that only these two tiers
implement -- provenance-dependent GC coalescing, Skip gaps, multi-block updates, re-encoded structs, up to 64 clients.

Every document is built so that the lean kernels refuse it; the reason stands next to its family.  `census` counts
what the caps count, `expected_tier` restates the caps.  The corpus is plain data: `families()` returns
{name: [batch, ...]}, a batch being a list of `Doc`s that go to the device together."""
import random

from lean_docs import item, text, upd
from v1util import _skip_struct, encode_ds, rd_vu, read_ds, vu


class Doc:
    """us: the updates; tier: 'wave' / 'workgroup' / 'large', or None where the family asserts parity only;
    valid: the oracle must return status 0; want: census values the builder intends (checked by the CPU test)."""

    def __init__(self, name, us, tier, valid=True, **want):
        self.name, self.us, self.tier, self.valid, self.want = name, list(us), tier, valid, want


# ---------------------------------------------------------------- building blocks
def gc(n=1):
    return b"\x00" + vu(n)


def skip(n):
    return b"\x0a" + vu(n)


def ch(c="a"):
    """One character under the parent key 't': 6 bytes, clock length 1."""
    return item(4, text(c))


def block(client, clock, structs):
    cl = client if isinstance(client, bytes) else vu(client)
    return vu(len(structs)) + cl + vu(clock) + b"".join(structs)


def update(blocks, ds=b"\x00"):
    return vu(len(blocks)) + b"".join(blocks) + ds


EMPTY = b"\x00\x00"


def str_update(client, clock, size):
    """A one-struct update (a string under 't') of exactly `size` bytes; returns it and its clock length."""
    for n in range(max(size - 16, 1), size):
        u = upd(client, clock, [item(4, text("x" * n))])
        if len(u) == size:
            return u, n
    raise ValueError(size)


def padded(nbytes, head, client=9, clock=0, piece=1000):
    """`head` (updates) followed by string updates of at most `piece` bytes up to exactly `nbytes`."""
    us = list(head)
    left = nbytes - sum(len(u) for u in us)
    while left:
        n = left if left <= piece else piece if left - piece >= 32 else left - 32
        u, ln = str_update(client, clock, n)
        us.append(u)
        clock += ln
        left -= n
    assert sum(len(u) for u in us) == nbytes
    return us


# ---------------------------------------------------------------- census and tier prediction
def struct_len(b, p):
    """Clock length of the struct at p."""
    info = b[p]
    ref = info & 31
    q = p + 1
    if info == 10 or ref == 0:
        return rd_vu(b, q)[0]
    if info & 0x80:
        q = rd_vu(b, rd_vu(b, q)[1])[1]
    if info & 0x40:
        q = rd_vu(b, rd_vu(b, q)[1])[1]
    if (info & 0xC0) == 0:
        pi, q = rd_vu(b, q)
        if pi == 1:
            n, q = rd_vu(b, q)
            q += n
        else:
            q = rd_vu(b, rd_vu(b, q)[1])[1]
        if info & 0x20:
            n, q = rd_vu(b, q)
            q += n
    if ref in (1, 2, 8):
        return rd_vu(b, q)[0]
    if ref == 4:
        n, q = rd_vu(b, q)
        return len(bytes(b[q:q + n]).decode("utf-8").encode("utf-16-le")) // 2
    return 1


def walk(u):
    """[(client, clock, kind, length)] of every struct of update u in input order (kind 'skip' / 'gc' / 'item'),
    and its delete set [(client, [(clock, len)])]."""
    out = []
    nb, p = rd_vu(u, 0)
    for _ in range(nb):
        ns, p = rd_vu(u, p)
        client, p = rd_vu(u, p)
        clock, p = rd_vu(u, p)
        for _ in range(ns):
            ln = struct_len(u, p)
            kind = "skip" if u[p] == 10 else "gc" if (u[p] & 31) == 0 else "item"
            out.append((client, clock, kind, ln))
            clock += ln
            p = _skip_struct(u, p)
    ds, p = read_ds(u, p)
    assert p == len(u), (p, len(u))
    return out, ds


def census(us):
    """What the tier caps count, of a document whose updates all parse."""
    S = D = 0
    scl, dcl = set(), set()
    defer = False       # the deferral conditions the wave and workgroup kernels share
    for u in us:
        structs, ds = walk(u)
        prev = None
        for client, clock, kind, ln in structs:
            if client >= 2 ** 32:
                defer = True
            if kind == "skip":
                continue
            S += 1
            scl.add(client)
            if ln == 0 or clock + ln >= 2 ** 32:
                defer = True
            if prev and (client > prev[0] or (client == prev[0] and clock < prev[1])):
                defer = True
            prev = (client, clock + ln)
        for client, rs in ds:
            for ck, ln in rs:
                D += 1
                dcl.add(client)
                if client >= 2 ** 32 or ck + ln >= 2 ** 32:
                    defer = True
    return dict(k=len(us), nbytes=sum(len(u) for u in us), largest=max([len(u) for u in us] or [0]), S=S, D=D,
                struct_clients=len(scl), ds_clients=len(dcl), defer=defer)


def expected_tier(us):
    """The tier that finishes an overlap-free, valid document of two or more updates.  The caps restate
    ygm_kernels.hip (BIG_ROUTE_MIN 1024; M_KCAP 256, M_INCAP 16384, M_SCAP 512, M_DCAP 256) and ygm_merge_wave.hpp
    (W_K 256, W_IN 8192 -- the kernel tests nbytes + 16 > W_IN --, W_S 256, W_D 128, W_C 64, W_BLK 64)."""
    c = census(us)
    if c["largest"] >= 1024:
        return "large"
    if (c["k"] <= 256 and c["nbytes"] <= 8176 and c["S"] <= 256 and c["D"] <= 128 and c["struct_clients"] <= 64 and
            c["ds_clients"] <= 64 and not c["defer"]):
        return "wave"
    if c["k"] <= 256 and c["nbytes"] <= 16384 and c["S"] <= 512 and c["D"] <= 256 and not c["defer"]:
        return "workgroup"
    return "large"


def routed_by_size(us):
    return len(us) >= 2 and max(len(u) for u in us) >= 1024


# ---------------------------------------------------------------- client id sets
def client_ids(n, kind, seed=0):
    """n distinct client ids: 'one' one-byte varuints (client 0 among them), 'five' five-byte (the largest 32-bit id
    among them), 'mixed' every varuint length."""
    rng = random.Random(seed)
    one = [0] + rng.sample(range(1, 128), min(n, 127) - 1) if n > 1 else [5]
    five = [2 ** 32 - 1] + rng.sample(range(2 ** 28, 2 ** 32 - 1), n - 1)
    if kind == "one":
        ids = one
    elif kind == "five":
        ids = five
    else:
        pool = [2 ** 32 - 1, 0, 127, 128, 2 ** 14 - 1, 2 ** 14, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28]
        pool += rng.sample(range(1, 127), 20) + rng.sample(range(129, 2 ** 14 - 1), 20) + rng.sample(range(2 ** 21 + 1, 2 ** 28 - 1), 30)
        ids = pool[:n]
    ids = ids[:n]
    assert len(set(ids)) == n, (n, kind)
    rng.shuffle(ids)
    return ids


# ---------------------------------------------------------------- A: sort widths and client counts
# Lean refusal: every 11th struct (the first one included) is a GC.
A_SHAPES = [  # (S, struct clients, tier)
    (1, 1, "wave"), (2, 1, "wave"), (63, 8, "wave"), (64, 9, "wave"), (65, 63, "wave"), (65, 65, "workgroup"),
    (127, 64, "wave"), (128, 8, "wave"), (128, 65, "workgroup"), (129, 9, "wave"), (191, 1, "wave"), (192, 63, "wave"),
    (193, 64, "wave"), (255, 8, "wave"), (256, 64, "wave"), (256, 1, "wave"),
    (257, 8, "workgroup"), (258, 9, "workgroup"), (511, 64, "workgroup"), (512, 63, "workgroup"), (512, 65, "workgroup"),
    (513, 8, "large"),
]


def plain_updates(S, clients, per=1, first_clock=0, gc_every=11):
    """S structs in log order: update i belongs to client i mod n and holds `per` structs at that client's next
    clocks (the last update may hold fewer)."""
    clock = {c: first_clock for c in clients}
    us, j, i = [], 0, 0
    while j < S:
        c = clients[i % len(clients)]
        n = min(per, S - j)
        structs = [gc(1 + j % 3) if (j + q) % gc_every == 0 else ch("abcdefg"[(j + q) % 7]) for q in range(n)]
        lens = [1 + j % 3 if (j + q) % gc_every == 0 else 1 for q in range(n)]
        us.append(upd(c, clock[c], structs))
        clock[c] += sum(lens)
        j += n
        i += 1
    return us


def family_a():
    docs = []
    for n, (S, ncl, tier) in enumerate(A_SHAPES):
        ids = client_ids(ncl, ("one", "five", "mixed")[n % 3], seed=n)
        base = plain_updates(S, ids, per=(S + 199) // 200)
        if len(base) < 2:
            base.append(EMPTY)
        for order in ("log", "reversed", "shuffled"):
            us = list(base)
            if order == "reversed":
                us.reverse()
            elif order == "shuffled":
                random.Random(S * 7 + ncl).shuffle(us)
            docs.append(Doc("A S=%d clients=%d %s" % (S, ncl, order), us, tier, S=S, struct_clients=ncl, D=0))
    return [docs]


# ---------------------------------------------------------------- B: update counts
# Lean refusal: the first struct of every document is a GC.
B_K = [(2, "wave"), (63, "wave"), (64, "wave"), (65, "wave"), (255, "wave"), (256, "wave"), (257, "large")]


def k_updates(k, clients=(77, 3000000001)):
    return plain_updates(k, list(clients), gc_every=50)


def family_b_valid():
    return [[Doc("B k=%d" % k, k_updates(k), tier, k=k, S=k) for k, tier in B_K]]


def _truncated(u):
    return u[:-3]            # ends inside the string content


def _past_2_53(u):
    # the same update with its clock written as 2^53 + 1 (eight varuint bytes): past MAX_SAFE_INTEGER
    nb, p = rd_vu(u, 0)
    ns, p = rd_vu(u, p)
    cl, p1 = rd_vu(u, p)
    ck, p2 = rd_vu(u, p1)
    return u[:p1] + vu(2 ** 53 + 1) + u[p2:]


def family_b_invalid():
    docs = []
    for at in (0, 63, 64, 255):
        for name, brk in (("truncated", _truncated), ("past 2^53", _past_2_53)):
            us = k_updates(256)
            if at % 50 == 0:      # (a GC there: break its neighbour's string instead)
                us[at + 1], us[at] = us[at], us[at + 1]
            us[at] = brk(us[at])
            docs.append(Doc("B invalid %s at %d" % (name, at), us, None, valid=False))
    for a, b, fa, fb in ((1, 66, _truncated, _past_2_53), (63, 64, _past_2_53, _truncated), (64, 255, _truncated, _truncated),
                         (2, 130, _past_2_53, _truncated)):
        us = k_updates(256)
        us[a], us[b] = fa(us[a]), fb(us[b])
        docs.append(Doc("B invalid at %d and %d" % (a, b), us, None, valid=False))
    return [docs]


# ---------------------------------------------------------------- C: bytes and routing
# Lean refusal: a GC first, and updates over 64 bytes.
C_BYTES = [(8175, "wave"), (8176, "wave"), (8177, "workgroup"), (16383, "workgroup"), (16384, "workgroup"), (16385, "large")]
C_HEAD = [upd(9, 0, [gc(2)])]


def sized_doc(nbytes):
    return padded(nbytes, C_HEAD, client=9, clock=2)


def family_c():
    docs = [Doc("C nbytes=%d" % n, sized_doc(n), tier, nbytes=n) for n, tier in C_BYTES]
    for size, tier in ((1023, "wave"), (1024, "large")):
        u, _ = str_update(9, 2, size)
        docs.append(Doc("C largest=%d" % size, C_HEAD + [u], tier, largest=size))
    return [docs, residue_batch()]


def residue_batch():
    """The 8176- and the 8177-byte document at every arena residue b0 mod 16: a single-update filler document of
    0-15 bytes in front of each (a single update is returned as it is)."""
    docs, at = [], 0
    for r in range(16):
        for n, tier in ((8176, "wave"), (8177, "workgroup")):
            f = (r - at) % 16
            docs.append(Doc("C filler %d" % f, [bytes([1] * f)], None, valid=True, nbytes=f))
            at += f
            assert at % 16 == r
            docs.append(Doc("C nbytes=%d residue %d" % (n, r), sized_doc(n), tier, nbytes=n))
            at += n
    return docs


def residues(batch):
    """{nbytes: set of b0 mod 16} of the batch's documents of two or more updates, packed in order."""
    at, out = 0, {}
    for d in batch:
        n = sum(len(u) for u in d.us)
        if len(d.us) >= 2:
            out.setdefault(n, set()).add(at % 16)
        at += n
    return out


# ---------------------------------------------------------------- D: GC coalescing (R-M step 3)
# Lean refusal: GC structs.
def chars(client, clock, n, per=100):
    """n characters of one client from `clock`, in updates of at most `per`."""
    us = []
    while n:
        m = min(n, per)
        us.append(upd(client, clock, [ch("abcdefg"[(clock + q) % 7]) for q in range(m)]))
        clock += m
        n -= m
    return us


def gc_run(client, clock, n, pattern):
    """n contiguous GCs from `clock`; bit b of `pattern`: the boundary after GC b is another update."""
    us, cur, start = [], [], clock
    for g in range(n):
        ln = 1 + (g + n) % 3
        cur.append(gc(ln))
        clock += ln
        if g == n - 1 or (pattern >> g) & 1:
            us.append(upd(client, start, cur))
            cur, start = [], clock
    return us, clock


def run_doc(name, before, n, pattern, after=3, client=40, reverse=False):
    """`before` characters, a run of n GCs (sorted positions before .. before + n - 1), `after` characters."""
    us = chars(client, 0, before)
    run, clock = gc_run(client, before, n, pattern)
    us += run + chars(client, clock, after)
    if len(us) < 2:
        us.append(EMPTY)
    if reverse:
        us.reverse()
    S = before + n + after
    return Doc(name, us, "wave" if S <= 256 else "workgroup", S=S, struct_clients=1)


def family_d():
    docs = []
    for n in range(2, 7):
        for pat in range(1 << (n - 1)):
            # the run covers sorted positions 2 .. n + 1 (n >= 3: across 3 | 4, the four-element lane block)
            docs.append(run_doc("D run %d pattern %d" % (n, pat), 2, n, pat))
            if n == 6:
                docs.append(run_doc("D run 6 pattern %d reversed" % pat, 2, n, pat, reverse=True))
    for n in range(2, 7):
        for l in (1, 16, 32, 63):       # the run's second GC is the first element of lane l's block
            docs.append(run_doc("D run %d at %d|%d" % (n, 4 * l - 1, 4 * l), 4 * l - 1, n, 0b10101 & ((1 << (n - 1)) - 1)))
            if 4 * l >= n:
                docs.append(run_doc("D run %d ends at %d" % (n, 4 * l - 1), 4 * l - n, n, 0b01010 & ((1 << (n - 1)) - 1)))
        docs.append(run_doc("D run %d at 255|256" % n, 255, n, 0b01101 & ((1 << (n - 1)) - 1)))      # S > 256: workgroup
        docs.append(run_doc("D run %d ends at 255" % n, 256 - n, n, 0b10010 & ((1 << (n - 1)) - 1), after=0))
    for p in (1, 3, 4, 5, 63, 64, 127, 128, 200, 255):
        us = [upd(40, 0, [gc()] * p), upd(40, p, [gc()] * (256 - p))]
        docs.append(Doc("D 256 GCs, source change at %d" % p, us, "wave", S=256, k=2))
        docs.append(Doc("D 256 GCs, source change at %d, reversed" % p, us[::-1], "wave", S=256, k=2))
    c = 40
    docs += [
        Doc("D run broken by an Item", [upd(c, 0, [gc(2), gc(1)]), upd(c, 3, [ch()]), upd(c, 4, [gc(1), gc(3)])], "wave", S=5),
        Doc("D run broken by an Item of the same update", [upd(c, 0, [gc(2), ch(), gc(1)]), upd(c, 4, [gc(3)])], "wave", S=4),
        Doc("D run broken by a clock gap", [upd(c, 0, [gc(2), gc(1)]), upd(c, 4, [gc(1), gc(3)])], "wave", S=4),
        Doc("D run broken by a client change", [upd(c, 0, [gc(2), gc(1)]), upd(c - 1, 3, [gc(1), gc(3)])], "wave", S=4,
            struct_clients=2),
        Doc("D same clocks, two clients", [update([block(c, 0, [gc(2)]), block(c - 1, 0, [gc(2)])]), upd(c, 2, [gc(1)]),
                                           upd(c - 1, 2, [gc(1)])], "wave", S=4, struct_clients=2),
        Doc("D GC straight after a Skip", [upd(c, 0, [gc(2), skip(3), gc(1)]), upd(c, 2, [gc(3)])], "wave", S=3),
        Doc("D GC after a Skip, the gap stays", [upd(c, 0, [gc(2), skip(3), gc(1), gc(1)]), upd(c, 7, [gc(3)])], "wave", S=4),
        Doc("D zero-length Skip between two GCs", [upd(c, 0, [gc(2), skip(0), gc(1)]), upd(c, 3, [gc(3)])], "wave", S=3),
        Doc("D zero-length Skip between two GCs, alone", [upd(c, 0, [gc(2), skip(0), gc(1)]), EMPTY], "wave", S=2),
        Doc("D C-10 [GC0,GC1] + [GC2]", [upd(c, 0, [gc(1), gc(1)]), upd(c, 2, [gc(1)])], "wave", S=3),
        Doc("D C-10 reversed", [upd(c, 2, [gc(1)]), upd(c, 0, [gc(1), gc(1)])], "wave", S=3),
        Doc("D [GC0] + [GC1,GC2]", [upd(c, 0, [gc(1)]), upd(c, 1, [gc(1), gc(1)])], "wave", S=3),
        Doc("D [GC0] + [GC1] + [GC2]", [upd(c, 0, [gc(1)]), upd(c, 1, [gc(1)]), upd(c, 2, [gc(1)])], "wave", S=3),
        Doc("D [GC0,GC1,GC2] + empty", [upd(c, 0, [gc(1), gc(1), gc(1)]), EMPTY], "wave", S=3),
    ]
    return [docs]


# ---------------------------------------------------------------- E: Skips and gaps
# Lean refusal: every document starts with a GC (and most hold a Skip or a gap).
E_GAPS = [1, 127, 128, 2 ** 14 - 1, 2 ** 14, 2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 32 - 4]


def family_e():
    docs = []
    c = 1000
    for g in E_GAPS:        # the output Skip's length takes 1 .. 5 varuint bytes, both edges of each
        docs.append(Doc("E gap %d" % g, [upd(c, 0, [gc(1), ch()]), upd(c, 2 + g, [ch("z")])], "wave", S=3))
        docs.append(Doc("E gap %d, reversed" % g, [upd(c, 2 + g, [ch("z")]), upd(c, 0, [gc(1), ch()])], "wave", S=3))
        docs.append(Doc("E input Skip %d" % g, [upd(c, 0, [gc(1), skip(g), ch()]), upd(c, 2 + g, [ch("z")])], "wave", S=3))
    # 2^32 - 4 above: the last struct ends at 2^32 - 1.  One clock more and it leaves the wave tier (and the workgroup tier)
    g = 2 ** 32 - 3
    docs.append(Doc("E gap ends at 2^32", [upd(c, 0, [gc(1), ch()]), upd(c, 2 + g, [ch("z")])], "large", S=3))
    docs.append(Doc("E Skip up to 2^32 - 1, then nothing", [upd(c, 0, [gc(1), skip(2 ** 32 - 2)]), upd(c, 1, [ch()])], "wave", S=2))
    docs += [
        Doc("E non-zero first clocks", [upd(c, 5, [gc(1)]), upd(c - 1, 1000, [ch()]), upd(c, 6, [ch()]), upd(c + 9, 2 ** 21, [ch()])],
            "wave", S=4, struct_clients=3),
        Doc("E Skip at the start", [upd(c, 0, [skip(4), gc(1), ch()]), upd(c, 6, [ch()])], "wave", S=3),
        Doc("E Skip at the start, filled", [upd(c, 0, [skip(4), gc(1), ch()]), upd(c, 0, [ch(), ch(), ch(), ch()])], "wave", S=6),
        Doc("E Skip in the middle", [upd(c, 0, [gc(1), skip(4), ch()]), upd(c, 6, [ch()])], "wave", S=3),
        Doc("E Skip at the end", [upd(c, 0, [gc(1), ch(), skip(4)]), upd(c, 6, [ch()])], "wave", S=3),
        Doc("E Skip at the end, next to it", [upd(c, 0, [gc(1), ch(), skip(4)]), upd(c, 2, [ch()])], "wave", S=3),
        Doc("E two Skips in a row", [upd(c, 0, [gc(1), skip(2), skip(3), ch()]), upd(c, 7, [ch()])], "wave", S=3),
        Doc("E only Skips", [upd(c, 0, [skip(4), skip(1)]), upd(c, 0, [gc(1)])], "wave", S=1),
        Doc("E only Skips, twice", [upd(c, 0, [skip(4)]), upd(c - 1, 3, [skip(1)]), upd(c, 9, [gc(2)])], "wave", S=1),
        Doc("E only Skips, two blocks", [update([block(c, 0, [skip(4)]), block(c - 1, 3, [skip(1)])]), upd(c, 4, [gc(2)])], "wave", S=1),
        Doc("E a struct inside a skipped region", [upd(c, 0, [gc(1), skip(10), ch()]), upd(c, 5, [ch("m")])], "wave", S=3),
        Doc("E structs fill a skipped region", [upd(c, 0, [gc(1), skip(3), ch()]), upd(c, 1, [ch("m"), gc(2)])], "wave", S=4),
        Doc("E a GC run across a skipped region", [upd(c, 0, [gc(1), skip(2), gc(1)]), upd(c, 1, [gc(2)])], "wave", S=3),
    ]
    # gaps at the lane-block edges of a full wave document: every fourth struct follows a gap
    us, clock = [upd(c, 0, [gc(1)])], 1
    for j in range(255):
        clock += 3 if j % 4 == 2 else 0
        us.append(upd(c, clock, [ch()]))
        clock += 1
    docs.append(Doc("E 64 gaps at 4l - 1 | 4l", us, "wave", S=256))
    return [docs]


# ---------------------------------------------------------------- F: struct shapes through the re-encoding path
# Lean refusal: the struct at sorted position 1 (position 2 where the odd struct comes first) is a GC.
HI, LO = 3000000001, 7     # the plain document's client; another one below it / above it for the two-block updates
ODD = [  # (name, struct bytes, clock length)
    ("deleted", item(1, vu(3), origin=(HI, 0)), 3),
    ("json", item(2, vu(2) + text('{"a":1}') + text("2")), 2),
    ("binary", item(3, vu(3) + b"\x01\x02\xff"), 1),
    ("string", item(4, text("hello"), right=(LO, 4)), 5),
    ("embed", item(5, text('{"k":1}')), 1),
    ("format", item(6, text("bold") + text("true"), origin=(HI, 0)), 1),
    ("type", item(7, vu(0)), 1),
    ("type xml", item(7, vu(3) + text("p"), sub=b"k"), 1),
    ("any", item(8, vu(2) + b"\x7d\x05" + b"\x77\x01a"), 2),
    ("doc", item(9, text("guid") + b"\x76\x00"), 1),
    ("non-ascii string", item(4, text("hé€\U0001F600")), 5),
    ("non-ascii key", item(4, text("a"), parent=b"\x01" + text("clé")), 1),
    ("parentSub", item(4, text("v"), sub=b"key"), 1),
    ("non-ascii parentSub", item(4, text("v"), sub="clé".encode()), 1),
    ("parentSub flag with an origin", item(4, text("v"), origin=(HI, 0), flag20=True), 1),
    ("parent id", item(4, text("q"), parent=b"\x00" + vu(LO) + vu(2)), 1),
    ("non-minimal id", item(4, text("q"), origin=vu(HI) + b"\x85\x00"), 1),
    ("non-minimal length", b"\x04\x01\x01t\x81\x00q", 1),
    ("non-minimal parentInfo", b"\x04\x81\x00\x01t\x01q", 1),
    ("non-minimal GC length", b"\x00\x82\x00", 2),
]
NONCANON = [  # ContentAny / ContentJSON the writer would not reproduce: the oracle decides
    ("any float32 of an integer", item(8, vu(1) + b"\x7c\x40\x00\x00\x00"), 1),
    ("any float64 of an integer", item(8, vu(1) + b"\x7b\x40\x00\x00\x00\x00\x00\x00\x00"), 1),
    ("any bigint", item(8, vu(1) + b"\x7a\x00\x00\x00\x00\x00\x00\x00\x05"), 1),
    ("json with spaces", item(2, vu(1) + text('{ "a" : 1 }')), 1),
    ("json undefined", item(2, vu(1) + text("undefined")), 1),
]


def odd_doc(S, at, odd, ln, blocks=None):
    """S structs, those of client HI one per update (two per update from S = 257 on); the struct at sorted position
    `at` of HI's is `odd`.  blocks: 'desc' / 'asc' -- the odd update carries a second block of one struct, of client
    LO / 2^32 - 2."""
    if blocks:
        S -= 1
    per = 1 if S <= 256 else 2
    us, clock, j = [], 0, 0
    gc_at = 2 if at == 0 else 1
    while j < S:
        structs, start, has_odd = [], clock, False
        for q in range(min(per, S - j)):
            if j == at:
                structs.append(odd)
                clock += ln
                has_odd = True
            elif j == gc_at:
                structs.append(gc(2))
                clock += 2
            else:
                structs.append(ch("abcdefg"[j % 7]))
                clock += 1
            j += 1
        if blocks and has_odd:
            us.append(update([block(HI, start, structs), block(LO if blocks == "desc" else 2 ** 32 - 2, 0, [ch("o")])]))
        else:
            us.append(upd(HI, start, structs))
    return us


def family_f():
    docs, nc = [], []
    for S, tier in ((256, "wave"), (512, "workgroup")):
        for at in (0, S // 2, S - 1):
            for name, odd, ln in ODD:
                docs.append(Doc("F %s at %d of %d" % (name, at, S), odd_doc(S, at, odd, ln), tier, S=S, k=256, struct_clients=1))
            docs.append(Doc("F two blocks descending at %d of %d" % (at, S), odd_doc(S, min(at, S - 2), ch("w"), 1, "desc"),
                            tier, S=S, struct_clients=2))
            docs.append(Doc("F two blocks ascending at %d of %d" % (at, S), odd_doc(S, min(at, S - 2), ch("w"), 1, "asc"),
                            "large", S=S, struct_clients=2))
            for name, odd, ln in NONCANON:
                nc.append(Doc("F %s at %d of %d" % (name, at, S), odd_doc(S, at, odd, ln), None, valid=False))
    return [docs], [nc]


# ---------------------------------------------------------------- G: delete sets
# Lean refusal: every document with structs starts with a GC; the delete-set-only documents hold an update of more than
# 64 bytes (and most of them more than 64 ranges).
G_SHAPES = [  # (D, delete-set clients, tier)
    (1, 1, "wave"), (64, 64, "wave"), (65, 65, "workgroup"), (65, 5, "wave"), (127, 63, "wave"), (128, 64, "wave"), (128, 1, "wave"),
    (128, 65, "workgroup"), (129, 1, "workgroup"), (129, 64, "workgroup"), (255, 63, "workgroup"), (256, 64, "workgroup"),
    (256, 65, "workgroup"), (257, 65, "large"), (257, 1, "large"),
]


def ranges_for(n, shift, rng):
    """n range records of one client: fresh, adjacent, overlapping, contained, duplicate and zero-length ones in
    turn, starting the turn at `shift` (so that each kind falls on both sides of the two-element lane block)."""
    out, start, ln = [], rng.randrange(0, 40), 3
    for i in range(n):
        kind = (i + shift) % 7 if i else 0
        if kind in (0, 6):
            start, ln = start + ln + 2 + rng.randrange(3), 1 + rng.randrange(4)     # fresh
        elif kind == 1:
            start, ln = start + ln, 2                                                 # adjacent
        elif kind == 2:
            start, ln = start + ln - 1, 3                                             # overlapping
        elif kind == 3:
            start, ln = start + 1, 1 if ln > 2 else ln                                # contained (or overlapping)
        elif kind == 4:
            pass                                                                      # duplicate
        else:
            start, ln = start + ln + 4, 0                                             # zero-length, on its own
        out.append((start, ln))
    return out


def ds_updates(D, ncl, seed, with_structs, per_update=9, grouped=False):
    """D range records of ncl clients spread over updates of at most `per_update` records, in shuffled order (the
    clients' first sight is not their descending order)."""
    rng = random.Random(seed)
    ids = client_ids(ncl, "one" if grouped else ("mixed", "one", "five")[seed % 3], seed=seed + 100) if ncl > 1 else [(7, 3000000001, 100)[seed % 3]]
    share = [D // ncl + (1 if c < D % ncl else 0) for c in range(ncl)]
    if grouped:    # (a client's records together, shuffled among themselves: fewer bytes)
        recs = []
        for c in range(ncl):
            mine = [(ids[c], r) for r in ranges_for(share[c], seed + c, rng)]
            rng.shuffle(mine)
            recs += mine
    else:
        recs = [(ids[c], r) for c in range(ncl) for r in ranges_for(share[c], seed + c, rng)]
        rng.shuffle(recs)
    us = []
    if with_structs:   # client 7: in the delete set of the one-client documents of seed 0 mod 3, absent otherwise
        us.append(upd(7, 0, [gc(2), ch()]))
    for i in range(0, len(recs), per_update):
        part, ds = recs[i:i + per_update], []
        for c, r in part:          # (one entry per run of a client: a client may stand twice in one update's delete set)
            if ds and ds[-1][0] == c:
                ds[-1][1].append(r)
            else:
                ds.append((c, [r]))
        if with_structs and i % (2 * per_update) == 0:
            us.append(upd(8 + i, 0, [ch()], ds=encode_ds(ds)))
        else:
            us.append(b"\x00" + encode_ds(ds))
    return us


def family_g():
    docs = []
    for n, (D, ncl, tier) in enumerate(G_SHAPES):
        us = ds_updates(D, ncl, n, with_structs=True)
        docs.append(Doc("G D=%d clients=%d" % (D, ncl), us, tier, D=D, ds_clients=ncl))
        if D >= 64:
            us = ds_updates(D, ncl, n + 50, with_structs=False, per_update=40)
            if len(us) < 2:
                us.append(EMPTY)
            docs.append(Doc("G D=%d clients=%d, delete set only" % (D, ncl), us, tier, D=D, ds_clients=ncl, S=0))
    # one update carrying 256 (and 300) ranges: the first-seen rank of its later ranges saturates in the records
    for D, ncl, tier in ((256, 2, "workgroup"), (256, 64, "workgroup"), (300, 3, "large")):
        us = ds_updates(D, ncl, D + ncl, with_structs=False, per_update=D, grouped=True)
        assert len(us) == 1 and len(us[0]) < 1024
        docs.append(Doc("G %d ranges in one update, %d clients" % (D, ncl), [upd(7, 0, [gc(1)])] + us, tier, D=D, ds_clients=ncl, S=1))
        docs.append(Doc("G %d ranges in one update, %d clients, then more" % (D, ncl), us + [upd(7, 0, [gc(1)])], tier, D=D,
                        ds_clients=ncl, S=1))
    # 128 ranges in one update and one more client seen first: the wave record's rank of the big update's ranges
    us = ds_updates(127, 3, 9, with_structs=False, per_update=127, grouped=True)
    docs.append(Doc("G 127 ranges in one update after another client", [upd(7, 0, [gc(1)], ds=encode_ds([(1, [(0, 1)])]))] + us, "wave",
                    D=128, ds_clients=4, S=1))
    return [docs]


# ---------------------------------------------------------------- the corpus
_FAMILIES = None


def families():
    """{family: [batch, ...]}; the families of throwing / non-canonical inputs ('B invalid', 'F noncanon') carry no
    tier labels."""
    global _FAMILIES
    if _FAMILIES is None:
        f, fnc = family_f()
        _FAMILIES = {"A": family_a(), "B": family_b_valid(), "B invalid": family_b_invalid(), "C": family_c(), "D": family_d(),
                     "E": family_e(), "F": f, "F noncanon": fnc, "G": family_g()}
    return _FAMILIES


TIERED = ["A", "B", "C", "D", "E", "F", "G"]
PARITY_ONLY = ["B invalid", "F noncanon"]


def find(family, name):
    for batch in families()[family]:
        for d in batch:
            if d.name == name:
                return d
    raise KeyError(name)


def reuse_batches():
    """Batches for the persistent-grid reuse tests: a document that fills one of a wave's / workgroup's LDS arrays,
    then one that leaves it almost empty, in turn."""
    small = Doc("40 bytes", [upd(9, 0, [gc(2)]), str_update(9, 2, 40 - len(upd(9, 0, [gc(2)])))[0]], "wave", nbytes=40)
    wave = [find("A", "A S=256 clients=64 shuffled"), find("G", "G D=128 clients=64, delete set only"),      # S = 256 then S = 0
            find("G", "G D=128 clients=1"), find("A", "A S=2 clients=1 log"),                                  # D = 128 then D = 0
            find("A", "A S=256 clients=64 log"), find("A", "A S=256 clients=1 reversed"),                      # 64 clients then 1
            find("B invalid", "B invalid truncated at 255"), find("B", "B k=256"),                             # an error then none
            find("C", "C nbytes=8176"), small,                                                                  # 8176 bytes then 40
            find("B invalid", "B invalid past 2^53 at 0"), find("D", "D 256 GCs, source change at 128"),
            find("E", "E 64 gaps at 4l - 1 | 4l"), find("D", "D C-10 [GC0,GC1] + [GC2]"),
            find("G", "G 127 ranges in one update after another client"), find("E", "E only Skips")]
    tiny = [find("A", "A S=65 clients=65 log"), find("G", "G D=65 clients=65, delete set only"), find("A", "A S=257 clients=8 log")]
    work = []
    for n, d in enumerate([find("C", "C nbytes=16384"), find("A", "A S=512 clients=63 shuffled"), find("G", "G D=256 clients=64"),
                           find("A", "A S=512 clients=65 reversed"), find("G", "G D=256 clients=65, delete set only"),
                           find("D", "D run 6 at 255|256"), find("F", "F non-minimal id at 511 of 512")]):
        work += [d, tiny[n % 3]]
    return wave * 2, work * 2

"""Hand-built update-V1 documents for the large-document merge tier: k_big_pick, k_big_scan, k_big_val and k_merge_big
in its mid (4 waves, 1 KB tiles) and wide (16 waves, 4 KB tiles) size.  Every document's largest update -- U0, the
snapshot, the first of equal ones -- has at least ROUTE bytes, so the routing pass sends it to the tier; the other
updates are its log.  Every document sits on a constant of the tier (restated below with the line it mirrors), and
carries the outcome the kernels' rules give it:

  'mid'          on the mid list, finished by the mid size
  'wide_first'   U0 over MID_U0 bytes: on the wide list, finished by the wide size
  'mid_to_wide'  on the mid list; the log has more than MID_MAXS structs or MID_MAXD delete ranges, so the mid size
                 hands it to the wide size, which finishes it
  'seq'          handed to the sequential replay (Doc.via_wide: by the wide size, after a hand-on from the mid size)

`expected_outcome` restates those rules over a byte-level census (`layout`, `census`); `scan_contrib` restates what
the scan carves for a document (positions, tasks) and a lower bound of its slow queue.  The corpus is plain data:
`families()` returns {name: [batch, ...]}, a batch being a list of `Doc`s that go to the device together.

Labels corrected against the kernel (the issue's first guess in brackets):
  * non-minimal block-header varuints [seq]: 'mid'.  The follow records hcanon = 0 for such a block and acanon = 0
    for the document; the serial emit then writes the header again from its values (o.vu) instead of copying it, which
    is what the oracle writes.  Nothing defers.
  * U0 over MID_U0 with small blocks [a switch]: YGM_BIG_SMALLBLK_KB equals YGM_BIG_MID_KB, so k_big_pick's block test
    only runs for documents already on the wide list; both documents are 'wide_first'.  They still differ inside
    k_merge_big (use_bh: the tile's block table).
  * a ContentDoc struct in U0 [second scan class]: big_cand() refuses ref 9, big_struct() refuses it too ("validated by
    the general path"): 'seq'.
  * parentInfo 2 [left open]: the oracle reads it as an id parent and writes parentInfo 0, the tier copies bytes, so
    big_struct() refuses it: 'seq'.  The same for a non-minimal varuint in a first-class struct.

Left out: overflow of the slow queue (vq_cap = npos_cap / 4 + 1024) and of npos_cap / ntask_cap.  All three are sized
from the batch's own bytes with slack (big_scan_layout), so no input reaches them by construction."""
from general_tier_docs import block, ch, chars, gc, padded, skip, struct_len, update
from lean_docs import item, text, upd
from v1util import _skip_struct, encode_ds, rd_vu, read_ds, vu

# ---------------------------------------------------------------- the tier's constants
ROUTE = 1024                                   # ygm_kernels.hip: BIG_ROUTE_MIN (k_route_big)
SCAN_CH, WCH, MARGIN = 4096, 1024, 256         # k_big_scan: BIG_SCAN_CH, WCH = BIG_SCAN_CH / 4, MARGIN
VCAP = 64                                      # BIG_VCAP: bytes of a struct the scan gives a verdict
LEN15 = 0x8000                                 # big_word: the scan's 15-bit byte length
V16_MAX = 0xFFFE                               # big_v16: the largest clock length of the 16-bit verdict
MID_U0 = 512 * 1024                            # BIG_MID_U0 (and YGM_BIG_SMALLBLK_KB)
MID_MAXS = MID_MAXD = 256                      # BigCfgM: log structs / delete ranges in the mid size's LDS
WIDE_MAXS = WIDE_MAXD = 1024                   # ygm_merge_big.hpp: LB_MAXS, LB_MAXD (BigCfgL)
LG_LIST = 256                                  # k_merge_big: log updates staged in LDS
TILE_M, TILE_W, TILE_OV = 1024, 4096, 80       # BigCfgM::CH, BigCfgL::CH, TILE = CH + 64 + 16
LG_CAP_M = 13 * TILE_M + TILE_OV - 16 * LG_LIST     # sizeof(Tile) - LG_LIST * sizeof(BigCp): 9296
LG_CAP_W = 13 * TILE_W + TILE_OV - 16 * LG_LIST     # 49232
FOLLOW = 64                                    # k_merge_big: structs of a block per follow step (block table: nst < 64)
PICK = 16                                      # k_big_pick: documents per workgroup

OUTCOMES = ("mid", "wide_first", "mid_to_wide", "seq")
C0 = 100              # U0's client in the one-block documents
LOGC = 60             # the log's client (absent from U0 unless a family says otherwise)


class Doc:
    """us: the updates; outcome: one of OUTCOMES, or None in the parity-only lists; via_wide: a 'seq' document the mid
    size hands to the wide size first; seq135: 'seq' under compat135 whatever `outcome` says; placed: {name: struct
    record} of the structs the builder placed in U0; want: what the CPU test checks of them."""

    def __init__(self, name, us, outcome, valid=True, via_wide=False, seq135=False, placed=None, **want):
        self.name, self.us, self.outcome, self.valid = name, list(us), outcome, valid
        self.via_wide, self.seq135, self.placed, self.want = via_wide, seq135, placed or {}, want


# ---------------------------------------------------------------- a snapshot with structs at chosen bytes
def pad(size, client=C0):
    """A string struct with an origin (first scan class) of exactly `size` bytes; returns (bytes, clock length)."""
    for origin, right in (((client, 0), None), ((client, 0), (client, 1))):
        base = len(item(4, b"", origin=origin, right=right))
        for ln in (1, 2, 3):
            n = size - base - ln
            if n >= 1 and len(vu(n)) == ln:
                b = item(4, text("x" * n), origin=origin, right=right)
                assert len(b) == size
                return b, n
    raise ValueError(size)


def S(b, clen=1, name=None):
    return ("s", b, clen, name)


def TO(offset, piece=None):
    """Pad structs up to U0 byte `offset`: one, or pieces of `piece` bytes and a last one."""
    return ("to", offset, piece)


FILL = ("fill", None, None)    # pad up to the update's `total` bytes (last block only)
FILL40 = ("fill", None, 40)


def _block(start, client, clock0, ops, nlen, end, placed, bi):
    pos = start + nlen + len(vu(client)) + len(vu(clock0))
    structs, clock = [], clock0

    def put(b, clen, name):
        nonlocal pos, clock
        if name:
            placed[name] = dict(off=pos, nbytes=len(b), clock=clock, clen=clen, block=bi, index=len(structs))
        structs.append(b)
        pos += len(b)
        clock += clen

    for op in ops:
        if op[0] == "s":
            put(op[1], op[2], op[3])
            continue
        target = end if op[0] == "fill" else op[1]
        piece = op[2]
        assert target >= pos, (target, pos)
        while piece and target - pos >= piece + 8:
            put(*pad(piece, client), None)
        if target > pos:
            put(*pad(target - pos, client), None)
    if len(vu(len(structs))) != nlen:
        return None
    return block(client, clock0, structs)


def snapshot(blocks, ds=b"\x00", total=None):
    """blocks: [(client, clock0, ops)].  Returns the update and {name: record} of its named structs."""
    out, placed = vu(len(blocks)), {}
    for bi, (client, clock0, ops) in enumerate(blocks):
        for nlen in (1, 2, 3):
            trial = {}
            b = _block(len(out), client, clock0, ops, nlen, (total or 0) - len(ds), trial, bi)
            if b is not None:
                break
        out += b
        placed.update(trial)
    out += ds
    assert total is None or len(out) == total, (len(out), total)
    return out, placed


def one_block(ops, total=None, ds=b"\x00", client=C0, clock0=0):
    return snapshot([(client, clock0, ops)], ds, total)


SMALL_LOG = [upd(LOGC, 0, [ch("l")])]


def doc(name, u0, outcome, log=None, placed=None, u0_first=True, **kw):
    log = list(SMALL_LOG if log is None else log)
    return Doc(name, [u0] + log if u0_first else log + [u0], outcome, placed=placed, **kw)


# ---------------------------------------------------------------- byte-level walker and census
def layout(u):
    """U0 as the kernels see it: blocks [dict(h0, client, clock0, nst, structs)], a struct being dict(off, nbytes, clock,
    clen, info), and the delete set's offset."""
    blocks = []
    nb, p = rd_vu(u, 0)
    for _ in range(nb):
        h0 = p
        nst, p = rd_vu(u, p)
        client, p = rd_vu(u, p)
        clock, p = rd_vu(u, p)
        B = dict(h0=h0, client=client, clock0=clock, nst=nst, structs=[])
        for _ in range(nst):
            e = _skip_struct(u, p)
            ln = struct_len(u, p)
            B["structs"].append(dict(off=p, nbytes=e - p, clock=clock, clen=ln, info=u[p]))
            clock += ln
            p = e
        B["clock1"] = clock
        blocks.append(B)
    ds0 = p
    ds, p = read_ds(u, p)
    assert p == len(u), (p, len(u))
    return blocks, ds0, ds


def pick_u0(us):
    """Index of U0: the largest update, the first of equal ones (k_big_pick, k_merge_big)."""
    return max(range(len(us)), key=lambda i: (len(us[i]), -i))


def big_cand(ib):
    rf = ib & 31
    return ib == 0 or (1 <= rf <= 8 and not ((ib & 0xC0) and (ib & 0x20)))


def first_class(info):
    """The scan's first queue class: GC, and Items with an origin and deleted / string content."""
    return info == 0 or bool((info & 0xC0) and (info & 31) in (1, 4))


def _scan_parses(u, s):
    """big_skip with jcap 8 takes the struct: no Skip, refs 1-8, JSON / Any of at most 8 entries, Any scalars only."""
    info, p = s["info"], s["off"]
    ref = info & 31
    if info == 10 or ref > 8:
        return False
    if ref in (2, 8):
        q = _content_at(u, p)
        n, q = rd_vu(u, q)
        if n > 8:
            return False
        if ref == 8:
            for _ in range(n):
                if u[q] in (117, 118):
                    return False
                q = _skip_any_scalar(u, q)
    return True


def _content_at(u, p):
    info = u[p]
    q = p + 1
    for bit in (0x80, 0x40):
        if info & bit:
            q = rd_vu(u, rd_vu(u, q)[1])[1]
    if (info & 0xC0) == 0:
        pi, q = rd_vu(u, q)
        if pi == 1:
            n, q = rd_vu(u, q)
            q += n
        else:
            q = rd_vu(u, rd_vu(u, q)[1])[1]
        if info & 0x20:
            n, q = rd_vu(u, q)
            q += n
    return q


def _skip_any_scalar(u, q):
    from v1util import _skip_any
    return _skip_any(u, q)


def scan_contrib(us):
    """What k_big_pick carves for the document, and a lower bound of its slow-queue entries: U0's real structs of the
    second class that the scan parses in at most VCAP bytes and whose end is a candidate byte (k_big_scan's `slow`).
    Bytes inside other structs that parse by chance add to the real count, never take from it."""
    u = us[pick_u0(us)]
    n0 = len(u)
    blocks, ds0, _ = layout(u)
    slow = 0
    for B in blocks:
        for s in B["structs"]:
            if first_class(s["info"]) or not big_cand(s["info"]) or s["nbytes"] > VCAP or not _scan_parses(u, s):
                continue
            if (s["info"] & 0xC0) == 0 and u[s["off"] + 1] > 1:     # (parentInfo over 1: taken off the queue)
                continue
            end = s["off"] + s["nbytes"]
            slow += 1 if big_cand(u[end]) else 0
    return dict(positions=(n0 + 16 + 31) // 32 * 32, tasks=(n0 + SCAN_CH - 1) // SCAN_CH, slow_queue=slow)


def census(us):
    """The log's counts (every update but U0) and the reasons a document leaves the tier for the sequential replay."""
    i0 = pick_u0(us)
    u0 = us[i0]
    n0 = len(u0)
    S_ = D = 0
    reasons = []
    pieces = {}          # client -> [(clock, end, is_gc, 'log' / 'u0')]
    dsc = set()
    for i, u in enumerate(us):
        if i == i0:
            continue
        blocks, _, ds = layout(u)
        prev = None
        for B in blocks:
            if B["client"] >= 2 ** 32 or (prev is not None and B["client"] >= prev):
                reasons.append("log clients not descending")
            prev = B["client"]
            for s in B["structs"]:
                S_ += 1
                info = s["info"]
                if info == 10 or (info & 31) > 8 or ((info & 0xC0) and (info & 0x20)) or s["clen"] == 0:
                    reasons.append("log struct the tier does not take")
                pieces.setdefault(B["client"], []).append((s["clock"], s["clock"] + s["clen"], (info & 31) == 0, "log"))
        for client, rs in ds:
            D += len(rs)
            dsc.add(client)
    blocks, ds0, ds = layout(u0)
    dsc |= {c for c, _ in ds}
    nb = len(blocks)
    if nb > n0 // 4 + 1:
        reasons.append("more blocks than n0 / 4 + 1")
    prev = None
    for B in blocks:
        if B["nst"] == 0:
            reasons.append("empty block")
        if B["client"] >= 2 ** 32 or (prev is not None and B["client"] >= prev):
            reasons.append("U0 clients not descending")
        prev = B["client"]
        for s in B["structs"]:
            if s["info"] == 10 or (s["info"] & 31) > 8 or s["clen"] == 0:
                reasons.append("U0 struct the tier does not take")
        if B["structs"]:
            st = B["structs"]
            pieces.setdefault(B["client"], []).append((B["clock0"], B["clock1"], (st[0]["info"] & 31) == 0, "u0", (st[-1]["info"] & 31) == 0))
    for client, ps in pieces.items():
        ps.sort(key=lambda x: (x[0], x[3] != "u0"))
        for a, b in zip(ps, ps[1:]):
            last_gc = a[4] if a[3] == "u0" else a[2]
            if b[0] < a[1]:
                reasons.append("overlap")
            elif b[0] == a[1] and last_gc and b[2]:
                reasons.append("GC junction")
    return dict(k=len(us), n0=n0, u0=i0, S=S_, D=D, log_updates=len(us) - 1, log_bytes=sum(map(len, us)) - n0, nb=nb,
                ds_clients=len(dsc), reasons=reasons)


def expected_outcome(us, noncanon=False, compat135=False):
    """(outcome, via_wide).  noncanon: the builder says U0 or the log holds a struct write_struct would not reproduce
    (big_struct refuses it: not something a census of lengths sees)."""
    c = census(us)
    wide = c["n0"] > MID_U0
    log_bad = any(r.startswith("log") for r in c["reasons"])
    over_mid = c["S"] > MID_MAXS or c["D"] > MID_MAXD
    over_wide = c["S"] > WIDE_MAXS or c["D"] > WIDE_MAXD
    hand_on = not wide and over_mid and not log_bad and not noncanon == "log"
    seq = bool(c["reasons"]) or bool(noncanon) or over_wide or (compat135 and c["ds_clients"] > 1)
    if seq:
        return "seq", hand_on
    return ("wide_first" if wide else "mid_to_wide" if hand_on else "mid"), False


# ---------------------------------------------------------------- S: the scan
def sized(kind, nbytes, origin=(C0, 0)):
    """A second-class struct (or 'string' / 'deleted': first class) of exactly nbytes; (bytes, clock length)."""
    def fit(make, lo=0):
        for n in range(lo, nbytes):
            b = make(n)
            if len(b) == nbytes:
                return b
        raise ValueError((kind, nbytes))
    if kind == "string":
        return pad(nbytes)
    if kind == "parent string":
        b = fit(lambda n: item(4, text("p" * n)), 1)
        return b, rd_vu(b, 4)[0]
    if kind == "any":
        return fit(lambda n: item(8, vu(2) + b"\x7d\x05" + b"\x77" + text("a" * n), origin=origin)), 2
    if kind == "binary":
        return fit(lambda n: item(3, vu(n) + bytes([0x80 | (i & 0x7f) for i in range(n)]), origin=origin)), 1
    if kind == "embed":
        return fit(lambda n: item(5, text('"%s"' % ("e" * n)), origin=origin)), 1
    if kind == "format":
        return fit(lambda n: item(6, text("bold") + text('"%s"' % ("f" * n)), origin=origin)), 1
    if kind == "type":
        return fit(lambda n: item(7, vu(3) + text("n" * n), origin=origin), 1), 1
    if kind == "json8":
        return fit(lambda n: item(2, vu(8) + text('"%s"' % ("j" * n)) + text("1") * 7, origin=origin)), 8
    if kind == "json9":
        return fit(lambda n: item(2, vu(9) + text('"%s"' % ("j" * n)) + text("1") * 8, origin=origin)), 9
    raise ValueError(kind)


SECOND_CLASS = ["parent string", "any", "binary", "embed", "format", "type", "json8", "json9"]


def family_s():
    docs, nc = [], []
    for n0 in (4095, 4096, 4097, 8191, 8192, 8193):
        u, _ = one_block([FILL40], total=n0)
        docs.append(doc("S n0=%d" % n0, u, "mid", n0=n0))
    # struct starts at the last byte of a wave's quarter and at the first of the next (chunk 0 and chunk 1)
    for q0 in (0, SCAN_CH + 2 * WCH):
        for at in (q0 + WCH - 1, q0 + WCH):
            st = sized("any", 20)
            u, pl = one_block([TO(at, 40), S(*st, "x"), FILL40], total=at + 700)
            docs.append(doc("S struct starts at %d" % at, u, "mid", placed=pl, off={"x": at}))
    # the stage's end w0 + WCH + MARGIN: a string that begins in the quarter's last 24 bytes
    for q0 in (0, SCAN_CH + WCH):
        se = q0 + WCH + MARGIN
        for over in (0, 1, 300):
            at = q0 + WCH - 10
            st = pad(se + over - at)
            u, pl = one_block([TO(at, 40), S(*st, "x"), FILL40], total=se + 700)
            docs.append(doc("S string from %d ends %d past the stage" % (at, over), u, "mid", placed=pl, off={"x": at},
                            nbytes={"x": se + over - at}))
        at = q0 + WCH - 10            # ... and in U0's last chunk: the stage ends at n0
        st = pad(200)
        u, pl = one_block([TO(at, 40), S(*st, "x")], total=at + 201)
        docs.append(doc("S string from %d ends at n0 - 1" % at, u, "mid", placed=pl, off={"x": at}, n0=at + 201))
    # byte lengths VCAP - 1, VCAP, VCAP + 1: first class ...
    ops = []
    for n in (VCAP - 1, VCAP, VCAP + 1):
        ops += [S(*sized("string", n), "string %d" % n), S(gc(3), 3), S(item(1, vu(5), origin=(C0, 0)), 5)]
    u, pl = one_block(ops + [FILL40], total=1400)
    docs.append(doc("S first class 63 / 64 / 65", u, "mid", placed=pl, nbytes={"string %d" % n: n for n in (63, 64, 65)}))
    # ... second class, each mid-block (queued for k_big_val) and last in its block (k_merge_big validates)
    for kind in SECOND_CLASS:
        blocks, names = [], {}
        for j, n in enumerate((VCAP - 1, VCAP, VCAP + 1)):
            st = sized(kind, n)
            # (nine structs to a block: the count byte after a block's last struct is then no candidate info byte, so the
            #  scan's `slow` test fails for that struct)
            lead = [S(*pad(12, C0 - j)) for _ in range(5)]
            blocks.append((C0 - j, 0, lead + [S(*pad(30, C0 - j)), S(*st, "mid %d" % n), S(*pad(30, C0 - j)), S(*st, "last %d" % n)]))
            names["mid %d" % n] = names["last %d" % n] = n
        blocks.append((C0 - 3, 0, [FILL40]))
        u, pl = snapshot(blocks, total=1500)
        docs.append(doc("S second class %s 63 / 64 / 65" % kind, u, "mid", placed=pl, nbytes=names,
                        last_in_block=[k for k in names if k.startswith("last")]))
    st = item(9, text("guid") + b"\x76\x00", origin=(C0, 0))
    u, pl = one_block([S(*pad(30)), S(st, 1, "x"), FILL40], total=1200)
    docs.append(doc("S ContentDoc in U0", u, "seq", placed=pl))
    # the scan's 15-bit byte length, the 16-bit verdict
    for n in (LEN15 - 1, LEN15):
        u, pl = one_block([S(*pad(30)), S(*pad(n), "x"), FILL40], total=n + 1200)
        docs.append(doc("S struct of %d bytes" % n, u, "mid", placed=pl, nbytes={"x": n}))
    for n in (V16_MAX, V16_MAX + 1, V16_MAX + 2):
        u, pl = one_block([S(gc(n), n, "gc"), S(*pad(30)), S(item(1, vu(n), origin=(C0, 0)), n, "deleted"), FILL40], total=1300)
        docs.append(doc("S clock length %d" % n, u, "mid", placed=pl, clen={"gc": n, "deleted": n}))
    # strings: every tail of the 8-byte ASCII views; UTF-8 of 2, 3 and 4 bytes
    ops = [S(item(4, text("abcdefghijklmnopq"[:n]), origin=(C0, 0)), n, "ascii %d" % n) for n in range(1, 18)]
    u, pl = one_block(ops + [FILL40], total=1300)
    docs.append(doc("S ASCII strings of 1-17 bytes", u, "mid", placed=pl, clen={"ascii %d" % n: n for n in range(1, 18)}))
    multi = [("é", 1), ("€", 1), ("\U0001F600", 2), ("aé€\U0001F600z", 6), ("ééééééééé", 9), ("1234567€", 8), ("\U0001F600" * 5, 10)]
    ops = [S(item(4, text(s), origin=(C0, 0)), n, "utf8 %d" % i) for i, (s, n) in enumerate(multi)]
    ops += [S(item(4, text(s)), n, "utf8 parent %d" % i) for i, (s, n) in enumerate(multi)]
    u, pl = one_block(ops + [FILL40], total=1300)
    docs.append(doc("S UTF-8 strings", u, "mid", placed=pl, clen={"utf8 %d" % i: n for i, (s, n) in enumerate(multi)}))
    for name, raw in (("lone surrogate", b"a\xed\xa0\x80b"), ("overlong", b"a\xc0\x80b"), ("truncated sequence", b"ab\xe2\x82")):
        for form, mk in (("origin", lambda r: item(4, vu(len(r)) + r, origin=(C0, 0))), ("parent", lambda r: item(4, vu(len(r)) + r))):
            u, _ = one_block([S(*pad(30)), S(mk(raw), 3), FILL40], total=1200)
            nc.append(doc("S %s, %s form" % (name, form), u, None, valid=False))
    # parent-form Items
    forms = [("parentInfo 1", item(4, text("q")), "mid", False), ("parentInfo 0", item(4, text("q"), parent=b"\x00" + vu(C0) + vu(0)), "mid", False),
             ("parentInfo 2", item(4, text("q"), parent=b"\x02" + vu(C0) + vu(0)), "seq", True)]
    for name, st, outcome, noncanon in forms:
        u, pl = one_block([S(*pad(30)), S(st, 1, "x"), S(*pad(30)), S(st, 1, "y"), FILL40], total=1200)
        docs.append(doc("S %s" % name, u, outcome, placed=pl, noncanon=noncanon))
    for name, st, ln in (("GC length", b"\x00\x82\x00", 2), ("string length", item(4, b"\x81\x00q", origin=(C0, 0)), 1),
                         ("origin clock", item(4, text("q"), origin=vu(C0) + b"\x85\x00"), 1)):
        u, pl = one_block([S(*pad(30)), S(st, ln, "x"), FILL40], total=1200)
        docs.append(doc("S non-minimal %s" % name, u, "seq", placed=pl, noncanon=True))
    return [docs], [nc]


# ---------------------------------------------------------------- P: the pick
def small_doc(i, size=1100):
    u, _ = one_block([FILL40], total=size + i % 7, client=C0 + i % 20)
    return doc("P small %d" % i, u, "mid")


def many_blocks(n0, avg):
    """U0 of about n0 bytes in blocks of `avg` bytes on average (descending five-byte clients)."""
    nb = n0 // avg
    blocks = []
    for j in range(nb - 1):
        blocks.append((2 ** 31 - j, 0, [S(*pad(avg - 7 - 100, 2 ** 31 - j)), S(*pad(100, 2 ** 31 - j))]))
    head = snapshot(blocks)[0]
    total = nb * avg
    u, _ = snapshot(blocks + [(5, 0, [FILL40])], total=total + (0 if total - len(head) > 16 else 64))
    return u


_BIG = None


def big_docs():
    """The four documents around MID_U0 (built once)."""
    global _BIG
    if _BIG is None:
        at, over = one_block([TO(4000, 40), FILL], total=MID_U0), one_block([TO(4000, 40), FILL], total=MID_U0 + 1)
        _BIG = [doc("P n0=%d" % MID_U0, at[0], "mid", n0=MID_U0), doc("P n0=%d" % (MID_U0 + 1), over[0], "wide_first", n0=MID_U0 + 1),
                doc("P over 512 KB, blocks of 255", many_blocks(MID_U0 + 4096, 255), "wide_first", use_bh=True),
                doc("P over 512 KB, blocks of 257", many_blocks(MID_U0 + 4096, 257), "wide_first", use_bh=False)]
    return _BIG


def family_p():
    batches = [[small_doc(i) for i in range(n)] for n in (PICK - 1, PICK, PICK + 1, 2 * PICK + 1)]
    big = big_docs()
    batches.append([small_doc(0), big[1], small_doc(1), big[0], small_doc(2)])      # both lists: k_big_wait
    batches.append([big[1], big[2], big[3]])                                         # the wide list alone
    # two equal largest updates: the first is U0.  A (300 structs) first leaves B's 3 structs as the log; B first
    # leaves A's 300: over MID_MAXS
    a = upd(C0, 0, [ch("a")] * 300)
    b, _ = one_block([S(*pad(30, C0 - 1)), S(*pad(30, C0 - 1)), FILL], total=len(a), client=C0 - 1)
    assert len(a) == len(b) >= ROUTE
    batches.append([Doc("P equal largest, many structs first", [a, b] + SMALL_LOG, "mid", u0=0),
                    Doc("P equal largest, few structs first", [b, a] + SMALL_LOG, "mid_to_wide", u0=0),
                    Doc("P equal largest, after the log", SMALL_LOG + [b, a], "mid_to_wide", u0=1)])
    return batches


# ---------------------------------------------------------------- L: the log's caps
def base_u0(size=1100, client=C0, clock0=0, ds=b"\x00"):
    return one_block([FILL40], total=size, client=client, clock0=clock0, ds=ds)[0]


def ds_only(client, first, n, per=100):
    """n separate one-clock ranges of `client` from clock `first` (every other clock), `per` to an update."""
    us = []
    for i in range(0, n, per):
        us.append(b"\x00" + encode_ds([(client, [(first + 2 * j, 1) for j in range(i, min(i + per, n))])]))
    return us


def family_l():
    docs = []
    outs = {MID_MAXS: ("mid", False), MID_MAXS + 1: ("mid_to_wide", False), WIDE_MAXS: ("mid_to_wide", False), WIDE_MAXS + 1: ("seq", True)}
    for n, (outcome, via) in outs.items():
        docs.append(doc("L %d log structs" % n, base_u0(), outcome, log=chars(LOGC, 0, n), via_wide=via, S=n, D=0))
        docs.append(doc("L %d log ranges" % n, base_u0(), outcome, log=ds_only(LOGC, 0, n), via_wide=via, S=0, D=n))
    for k in (LG_LIST, LG_LIST + 1):     # staged in LDS / parsed from global memory
        log = chars(LOGC, 0, 200, per=1) + [b"\x00\x00"] * (k - 200)
        docs.append(doc("L %d log updates" % k, base_u0(), "mid", log=log, u0_first=False, log_updates=k, S=200))
    for cap, n_extra, outcome in ((LG_CAP_M, 0, "mid"), (LG_CAP_W, MID_MAXS + 1, "mid_to_wide")):
        for nbytes in (cap, cap + 1):
            head = chars(LOGC - 1, 0, n_extra)
            log = padded(nbytes, head, client=LOGC, clock=0, piece=1000)
            docs.append(doc("L log of %d bytes" % nbytes, base_u0(), outcome, log=log, log_bytes=nbytes))
        for nbytes in (cap - 1, cap, cap + 1):     # one log update alone at the stage's capacity (the kernel tests sz >= cap)
            head = chars(LOGC - 1, 0, n_extra)
            one, _ = one_block([FILL], total=nbytes, client=LOGC)
            docs.append(doc("L one log update of %d bytes" % nbytes, base_u0(cap + 100), outcome, log=head + [one],
                            log_bytes=nbytes + sum(map(len, head))))
    return [docs]


# ---------------------------------------------------------------- W: the walk
def residue_batch():
    """The same small document with U0 at every arena residue 0-15: a single-update filler document in front."""
    docs, at = [], 0
    for r in range(16):
        f = (r - at) % 16
        docs.append(Doc("W filler %d" % f, [bytes([1] * f)], None, nbytes=f))
        at += f
        d = doc("W residue %d" % r, base_u0(1100), "mid", residue=r)
        docs.append(d)
        at += sum(map(len, d.us))
    return docs


def residues(batch):
    at, out = 0, set()
    for d in batch:
        if len(d.us) >= 2:
            out.add(at % 16)
        at += sum(len(u) for u in d.us)
    return out


A8 = item(8, vu(1) + b"\x7d\x05", origin=(C0, 0), flag20=True)     # info 0xA8: written back as 0x88
MAPENT = item(8, vu(1) + b"\x7d\x05", sub=b"k")                    # info 0x28: a map entry, kept as it is
assert A8[0] == 0xA8 and MAPENT[0] == 0x28


def to_wide(n=MID_MAXS + 1):
    """A log that sends a document of the mid list on to the wide size."""
    return chars(LOGC, 0, n)


def family_w():
    docs, nc = [], []
    # tile edges: the first tile's positions are [1, 1 + CH) -- the walk starts at the first header, U0 byte 1
    for ch_, outcome, log in ((TILE_M, "mid", None), (TILE_W, "mid_to_wide", to_wide())):
        last = ch_                                  # the tile's last position
        big_client = 2 ** 32 - 5                    # five varuint bytes
        blocks = [(big_client + 1, 0, [TO(last - 1, 40)]), (big_client, 7, [S(*pad(30, 9)), FILL40])]
        u, pl = snapshot(blocks, total=last + 900)
        docs.append(doc("W client varuint across the last byte of the %d tile" % ch_, u, outcome, log=log, h0={1: last - 1}))
        u, pl = one_block([TO(last, 40), S(*sized("any", 20), "x"), FILL40], total=last + 900)
        docs.append(doc("W struct starts on the last byte of the %d tile" % ch_, u, outcome, log=log, placed=pl, off={"x": last}))
        u, pl = one_block([TO(last, 40), S(A8, 1, "x"), FILL40], total=last + 900)
        docs.append(doc("W 0xA8 struct on the last byte of the %d tile" % ch_, u, outcome, log=log, placed=pl, off={"x": last}))
    # structs per block around the follow step (and the block table's nst < 64)
    counts = (1, FOLLOW - 1, FOLLOW, FOLLOW + 1, 2 * FOLLOW - 1, 2 * FOLLOW, 2 * FOLLOW + 1)
    blocks = [(200 - j, 3, [S(item(4, text("abcdefg"[q % 7]), origin=(200 - j, 0))) for q in range(n)]) for j, n in enumerate(counts)]
    u, _ = snapshot(blocks)
    docs.append(doc("W blocks of 1-129 structs", u, "mid", nst=list(counts), use_bh=False))
    more = blocks + [(100 - j, 0, [S(item(4, text("z"), origin=(100 - j, 0)))]) for j in range(20)]
    u, _ = snapshot(more)
    docs.append(doc("W blocks of 1-129 structs, block table", u, "mid", nst=list(counts) + [1] * 20, use_bh=True))
    for log, outcome in ((None, "mid"), (to_wide(), "mid_to_wide")):
        for avg in (255, 257):
            blocks = [(200 - j, 0, [S(*pad(avg - 3 - 60, 200 - j)), S(*pad(60, 200 - j))]) for j in range(7)]
            u, _ = snapshot(blocks + [(5, 0, [FILL40])], total=8 * avg)
            docs.append(doc("W 8 blocks of %d bytes, %s" % (avg, outcome), u, outcome, log=log, use_bh=avg < 256, nb=8))
    # header errors
    ok = snapshot([(C0, 0, [S(*pad(30)), FILL40])], total=1200)[0][1:-1]           # one block's bytes
    blk2 = lambda client: block(client, 0, [pad(40, 7)[0]] * 14)
    for name, u, outcome, kw in (
            ("non-minimal struct count", vu(1) + b"\x83\x00" + vu(C0) + vu(0) + b"".join(pad(400)[0:1] * 3) + b"\x00", "mid", {}),
            ("non-minimal client", vu(1) + vu(3) + b"\xe4\x00" + vu(0) + b"".join(pad(400)[0:1] * 3) + b"\x00", "mid", {}),
            ("non-minimal clock", vu(1) + vu(3) + vu(C0) + b"\x80\x00" + b"".join(pad(400)[0:1] * 3) + b"\x00", "mid", {}),
            ("client 2^32", update([blk2(2 ** 32), blk2(9)]), "seq", {}),
            ("equal clients", update([blk2(9), block(9, 14 * 31, [pad(40, 7)[0]] * 14)]), "seq", {}),
            ("ascending clients", update([blk2(9), blk2(10)]), "seq", {})):
        docs.append(doc("W header: %s" % name, u, outcome, **kw))
    # empty client blocks: three bytes each, more than n0 / 4 + 1 of them (the oracle takes them: status 0, no output block)
    nb = 400
    u = vu(nb) + b"".join(b"\x00" + vu(127 - j % 128) + b"\x00" for j in range(nb)) + b"\x00"
    docs.append(doc("W %d empty client blocks" % nb, u, "seq", nb=nb))
    u = vu(nb) + b"".join(b"\x00" + vu(127 - j % 128) + b"\x00" for j in range(nb - 1)) + block(0, 0, [ch()]) + b"\x00"
    docs.append(doc("W empty client blocks, then a struct", u, "seq", nb=nb))
    u = vu(2) + block(C0, 0, [pad(520)[0], pad(520)[0]]) + b"\x00" + vu(C0 - 1) + b"\x00" + b"\x00"
    docs.append(doc("W one empty client block after a full one", u, "seq", nb=2))
    for name, raw in (("a truncated struct", ok[:-9]), ("a struct count one too many", vu(rd_vu(ok, 0)[0] + 1) + ok[1:])):
        nc.append(doc("W %s" % name, vu(1) + raw + b"\x00", None, valid=False))
    # log pieces against U0's blocks: clients 100 (clocks 10-...) and 50
    def u0_two(first_gc=False, last_gc=False):
        ops = ([S(gc(2), 2)] if first_gc else [S(*pad(12))]) + [TO(700, 40)] + ([S(gc(3), 3)] if last_gc else [S(*pad(13))])
        return snapshot([(C0, 10, ops), (50, 0, [FILL40])], total=1200)[0]
    plain = u0_two()
    end = layout(plain)[0][0]["clock1"]
    cases = [("before U0's block, with a gap", plain, [upd(C0, 2, [ch(), ch()])], "mid"),
             ("contiguous before U0's block", plain, [upd(C0, 8, [ch(), ch()])], "mid"),
             ("from clock 0 up to U0's block", plain, [upd(C0, 0, [ch()] * 10)], "mid"),
             ("contiguous after U0's block", plain, [upd(C0, end, [ch()])], "mid"),
             ("a gap after U0's block", plain, [upd(C0, end + 5, [ch()])], "mid"),
             ("before and after U0's block", plain, [upd(C0, 9, [ch()]), upd(C0, end, [ch()]), upd(C0, end + 3, [ch()])], "mid"),
             ("overlaps U0's first clock", plain, [upd(C0, 9, [ch(), ch()])], "seq"),
             ("overlaps U0's last clock", plain, [upd(C0, end - 1, [ch()])], "seq"),
             ("inside U0's block", plain, [upd(C0, 20, [ch()])], "seq"),
             ("a log GC before U0's Item", plain, [upd(C0, 8, [gc(2)])], "mid"),
             ("a log GC after U0's Item", plain, [upd(C0, end, [gc(2)])], "mid")]
    g0 = u0_two(first_gc=True)
    g1 = u0_two(last_gc=True)
    end1 = layout(g1)[0][0]["clock1"]
    cases += [("a log GC before U0's GC", g0, [upd(C0, 8, [gc(2)])], "seq"),
              ("a log Item before U0's GC", g0, [upd(C0, 9, [ch()])], "mid"),
              ("a log GC after U0's GC", g1, [upd(C0, end1, [gc(2)])], "seq"),
              ("a log GC one clock after U0's GC", g1, [upd(C0, end1 + 1, [gc(2)])], "mid"),
              ("two log GCs in a row", plain, [upd(C0, end, [ch(), gc(1)]), upd(C0, end + 2, [gc(2)])], "seq"),
              ("a log client above U0's", plain, [upd(120, 0, [ch()])], "mid"),
              ("a log client between U0's", plain, [upd(70, 4, [ch()])], "mid"),
              ("a log client below U0's", plain, [upd(10, 0, [ch(), gc(2)])], "mid"),
              ("log clients above, between and below", plain, [upd(10, 0, [ch()]), upd(120, 0, [ch()]), upd(70, 0, [ch()]), upd(C0, end, [ch()])], "mid"),
              ("a log Skip", plain, [upd(LOGC, 0, [ch(), skip(3), ch()])], "seq"),
              ("a log 0xA8 struct", plain, [upd(LOGC, 0, [A8])], "seq")]
    for name, u, log, outcome in cases:
        docs.append(doc("W log: %s" % name, u, outcome, log=log))
        if outcome == "mid":
            docs.append(doc("W log: %s, wide" % name, u, "mid_to_wide", log=log + chars(LOGC - 1, 0, MID_MAXS + 1)))
    # bit 0x20 beside an origin: the document's bitmap has one bit per U0 position, 32 to a word
    ats = (95, 128, 161, 320 + 31, 384, 416 + 1)
    ops = []
    for at in ats:
        ops += [TO(at, 40), S(A8, 1, "a8 %d" % at)]
    u, pl = one_block(ops + [FILL40], total=1300)
    docs.append(doc("W 0xA8 structs at bits 31, 0 and 1", u, "mid", placed=pl, off={"a8 %d" % at: at for at in ats}))
    docs.append(doc("W 0xA8 structs at bits 31, 0 and 1, wide", u, "mid_to_wide", log=to_wide(), placed=pl))
    return [docs, residue_batch(), ds_pair()], [nc]


def ds_pair():
    """The merged delete set of one client and of two (13.5 writes clients in first-seen order: the tier defers)."""
    one = doc("W delete set of one client", base_u0(ds=encode_ds([(C0, [(0, 2)])])), "mid", log=[upd(LOGC, 0, [ch()], ds=encode_ds([(C0, [(5, 1)])]))])
    two = doc("W delete set of two clients", base_u0(ds=encode_ds([(C0, [(0, 2)])])), "mid", seq135=True,
              log=[upd(LOGC, 0, [ch()], ds=encode_ds([(C0 + 1, [(5, 1)])]))])
    two_u0 = doc("W delete set of two clients in U0", base_u0(ds=encode_ds([(C0, [(0, 2)]), (C0 - 1, [(1, 1)])])), "mid", seq135=True)
    return [one, two, two_u0]


# ---------------------------------------------------------------- R: one context, batch after batch
_REUSE = None


def reuse_sequences():
    """{name: [batch, ...]} run in order on a fresh engine (built once)."""
    global _REUSE
    if _REUSE is None:
        _REUSE = _reuse_sequences()
    return _REUSE


def _reuse_sequences():
    ats = list(range(40, 1000, 24))
    rich, plain, one = [], [], []
    for i in range(6):
        total = 1200 + 32 * i
        ops_a, ops_m, ops_o = [], [], []
        for n, at in enumerate(ats):
            ops_a += [TO(at), S(A8, 1)]
            ops_m += [TO(at), S(MAPENT, 1)]
            ops_o += [TO(at), S(A8 if n == (i + 1) % len(ats) else MAPENT, 1)]
        rich.append(doc("R 0xA8 at every position %d" % i, one_block(ops_a + [FILL40], total=total)[0], "mid"))
        plain.append(doc("R map entries at the same positions %d" % i, one_block(ops_m + [FILL40], total=total)[0], "mid"))
        one.append(doc("R one 0xA8 among map entries %d" % i, one_block(ops_o + [FILL40], total=total)[0], "mid"))
    big = big_docs()
    large = [doc("R 40 KB %d" % i, one_block([FILL40], total=40000 + i)[0], "mid") for i in range(8)]
    small = [small_doc(i) for i in range(3)]
    return {"stale pbits": [rich, one, plain, rich],
            "grow-only scratch": [large + [big[0]], small, large[:2], small[:1]],
            "stream reuse": [[big[1], small_doc(5)], [small_doc(6), small_doc(7)], [big[1]], small]}


# ---------------------------------------------------------------- the corpus
_FAMILIES = None


def families():
    global _FAMILIES
    if _FAMILIES is None:
        s, snc = family_s()
        w, wnc = family_w()
        _FAMILIES = {"S": s, "S oracle decides": snc, "P": family_p(), "L": family_l(), "W": w, "W oracle decides": wnc}
    return _FAMILIES


TIERED = ["S", "P", "L", "W"]
PARITY_ONLY = ["S oracle decides", "W oracle decides"]


def find(family, name):
    for batch in families()[family]:
        for d in batch:
            if d.name == name:
                return d
    raise KeyError(name)


def predicted(docs, compat135=False, force_seq=False):
    """The `ygm large tiers:` line of one call over labelled documents (slow_queue: the lower bound)."""
    multi = [d for d in docs if len(d.us) >= 2]
    out = dict(docs=len(multi), positions=0, tasks=0, slow_queue=0, wide_first=0, mid_first=0, mid_to_wide=0, to_seq=0)
    for d in multi:
        c = scan_contrib(d.us)
        for k in ("positions", "tasks", "slow_queue"):
            out[k] += c[k]
        wide = len(d.us[pick_u0(d.us)]) > MID_U0
        out["wide_first" if wide else "mid_first"] += 1
        seq = force_seq or d.outcome == "seq" or (compat135 and d.seq135)
        out["to_seq"] += seq
        if not force_seq:
            out["mid_to_wide"] += d.outcome == "mid_to_wide" or (d.outcome == "seq" and d.via_wide)
    return out

"""The narrow lean merge kernel on the single-Item debounce shape and around it: row edges of the lane-per-update
parse, one odd update inside a row of plain ones, every varuint length, clock gaps / overlaps at the places a
per-block contiguity check can miss, and more documents than the persistent grid.  Every document is compared
with the CPU oracle; the tests describe behaviour (what is finished by the lean kernel, what is exact), not how
the kernel parses."""
import random

import numpy as np
import pytest

import oracle
from v1util import vu

pytestmark = pytest.mark.gpu

THROWS = {1, 2, 4, 5}


@pytest.fixture(scope="module")
def eng():
    from hocuspocus_amd import Engine
    e = Engine(0)
    yield e
    e.close()


# ---- a sequential log generator: every client's clocks stay contiguous unless a test shifts them
def item(info_ref, content, origin=None, right=None, parent=None, sub=None, flag20=False):
    """One struct: info byte, origins / parent, content bytes."""
    info = info_ref | (0x80 if origin else 0) | (0x40 if right else 0) | (0x20 if (sub is not None or flag20) else 0)
    b = bytes([info])
    for o in (origin, right):
        if o:
            b += o if isinstance(o, bytes) else vu(o[0]) + vu(o[1])
    if not origin and not right:
        b += parent if parent is not None else b"\x01\x01t"
        if sub is not None:
            b += vu(len(sub)) + sub
    return b + content


def text(s):
    raw = s.encode()
    return vu(len(raw)) + raw


def upd(client, clock, structs, ds=b"\x00", nst=None):
    cl = client if isinstance(client, bytes) else vu(client)
    ck = clock if isinstance(clock, bytes) else vu(clock)
    return vu(1) + vu(len(structs) if nst is None else nst) + cl + ck + b"".join(structs) + ds


class Log:
    """A document's log in the C2 shape: the first update inserts under the parent key 't', every later one is one
    character with an origin (and, every third, a right origin too) pointing at earlier characters."""

    def __init__(self, clients, clocks=None, seed=0):
        self.clients = list(clients)
        self.clock = dict(zip(self.clients, clocks or [0] * len(self.clients)))
        self.rng = random.Random(seed)
        self.ups = []
        self.last = None     # (client, clock) of the latest character

    def plain(self, c):
        """The fast shape: one ASCII character."""
        ch = self.rng.choice("abcdefghijklmnopqrstuvwxyz")
        if self.last is None:
            s = item(4, text(ch))
        elif len(self.ups) % 3 == 2:
            s = item(4, text(ch), origin=self.last, right=(self.clients[0], self.clock[self.clients[0]] // 2))
        elif len(self.ups) % 7 == 5:
            s = item(4, text(ch), right=self.last)
        else:
            s = item(4, text(ch), origin=self.last)
        self.put(c, [s], 1)

    def put(self, c, structs, clen, ds=b"\x00", shift=0, tail=b"", client_bytes=None, clock_bytes=None):
        ck = self.clock[c] + shift
        self.ups.append(upd(client_bytes or c, clock_bytes or ck, structs, ds) + tail)
        if clen:
            self.last = (c, ck + clen - 1)
        self.clock[c] = ck + clen

    def raw(self, u):
        self.ups.append(u)


def fast_doc(k, clients, clocks=None, seed=0, order=None):
    """k plain updates; order(i) -> client index of update i (default: round robin)."""
    g = Log(clients, clocks, seed)
    for i in range(k):
        g.plain(clients[order(i) if order else i % len(clients)])
    return g.ups


CLIENTS = [3000000001, 77, 2 ** 31 + 5, 12345, 999, 4000000000, 2, 65536]


def same(o, g):
    so, bo = o
    sg, bg = g
    if so in THROWS:
        return sg in THROWS
    return so == sg and bo == bg


def _pack(docs):
    blobs = [u for us in docs for u in us]
    a = np.frombuffer(b"".join(blobs) + bytes(64), np.uint8)
    lens = np.array([len(b) for b in blobs], np.uint16)
    off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.uint64)
    du = np.cumsum([0] + [len(us) for us in docs]).astype(np.uint32)
    doff = off[du]
    return blobs, a, lens, off, du, doff


def _unpack(r, n):
    import torch
    import bench
    torch.cuda.synchronize()
    offs = bench._d2h(r.off, n * 8).view(np.uint64)
    ln = bench._d2h(r.len, n * 8).view(np.uint64)
    sts = bench._d2h(r.status, n * 4).view(np.int32)
    data = bench._d2h(r.data, int(r.data_bytes)).tobytes()
    return [(int(sts[d]), data[int(offs[d]):int(offs[d]) + int(ln[d])] if sts[d] == 0 else None) for d in range(n)]


def run_device(eng, docs, form):
    """docs through the u64-offset device API ('off') or the compact one ('lens'): results, documents finished lean."""
    import torch
    blobs, a, lens, off, du, doff = _pack(docs)
    dev = torch.device("cuda", 0)
    ta, to, tl, td, tdo = (torch.from_numpy(x.copy()).to(dev) for x in
                           (a, off.view(np.int64), lens.view(np.int16), du.view(np.int32), doff.view(np.int64)))
    lean0 = eng.stats().docs_lean
    if form == "off":
        r = eng.merge_device(ta.data_ptr(), len(a) - 64, to.data_ptr(), td.data_ptr(), len(blobs), len(docs))
    else:
        r = eng.merge_device_lens(ta.data_ptr(), len(a) - 64, tdo.data_ptr(), tl.data_ptr(), td.data_ptr(), len(blobs), len(docs))
    res = _unpack(r, len(docs))
    return res, eng.stats().docs_lean - lean0


_ORACLE = {}


def expect(key, docs):
    """The oracle's results of a corpus, computed once."""
    if key not in _ORACLE:
        _ORACLE[key] = [oracle.merge_updates(us) for us in docs]
    return _ORACLE[key]


def check(eng, key, docs, form, lean=None):
    exp = expect(key, docs)
    res, took = run_device(eng, docs, form)
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

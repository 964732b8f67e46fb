"""Builders of the lean merge kernels' test documents: a sequential log generator in the single-Item debounce shape
(every client's clocks stay contiguous unless a test shifts them) and the pieces several suites share -- delete sets, a
non-minimal varuint, the deletion documents, the longest fast update.  A plain module: the lean test files, the general
and large tier corpora and the update-V2 tests build their documents from it; tests/test_lean_docs.py checks the corpora
of lean_slowclass_docs.py and lean_chunkmask_docs.py on the CPU."""
import random

from v1util import vu

CLIENTS = [3000000001, 77, 2 ** 31 + 5, 12345, 999, 4000000000, 2, 65536]
A, B, C = 5, 9, 70     # one-byte client ids: room for the long shapes inside 32 bytes


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


def text1(ch="q"):
    return b"\x01" + ch.encode()


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


def _ds(entries):
    """A delete set: entries = [(client, [(clock, len), ...]), ...]."""
    b = vu(len(entries))
    for cl, rs in entries:
        b += vu(cl) + vu(len(rs)) + b"".join(vu(ck) + vu(ln) for ck, ln in rs)
    return b


def _ds_only(client, clock, n=1):
    """A delete-set-only update: one range of one client."""
    return b"\x00\x01" + vu(client) + b"\x01" + vu(clock) + vu(n)


def overlong(b):
    """The same value with its last byte continued into a zero byte: ... | 0x80, 0x00."""
    return b[:-1] + bytes([b[-1] | 0x80, 0])


# ---- deletions between inserts; lanes holding only deletions
def _deletion_doc(ncl, k, dels, empty, seed):
    """k updates; the ones at the positions `dels` are deletions (no structs).  empty: their delete sets hold nothing
    (the union is empty); else one range each, of client ids in ascending order of first sight."""
    ids = [A, B, C, 200][:ncl]
    g = Log(ids, [5] * ncl, seed)
    n = 0
    for j in range(k):
        if j in dels:
            g.raw(b"\x00\x00" if empty else b"\x00" + _ds([(ids[n % ncl] if n % 3 else 300 + n, [(5 + 2 * n, 1)])]))
            n += 1
        else:
            g.plain(ids[(j * 7 // 3) % ncl])
    return g.ups


def _deletion_docs():
    docs = []
    for ncl in (1, 2, 3, 4):
        for empty in (False, True):
            docs.append(_deletion_doc(ncl, 90, {1, 2, 30, 63, 64, 89}, empty, 1))                       # between inserts
            docs.append(_deletion_doc(ncl, 90, set(range(8, 12)) | set(range(40, 48)), empty, 2))      # lanes 2, 10, 11: only deletions
            docs.append(_deletion_doc(ncl, 90, set(range(0, 8)) | set(range(84, 90)), empty, 3))       # the first two lanes, the last lanes
            docs.append(_deletion_doc(ncl, 61, set(range(6, 61)) - {33}, empty, 4))                    # nearly all deletions
            docs.append(_deletion_doc(ncl, 40, set(range(40)), empty, 5))                              # no structs at all
    return docs


# ---- the longest fast shape (a 32-byte update: parent key, one character)
def _longest(c, ck):
    pre = len(vu(1) + vu(1) + vu(c) + vu(ck))
    key = b"k" * (32 - pre - 1 - 5)      # info, parentInfo, key length, key, string length, character; the delete set's 0
    u = upd(c, ck, [item(4, text1("x"), parent=b"\x01" + vu(len(key)) + key)])
    assert len(u) == 32
    return u

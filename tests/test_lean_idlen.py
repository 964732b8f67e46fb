"""The narrow lean merge kernel's parse specialised for five-byte client ids.  Once per document the kernel asks
whether every update with structs carries a five-byte id (a client >= 2^28: fifteen of sixteen random uint32) and, if
so, parses all of its rows with that length built in; one foreign length anywhere sends the document down the generic
parse.  What can go wrong is a document taking the specialised parse that must not, a value cut from the wrong bytes
(client, clock, the info byte and what follows it all sit behind the id), and a document taken or deferred that was
not before -- so the corpora are

  lengths    one client on both sides of every id length, 2 to 4 clients in every mix of four- and five-byte ids, a
             document all five-byte except its first update, its last, or the update in each row of a lane;
  values     a fifth id byte with each bit of 0x70 (past a uint32: deferred), clocks of 1 to 5 bytes and the clock
             0xFFFFFFFF, every info byte of the fast shape, origins that name a four-byte client;
  shapes     delete-set-only updates between, before and after the inserts, a multi-character insert in one lane of
             each row, documents of 200 and 255 updates (every lane, all four rows), one with a fifth client.

Every corpus runs on two contexts, the default one and one opened under YGM_LN_NO_IDLEN=1 (every document takes the
generic parse), in both input forms: each result is the CPU oracle's, and the two contexts agree in status, bytes,
and in the counts of documents the narrow and the wide lean kernel finished.  Documents have 2 to 8 updates unless
stated."""
import itertools
import os
import subprocess

import pytest

from devrun import Memo, run_merge, same
from lean_docs import Log, _ds_only, item, text
from v1util import vu

gpu = pytest.mark.gpu
FORMS = ["off", "lens"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F4 = [2 ** 21, 2 ** 28 - 1, 12345678, 99999999]              # four-byte ids
F5 = [2 ** 28, 2 ** 31, 0xFFFFFFFF, 3000000001, 2 ** 28 + 1, 0x7FFFFFFF]   # five-byte ids


@pytest.fixture(scope="module")
def engs():
    """(default context, context with the id-length decision switched off): the switch is read when a context opens."""
    from hocuspocus_amd import Engine
    e = Engine(0)
    os.environ["YGM_LN_NO_IDLEN"] = "1"
    try:
        g = Engine(0)
    finally:
        del os.environ["YGM_LN_NO_IDLEN"]
    yield e, g
    g.close()
    e.close()


MEMO = Memo()
expect = MEMO.expect


def run(e, docs, form):
    wide0 = e.stats().docs_lean_wide
    res, lean = run_merge(e, docs, form)
    return res, lean, e.stats().docs_lean_wide - wide0


def check(engs, key, docs, lean=None, ok=True, wide=None):
    """Both contexts, both forms: exact against the oracle, identical to each other, the same tier counts; `lean`: the
    number of documents the lean kernels finish, `wide`: of them by the wide one; ok: the oracle merges every document."""
    exp = expect(key, docs)
    if ok:
        assert all(st == 0 for st, _ in exp), key
    for form in FORMS:
        got = [run(e, docs, form) for e in engs]
        for which, (res, _, _) in zip(("idlen", "generic"), got):
            bad = [d for d in range(len(docs)) if not same(exp[d], res[d])]
            assert not bad, (key, form, which, len(bad), bad[:5], [u.hex() for u in docs[bad[0]]][:8])
        (r0, l0, w0), (r1, l1, w1) = got
        diff = [d for d in range(len(docs)) if r0[d] != r1[d]]
        assert not diff, (key, form, "the two parses differ", diff[:5])
        assert (l0, w0) == (l1, w1), (key, form, "tier counts", (l0, w0), (l1, w1))
        if lean is not None:
            assert l0 == lean, (key, form, l0, lean)
        if wide is not None:
            assert w0 == wide, (key, form, w0, wide)


def log_doc(k, clients, clocks=None, order=None, infos=("o",), seed=0, origin_client=None):
    """k updates of one character: the first under the parent key, update i >= 1 with the ids infos[i % len(infos)]
    names -- 'o' an origin, 'r' a right origin, 'b' both (small clocks keep 'b' inside 32 bytes).  origin_client: the
    client every origin names (with clocks of its own), instead of the latest character's."""
    g = Log(clients, clocks, seed)
    for i in range(k):
        c = clients[order(i) if order else i % len(clients)]
        ch = text("abcdefgh"[i % 8])
        o = g.last if origin_client is None else (origin_client, i)
        if g.last is None:
            s = item(4, ch)
        else:
            kind = infos[i % len(infos)]
            s = item(4, ch, origin=o if kind in "ob" else None, right=(o[0], o[1] // 2) if kind in "rb" else None)
        g.put(c, [s], 1)
    assert all(len(u) <= 32 for u in g.ups), max(map(len, g.ups))
    return g.ups


# ======================================================================= lengths
def _boundary_docs():
    docs = []
    for c in (2 ** 21 - 1, 2 ** 21, 2 ** 28 - 1, 2 ** 28, 2 ** 31, 0xFFFFFFFF):
        for k in (2, 5, 8):
            docs.append(log_doc(k, [c], seed=k))
    for ncl in (2, 3, 4):
        for mix in itertools.product((4, 5), repeat=ncl):
            cl = [(F4 if b == 4 else F5)[j] for j, b in enumerate(mix)]
            docs.append(log_doc(8, cl, seed=ncl))
            docs.append(log_doc(8, cl, order=lambda i: (i * 3 + 1) % ncl, infos=("o", "r", "b"), seed=ncl))
    return docs


@gpu
def test_id_length_at_every_boundary_and_mix(engs):
    docs = _boundary_docs()
    check(engs, "bound", docs, lean=len(docs))


def _one_foreign_docs():
    """Eight updates (lanes 0 and 1, all four rows each) and twelve (a third lane) of a five-byte client, one of them
    -- each position in turn -- by a client of another id length (four, three, one byte)."""
    docs = []
    for k in (8, 12):
        for at in range(k):
            for other in (F4[at % 4], 2 ** 14 + 5, 77):
                g = Log([F5[at % 6], other], seed=at)
                for i in range(k):
                    c = other if i == at else g.clients[0]
                    g.put(c, [item(4, text("xy"[i % 2]), origin=g.last)], 1)
                docs.append(g.ups)
    return docs


@gpu
def test_all_five_byte_except_one_update(engs):
    docs = _one_foreign_docs()
    check(engs, "foreign", docs, lean=len(docs))


# ======================================================================= values
def _fifth_byte_docs():
    """The id's fifth byte with each bit of 0x70 (clients of 2^32, 2^33, 2^34 and beyond, as yjs would write them) in
    the first update, the last, or one in between, beside clean five-byte documents."""
    docs, kinds = [], []
    for bit in (0x10, 0x20, 0x40, 0x70):
        big = (bit << 28) | 0x0ABCDEF1
        assert len(vu(big)) == 5 and vu(big)[4] & 0x70 == bit
        for at in (0, 3, 7):
            g = Log([F5[1], big], seed=bit + at)
            for i in range(8):
                g.put(big if i == at else F5[1], [item(4, text("q"), origin=g.last)], 1)
            docs.append(g.ups)
            kinds.append(False)
            docs.append(log_doc(8, [F5[1], F5[2]], seed=bit + at))
            kinds.append(True)
    return docs, kinds


@gpu
def test_fifth_byte_past_a_uint32_is_deferred(engs):
    docs, kinds = _fifth_byte_docs()
    check(engs, "y70", docs, lean=sum(kinds))


CLOCK0 = [0, 120, 2 ** 14 - 4, 2 ** 21 - 4, 2 ** 28 - 4, 2 ** 32 - 9]   # eight clocks from each: across every length's edge


def _clock_docs():
    docs = []
    for c in (F5[0], F5[2]):
        for ck in CLOCK0:
            docs.append(log_doc(8, [c], [ck], seed=ck & 0xFF))
            docs.append(log_doc(8, [c, F5[3]], [ck, 2 ** 21 - 2], seed=ck & 0xFF))
            docs.append(log_doc(8, [c], [ck], origin_client=F5[4], seed=3))
    return docs


@gpu
def test_clock_of_every_length(engs):
    docs = _clock_docs()
    check(engs, "clocks", docs, lean=len(docs))


@gpu
def test_clock_ffffffff_is_exact_on_both_paths(engs):
    """A struct at clock 0xFFFFFFFF ends past a uint32: no lean document, whichever update holds it."""
    docs = []
    for k in (2, 5, 8):
        docs.append(log_doc(k, [F5[0]], [2 ** 32 - k], seed=k))            # the last update's clock is 0xFFFFFFFF
        docs.append(log_doc(k, [F5[0], F5[1]], [2 ** 32 - 1, 7], seed=k))   # the first one's
    check(engs, "ckmax", docs, ok=False)


def _info_docs():
    docs = []
    for infos in (("o",), ("r",), ("b",), ("o", "r", "b"), ("b", "o")):
        for cl in ([F5[0]], [F5[1], F5[2]], [F5[3], F5[4], F5[5], F5[0]]):
            docs.append(log_doc(8, cl, infos=infos, seed=len(docs)))
            docs.append(log_doc(8, cl, infos=infos, origin_client=F4[1], seed=len(docs)))   # origins name a four-byte client
            docs.append(log_doc(8, cl, infos=infos, origin_client=77, seed=len(docs)))      # and a one-byte one
    # the parent-key insert (row 0 of lane 0) with keys of 1 to 8 characters, alone with one successor and with seven
    for n in range(1, 9):
        for k in (2, 8):
            g = Log([F5[n % 6]], seed=n)
            g.put(g.clients[0], [item(4, text("a"), parent=b"\x01" + vu(n) + b"keykeyke"[:n])], 1)
            for i in range(1, k):
                g.put(g.clients[0], [item(4, text("b"), origin=g.last)], 1)
            docs.append(g.ups)
    return docs


@gpu
def test_info_bytes_and_origins_of_another_id_length(engs):
    docs = _info_docs()
    check(engs, "infos", docs, lean=len(docs))


# ======================================================================= shapes
def _ds_docs():
    docs = []
    for c, dc in ((F5[0], F5[0]), (F5[1], F4[0]), (F5[2], 77)):       # the delete set names a client of any id length
        for where in ("first", "last", "between", "most"):
            g = Log([c], seed=len(docs))
            k = 8
            for i in range(k):
                dso = {"first": i == 0, "last": i == k - 1, "between": i in (2, 3, 5), "most": i != 4}[where]
                if dso:
                    g.raw(_ds_only(dc, i))
                else:
                    g.put(c, [item(4, text("d"), origin=g.last)], 1)
            docs.append(g.ups)
    return docs


@gpu
def test_delete_set_only_updates_take_no_part(engs):
    docs = _ds_docs()
    check(engs, "dsonly", docs, lean=len(docs))


def _mixed_row_docs():
    """A multi-character insert (the generic grammar's shape) in one lane of each row: update 4 l + q for l = 0, 1, 2."""
    docs = []
    for k in (8, 12):
        for at in range(k):
            g = Log([F5[at % 6], F5[(at + 1) % 6]], seed=at)
            for i in range(k):
                c = g.clients[i % 2]
                if i == at:
                    g.put(c, [item(4, text("multi"), origin=g.last)], 5)
                else:
                    g.put(c, [item(4, text("s"), origin=g.last)], 1)
            docs.append(g.ups)
    return docs


@gpu
def test_rows_with_fast_and_other_lanes_mixed(engs):
    docs = _mixed_row_docs()
    check(engs, "mixed", docs, lean=len(docs))


def _long_docs(k):
    """64 documents of k updates: 1 to 4 five-byte clients, every fourth document with one four-byte client among them
    (at a lane and row that moves with the document), and -- k = 200 -- every eighth with a fifth client."""
    docs = []
    for d in range(64):
        ncl = 1 + d % 4
        cl = [F5[(d + j) % 6] for j in range(ncl)]
        if k == 200 and d % 8 == 7:
            cl = F5[:5]
        if d % 4 == 2:
            cl[-1] = F4[d % 4]
        at = (d * 37) % k
        order = (lambda i, n=len(cl), at=at: n - 1 if i == at else i % max(1, n - 1)) if d % 4 == 2 else None
        # (255 updates fit the narrow kernel's staging with an origin alone: 20 bytes an update at the most)
        docs.append(log_doc(k, cl, order=order, infos=("o", "o", "b") if k == 200 else ("o",), seed=d))
    assert max(sum(map(len, us)) for us in docs) <= 5100
    return docs


@gpu
@pytest.mark.parametrize("k", [200, 255])
def test_long_documents(engs, k):
    docs = _long_docs(k)
    check(engs, "long%d" % k, docs, lean=len(docs), wide=0)   # (the narrow kernel's documents: none goes on to the wide one)


# ======================================================================= the extraction, on the CPU
def test_idlen_check_program(tmp_path):
    """tools/idlen_check.cpp (the specialised client / clock / info extraction against the generic one), its quick
    pass: built and run, no mismatch."""
    exe = str(tmp_path / "idlen_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "tools", "idlen_check.cpp")])
    out = subprocess.run([exe, "--quick"], capture_output=True, text=True)
    assert out.returncode == 0 and '"mismatches": 0' in out.stdout, out.stdout + out.stderr

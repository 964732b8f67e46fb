"""The lean merge kernels' corpora checked on the CPU, against the oracle alone: the slow-class corpora
(lean_slowclass_docs.py) and the chunk-mask corpora (lean_chunkmask_docs.py) hold what their builders say, and the
census of each is printed.  The GPU runs are test_lean_slowclass.py and test_lean_chunkmask.py."""
import lean_chunkmask_docs as cm
import lean_slowclass_docs as sc
import oracle
from devrun import Memo
from v1util import vu

MEMO = Memo()
memo = MEMO.get


# ======================================================================= the slow-class corpora against the oracle
def test_corpora_against_the_oracle(capsys):
    rows = []
    for key, fn in sc.CORPORA:
        c = memo(key + "_cpu", fn)
        exp = memo("exp_" + key + "_cpu", lambda: [oracle.merge_updates(us) for us in c.docs])
        for d, us in enumerate(c.docs):
            assert key == "b255" or 2 <= len(us) <= 40, (key, d, len(us))
            if c.kind[d] == "lean":
                assert exp[d][0] == 0, (key, d, exp[d][0], [u.hex() for u in us][:6])
                assert all(len(u) <= 32 for u in us), (key, d)
        rows.append((key, len(c.docs), sum(k == "lean" for k in c.kind), sum(k == "bad" for k in c.kind),
                     sum(st == 0 for st, _ in exp)))
    # the census of the copy corpora: offsets and widths
    _, cover = sc._every_length_corpus()
    assert sorted(cover) == list(range(sc.SB_MIN, sc.SB_MAX + 1)) and all(len(v) == 16 for v in cover.values())
    _, widest = sc._width_corpus()
    assert all((w, s) in widest for w in (20, 21, 24, 25) for s in (False, True))
    _, heads = sc._packed_corpus()
    assert heads >= {(s, h) for s in (4, 5, 6) for h in range(4)}
    # a document's merged block is what `placements` says: the first struct of a checked document sits where it puts it
    us = sc.struct_doc([9, 14, "e", 5, 23])
    st, out = oracle.merge_updates(us)
    assert st == 0
    t = 1 + 1 + len(vu(sc.A)) + len(vu(3))
    for (n, h, _), u in zip(sc.placements(us, 0), [u for u in us if u[0]]):
        assert h == t & 3 and out[t:t + n] == u[4:4 + n], (n, h, t)
        t += n
    with capsys.disabled():
        print("\nslow-class corpora: documents / lean / never lean / merged by the oracle")
        for r in rows:
            print("  %-8s %4d / %4d / %3d / %4d" % r)


# ======================================================================= the chunk-mask corpus builder's census
def clean_ok(key, corpus):
    exp = MEMO.expect(key, corpus.docs)
    return all(exp[d][0] == 0 for d in range(len(corpus.docs)) if corpus.kind[d] != "bad")


def test_census_of_the_corpora(capsys):
    a = memo("align", cm._align_corpus)
    assert a.bit_offsets() == set(range(32))
    n, pos = memo("nonmin", cm._nonmin_corpus)
    splits = {f: sorted({p & 15 for p in ps}) for f, ps in pos.items()}
    assert all(s == list(range(16)) for s in splits.values())          # 15: the pair lies across a chunk edge
    assert all(1023 in pos[f] for f in cm.FIELDS)
    g = memo("neigh", cm._neighbour_corpus)
    k = memo("cap", cm._cap_corpus)
    w = memo("width", cm._width_corpus)
    for key, c in (("align", a), ("nonmin", n), ("neigh", g), ("cap", k), ("width", w)):
        assert clean_ok(key, c), key
        assert all(len(u) <= 32 for d, us in enumerate(c.docs) if c.kind[d] != "bad" for u in us)
    pool, lean = memo("reuse_pool", cm._reuse_pool)
    exp = memo("reuse_exp", lambda: [[oracle.merge_updates(us) for us in row] for row in pool])
    assert all(st == 0 for row in exp for st, _ in row)
    with capsys.disabled():
        print("\nchunk-mask corpora: documents / clean / bit offsets of update starts")
        for key, c in (("align", a), ("nonmin", n), ("neigh", g), ("cap", k), ("width", w)):
            print("  %-7s %4d / %4d / %d of 32" % (key, len(c.docs), c.lean(), len(c.bit_offsets())))
        print("  pair positions mod 16 per field:", {f: len(s) for f, s in splits.items()}, "and staged byte 1023 in",
              [f for f in cm.FIELDS if 1023 in pos[f]])

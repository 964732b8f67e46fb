"""The narrow lean merge kernel on the corpora of lean_chunkmask_docs.py (alignment, non-minimal varuints, neighbours,
capacity, widths, reuse: each laid out in one arena with every document's residue chosen; what they hold and why is
told there).  Every expectation is the CPU oracle's, in both input forms, with the count of documents the lean kernels
finished: a clean document is never deferred, a document with a non-minimal varuint is never taken.  The tests describe
behaviour, not the kernel.  The census of the corpora is taken on the CPU in test_lean_docs.py."""
import pytest

import lean_chunkmask_docs as g
import oracle
from devrun import Memo, engine_fixture, run_merge, same
from lean_chunkmask_docs import CAP_FILL, FIELDS, K_CAP, POOL

gpu = pytest.mark.gpu
FORMS = ["off", "lens"]

eng = engine_fixture()
MEMO = Memo()
memo = MEMO.get


def expect(key, corpus):
    """The oracle's results of a corpus, computed once and shared."""
    return MEMO.expect(key, corpus.docs)


def check(e, key, corpus):
    """Both input forms: exact against the oracle; the lean kernels finish the clean documents and no other."""
    exp = expect(key, corpus)
    for form in FORMS:
        res, took = run_merge(e, corpus.docs, form)
        bad = [d for d in range(len(corpus.docs)) if not same(exp[d], res[d])]
        assert not bad, (key, form, len(bad), bad[:5], corpus.kind[bad[0]], corpus.b0[bad[0]] % 16,
                         [u.hex() for u in corpus.docs[bad[0]]][:8])
        assert took == corpus.lean(), (key, form, took, corpus.lean())


def clean_ok(key, corpus):
    exp = expect(key, corpus)
    return all(exp[d][0] == 0 for d in range(len(corpus.docs)) if corpus.kind[d] != "bad")


# ======================================================================= alignment
@gpu
def test_clean_documents_at_every_residue(eng):
    c = memo("align", g._align_corpus)
    assert {c.b0[d] % 16 for d in range(len(c.docs)) if c.kind[d] == "clean"} == set(range(16))
    assert c.bit_offsets() == set(range(32))
    assert clean_ok("align", c)
    check(eng, "align", c)


# ======================================================================= non-minimal varuints
@gpu
def test_non_minimal_varuints_at_every_chunk_offset(eng):
    c, pos = memo("nonmin", g._nonmin_corpus)
    for f in FIELDS:
        assert {p & 15 for p in pos[f]} == set(range(16)) and 1023 in pos[f], (f, pos[f])
    assert {p & 15 for p in pos["run"]} == set(range(16))
    assert clean_ok("nonmin", c)
    check(eng, "nonmin", c)


# ======================================================================= neighbours
@gpu
def test_neighbouring_bytes_change_nothing(eng):
    c = memo("neigh", g._neighbour_corpus)
    assert clean_ok("neigh", c)
    check(eng, "neigh", c)


# ======================================================================= capacity
@gpu
def test_documents_that_fill_the_staged_buffer(eng):
    c = memo("cap", g._cap_corpus)
    full = [(c.b0[d] % 16) + sum(map(len, c.docs[d])) for d in range(len(c.docs)) if len(c.docs[d]) == K_CAP]
    assert sorted(set(full)) == sorted(CAP_FILL) and len(full) == 9
    assert clean_ok("cap", c)
    check(eng, "cap", c)


# ======================================================================= struct widths around the copy classes
@gpu
def test_struct_widths_around_the_copy_classes(eng):
    c = memo("width", g._width_corpus)
    assert clean_ok("width", c)
    check(eng, "width", c)


# ======================================================================= reuse: one wave, document after document
def _reuse_corpus(grid):
    """Document d is wave d % grid's document number d // grid: long, short, slow row, long, ..."""
    pool, lean = memo("reuse_pool", g._reuse_pool)
    exp = memo("reuse_exp", lambda: [[oracle.merge_updates(us) for us in row] for row in pool])
    n = 3 * grid + grid // 2 + 3
    pick = [((d // grid) % 3, (d + d // grid) % POOL) for d in range(n)]
    return [pool[k][j] for k, j in pick], [exp[k][j] for k, j in pick], sum(lean[k][j] for k, j in pick)


@gpu
def test_one_wave_per_cu_long_short_slow(eng, monkeypatch):
    import torch
    grid = torch.cuda.get_device_properties(0).multi_processor_count
    monkeypatch.setenv("YGM_LEAN_WAVES_PER_CU", "1")
    docs, exp, lean = _reuse_corpus(grid)
    assert len(docs) > 3 * grid and all(st == 0 for st, _ in exp)
    for form in FORMS:
        res, took = run_merge(eng, docs, form)
        bad = [d for d in range(len(docs)) if not same(exp[d], res[d])]
        assert not bad, (form, len(bad), bad[:5])
        assert took == lean, (form, took, lean)

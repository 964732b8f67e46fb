"""The narrow lean merge kernel on the corpora of lean_slowclass_docs.py (varuint values, struct copies, vote and
placement: what they hold and why is told there).  Every expectation is the CPU oracle's, in both input forms, with the
count of documents the lean kernels finished: a document marked "lean" is never deferred, one marked "bad" is never
taken.  The tests describe behaviour, not the kernel.  The corpora themselves are checked on the CPU in
test_lean_docs.py."""
import pytest

import lean_slowclass_docs as g
from devrun import Memo, engine_fixture, run_merge, same
from lean_slowclass_docs import SB_MAX, SB_MIN, Corpus
from v1util import vu

gpu = pytest.mark.gpu
FORMS = ["off", "lens"]

eng = engine_fixture()
MEMO = Memo()
memo = MEMO.get


def expect(key, corpus):
    """The oracle's results of a corpus, computed once and shared."""
    return MEMO.expect(key, corpus.docs)


def check(e, key, corpus):
    """Both input forms: exact against the oracle; the lean kernels finish the 'lean' documents and no other."""
    exp = expect(key, corpus)
    for form in FORMS:
        res, took = run_merge(e, corpus.docs, form)
        bad = [d for d in range(len(corpus.docs)) if not same(exp[d], res[d])]
        assert not bad, (key, form, len(bad), bad[:5], corpus.kind[bad[0]], [u.hex() for u in corpus.docs[bad[0]]][:8])
        if corpus.lean() is not None:
            assert took == corpus.lean(), (key, form, took, corpus.lean())


def lean_ok(key, corpus):
    """The oracle merges every 'lean' document, and each is inside the narrow kernel's 32-byte updates."""
    exp = expect(key, corpus)
    return all(exp[d][0] == 0 and all(len(u) <= 32 for u in corpus.docs[d])
               for d in range(len(corpus.docs)) if corpus.kind[d] == "lean")


# ======================================================================= varuints
@gpu
def test_client_and_clock_on_both_sides_of_every_length(eng):
    c = memo("clck", g._client_clock_corpus)
    assert lean_ok("clck", c)
    check(eng, "clck", c)
    lean = Corpus()                # the documents that make a claim, alone: with their count
    for d, us in enumerate(c.docs):
        if c.kind[d] == "lean":
            lean.add(us)
    check(eng, "clck_lean", lean)


@gpu
def test_the_byte_after_a_varuint_does_not_leak(eng):
    c = memo("next", g._next_byte_corpus)
    assert lean_ok("next", c)
    firsts = {u[2 + len(vu(cl)):][:1] for cl in (1,) for us in c.docs[:4] for u in us}
    assert {b"\x7f", b"\x80", b"\xff"} <= firsts
    check(eng, "next", c)


@gpu
def test_a_fifth_byte_past_uint32_is_never_taken(eng):
    c = memo("fifth", g._fifth_byte_corpus)
    assert lean_ok("fifth", c)
    check(eng, "fifth", c)


@gpu
def test_client_zero_is_exact(eng):
    check(eng, "zero", memo("zero", g._client_zero_corpus))


@gpu
def test_values_in_origins_and_in_the_generic_parse(eng):
    c = memo("origin", g._origin_corpus)
    assert lean_ok("origin", c)
    check(eng, "origin", c)


@gpu
def test_delete_set_values_fast_path_and_cursor_walk(eng):
    c = memo("ds", g._ds_corpus)
    assert lean_ok("ds", c)
    check(eng, "ds", c)


# ======================================================================= copies
@gpu
def test_structs_of_every_length_at_every_offset(eng):
    c, cover = memo("lengths", g._every_length_corpus)
    assert all(len(cover[sb]) == 16 for sb in range(SB_MIN, SB_MAX + 1))
    assert lean_ok("lengths", c)
    check(eng, "lengths", c)


@gpu
def test_documents_on_both_sides_of_the_copy_widths(eng):
    c, widest = memo("widths", g._width_corpus)
    for w in (20, 21, 24, 25):
        assert (w, False) in widest and (w, True) in widest, (w, sorted(widest))
    assert lean_ok("widths", c)
    check(eng, "widths", c)


@gpu
def test_short_structs_packed_between_long_ones(eng):
    c, heads = memo("packed", g._packed_corpus)
    assert heads >= {(s, h) for s in (4, 5, 6) for h in range(4)}, sorted(heads)
    assert lean_ok("packed", c)
    check(eng, "packed", c)


@gpu
def test_appends_and_mid_text_inserts_mixed(eng):
    c = memo("mixed", g._mixed_shape_corpus)
    assert lean_ok("mixed", c)
    check(eng, "mixed", c)


# ======================================================================= vote and placement
@gpu
def test_one_to_five_clients_in_every_order_of_first_sight(eng):
    c = memo("order", g._order_corpus)
    assert len(c.docs) == 2 * (1 + 2 + 6 + 24 + 120)
    assert lean_ok("order", c)
    check(eng, "order", c)


@gpu
def test_ids_that_differ_in_the_top_bit_or_the_fifth_byte(eng):
    c = memo("near", g._near_id_corpus)
    assert lean_ok("near", c)
    check(eng, "near", c)


@gpu
def test_a_client_named_only_by_a_delete_set(eng):
    c = memo("ghost", g._deletion_client_corpus)
    assert lean_ok("ghost", c)
    check(eng, "ghost", c)


@gpu
def test_a_block_of_255_records(eng):
    c = memo("b255", g._block255_corpus)
    assert lean_ok("b255", c)
    check(eng, "b255", c)


@gpu
def test_a_gap_and_an_overlap_in_the_block_of_every_rank(eng):
    c = memo("fault", g._fault_corpus)
    assert lean_ok("fault", c)
    check(eng, "fault", c)

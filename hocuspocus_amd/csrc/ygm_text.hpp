// ygm_text.hpp -- the plain text of a stored document (ygm_text_v1):
//
//     YGM_TEXT_FLAT   utf8(doc.getText(name).toString())       doc = Y.applyUpdate(new Y.Doc(), state)
//     YGM_TEXT_DEEP   the same walk, descending into nested types (XmlFragment / Tiptap documents)
//
// Restated from yjs 13.5.16 (YText.toString, Y@ types/YText: from _start along right, every item that is not deleted,
// is countable and holds a ContentString appends its string).  The deep walk descends at a live ContentType item into
// that type's list and, on return, appends one 0x0A unless the output is still empty or already ends in 0x0A; map
// entries (items with a parentSub) are on no list, so attributes and Y.Map values contribute nothing.
//
// The text of a type is its integrated list minus deleted items, which is what the snapshot's first three stages
// build: parse, integrate_all, apply_ds of snap::Doc (ygm_snapshot.hpp) and of snapt::TDoc (ygm_snap_text.hpp).  GC,
// the merge pass and the encoder are not run: a deleted item is skipped whether or not its content was collected,
// and merged items spell the same string as their parts.  So the text depends neither on F_COMPAT_135 nor on
// F_SNAP_NOGC.  This header adds the last stage for both tiers:
//   flat tier    (TDoc, LDS): flat_prepare -- the asked name against the update's single root name, the list
//                linearised into sq[]; the wave-wide copy is k_text_flat's (ygm_text.hip), flat_emit_seq its
//                sequential twin for the host harness (tools/snapdev/textdev.cpp)
//   general tier (Doc, global workspace; carve, Doc::load and find_root are the snapshot's): emit_text -- the walk
//                with an explicit stack in Doc::st
#pragma once
#include "ygm_snapshot.hpp"
#include "ygm_snap_text.hpp"

namespace ygm {
namespace text {

constexpr uint32_t MODE_FLAT = 0u, MODE_DEEP = 1u;   // YGM_TEXT_FLAT / YGM_TEXT_DEEP

// ------------------------------------------------------------------ flat tier
// the part capacity of a workspace of ws_bytes, and where the parts and their sequence array lie: the layout
// snapt::snapshot_text gives its TDoc, so the envelope (what fits) is k_snap_text's at the same LDS size
YDEV uint32_t flat_cap(uint32_t ws_bytes) {
  const uint32_t c = (ws_bytes - snapt::ws_fixed()) / snapt::part_bytes();
  return c > 0xFFF0u ? 0xFFF0u : c;
}
YDEV snapt::P* flat_parts(uint8_t* ws) { return (snapt::P*)(ws + snapt::ws_fixed()); }
YDEV uint16_t* flat_seq(uint8_t* ws, uint32_t ws_bytes) {
  return (uint16_t*)(ws + snapt::ws_fixed() + flat_cap(ws_bytes) * (uint32_t)sizeof(snapt::P));
}
YDEV bool flat_init(snapt::TDoc& D, const uint8_t* in, uint32_t n, uint32_t flags, uint8_t* ws, uint32_t ws_bytes) {
  if (n >= 0xFFFFu || ws_bytes < snapt::ws_fixed() + 16u * snapt::part_bytes()) return false;
  D.sh = (uint32_t)((uintptr_t)in & 3u); D.w32 = (snapt::InW)(in - D.sh); D.n = n; D.flags = flags;
  D.ct = (snapt::CT*)ws; D.ord = ws + snapt::CMAX * sizeof(snapt::CT); D.nc = 0;
  D.cap = flat_cap(ws_bytes);
  D.p = flat_parts(ws); D.np = 0;
  D.sq = flat_seq(ws, ws_bytes);
  D.name_off = D.name_len = 0; D.ds_pos = 0; D.epoch = 0; D.n_ins = 0; D.start = snapt::NIL; D.have_name = false; D.bad = false;
  return true;
}
// parse, integrate, delete; then the asked name against the update's root name and the list (start, right) into
// sq[].  Returns the number of list parts, or -1: outside the envelope, another name, or a list that does not end
// within np steps (the general tier takes the document and decides its status).
YDEV int32_t flat_prepare(snapt::TDoc& D, const uint8_t* name, uint32_t name_len) {
  D.parse();
  if (!D.bad) D.integrate_all();
  if (!D.bad) D.apply_ds();
  if (D.bad || !D.have_name || D.name_len != name_len) return -1;
  for (uint32_t i = 0; i < name_len; i++) if (D.at(D.name_off + i) != name[i]) return -1;
  uint32_t m = 0;
  for (uint16_t x = D.start; x != snapt::NIL; x = D.p[x].right) {
    if (m >= D.np) return -1;
    D.sq[m++] = x;
  }
  return (int32_t)m;
}
YDEV bool flat_live(uint8_t fl) { return (fl & (snapt::T_STR | snapt::T_DEL)) == snapt::T_STR; }
// the sequential emit (the host twin of k_text_flat's wave-wide copy): live parts' slices in list order
template <class O>
YDEV void flat_emit_seq(const snapt::TDoc& D, uint32_t cnt, O& o) {
  for (uint32_t i = 0; i < cnt; i++) {
    const snapt::P u = D.p[D.sq[i]];
    if (flat_live(u.fl)) D.copy_in(o, u.coff, u.len);
  }
}

// ------------------------------------------------------------------ general tier
// The walk.  Capacity: the string pieces are disjoint slices of the input (<= n bytes together); a split through a
// surrogate pair drops the pair's 4 bytes and adds a U+FFFD on each side (6 bytes: <= 3 more per split, and splits
// are parts beyond the S input structs, < it); one 0x0A at most per type returned from (<= ty = S + 2 <= it).  So
//     text bytes <= n + 3 it + ty <= n + 4 it < n + 48 it + 16 cl + 64 = Caps::out,
// the workspace's output region as caps_of sizes it (OutCap still stops at the cap: more is ST_NOMEM).
// Every loop is bounded: the walk visits each list item once and returns from each type once in a well-formed
// document, n_it + n_ty steps at most; a piece chain has at most n_pc pieces.  A list that cycles (a broken
// document) exhausts the bound and ends in ST_UNSUP.
YDEV void emit_text(snap::Doc& D, const uint8_t* name, uint32_t name_len, uint32_t mode, snap::OutCap& o) {
  using namespace snap;
  const int32_t root = find_root(D, name, name_len);
  if (root < 0) return;   // doc.getText(name) of a name the update has no root for: an empty type
  const uint64_t limit = (uint64_t)D.n_it + D.n_ty + 1u;
  uint64_t steps = 0;
  uint32_t sp = 0;
  uint8_t last = 0;
  int32_t x = D.ty[root].start;
  for (;;) {
    if (++steps > limit) { D.fail(ST_UNSUP); return; }   // (items + returns + the final end of the root's list)
    if (x < 0) {
      if (!sp) return;
      x = D.it[D.st[--sp]].right;   // back in the parent's list, after the type's item
      if (o.n && last != 0x0A) { o.b(0x0A); last = 0x0A; }
      continue;
    }
    const SI& u = D.it[x];
    if (u.kind == SK_ITEM && !(u.flags & F_DEL)) {
      if (u.ref == 4) {
        uint32_t np = 0;
        for (int32_t p = u.p0; p >= 0; p = D.pc[p].next) {
          if (++np > D.n_pc) { D.fail(ST_UNSUP); return; }
          const Piece q = D.pc[p];
          if (q.pre) { o.b(0xEF); o.b(0xBF); o.b(0xBD); last = 0xBD; }
          if (q.end > q.off) { o.copy(D.in + q.off, q.end - q.off); last = D.in[q.end - 1]; }
          if (q.post) { o.b(0xEF); o.b(0xBF); o.b(0xBD); last = 0xBD; }
        }
      } else if (u.ref == 7 && mode == MODE_DEEP && u.type >= 0) {
        if (sp >= D.cap_st) { D.fail(ST_NOMEM); return; }
        D.st[sp++] = x;
        x = D.ty[u.type].start;
        continue;
      }
    }
    x = u.right;
  }
}

// the text of root `name` of in[0, n) over a workspace carved from ws, at most out_cap bytes at out.  A document
// that leaves pending structs / a pending delete set is read through its integrated part (ST_OK).
YDEV_NI int text_run(const uint8_t* in, uint32_t n, uint32_t flags, uint8_t* ws, const snap::Caps& k, const uint8_t* name,
                     uint32_t name_len, uint32_t mode, uint8_t* out, uint32_t out_cap, uint32_t& out_len) {
  snap::Doc D;
  snap::carve(D, in, n, flags, ws, k, out, out_cap);
  out_len = 0;
  D.load();
  if (D.err) return D.err;
  snap::OutCap o{out, 0, out_cap};
  emit_text(D, name, name_len, mode, o);
  if (D.err) return D.err;
  if (o.n > o.cap) return ST_NOMEM;
  out_len = o.n;
  return ST_OK;
}
// document d's workspace from caps_of, its output region at the end (as snap::snapshot_doc)
YDEV int text_doc(const uint8_t* in, uint32_t n, uint32_t flags, uint8_t* ws, const snap::Caps& k, const uint8_t* name, uint32_t name_len,
                  uint32_t mode, uint32_t& out_off, uint32_t& out_len) {
  out_off = (uint32_t)snap::ws_core_bytes(k);
  return text_run(in, n, flags, ws, k, name, name_len, mode, ws + out_off, k.out, out_len);
}

}  // namespace text
}  // namespace ygm

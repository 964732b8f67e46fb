// ygm_tojson.hpp -- toJSON of a stored document's Map, Array or Text root (ygm_tojson_v1):
//
//     utf8(JSON.stringify(doc.getMap(name).toJSON()))     YGM_TOJSON_MAP      doc = Y.applyUpdate(new Y.Doc(), state)
//     utf8(JSON.stringify(doc.getArray(name).toJSON()))   YGM_TOJSON_ARRAY
//     utf8(JSON.stringify(doc.getText(name).toJSON()))    YGM_TOJSON_TEXT
//
// Restated from yjs 13.5.16 (YMap.toJSON, YArray.toJSON, YText.toJSON = toString):
//   Map    the type's map entries whose current item is not deleted; the value is the last element of the item's
//          content, a nested type its own toJSON.  Keys follow JavaScript's own-property order of the map[key] = v
//          assignments made in _map order: canonical array-index keys ascending, then the order the type's me[]
//          entries were created in (Walk::attrs' rule).  An undefined value drops its key.  List items are ignored.
//   Array  the list's live countable items, every content element in turn (undefined: null); map entries are ignored.
//   Text   YGM_TEXT_FLAT's walk (live ContentStrings, U+FFFD on both sides of a cut surrogate pair) as one JSON string.
// The asked kind decides how the root is read; a nested type is read by its typeRef (0 Array, 1 Map, 2 Text).  Any
// values are written by v2::any_json's TOJSON form, ContentJSON elements (canonical JSON text in V1) are copied, the
// word `undefined` counting as undefined.  The refusals (ST_UNSUP / ST_NONCANON / ST_MALFORMED) are include/ygm.h's
// table.  Like the text and the ProseMirror JSON this is a last stage over Doc::load: no gc, no merge pass, no encoder.
//
// The walk's stack is Doc::st.  A Map being written keeps a frame there: its live entries in output order, their count
// and the index of the next one; an Array keeps nothing while it is current.  Descending into a nested type pushes
// what the parent needs to go on (an Array: the ContentType item and T_ARR; a Map: T_MAP above its frame).
// Output size: a string of control characters grows sixfold, so the JSON is not bounded by Caps::out.  OutCap counts
// past its cap: tojson_run reports the needed length (ST_JSON_MORE) and the caller runs the document again into a
// region of that size (k_tojson's second launch; tools/snapdev/tojsondev.cpp).
#pragma once
#include "ygm_json.hpp"

namespace ygm {
namespace tojson {

constexpr uint32_t KIND_MAP = 0u, KIND_ARRAY = 1u, KIND_TEXT = 2u;   // YGM_TOJSON_MAP / _ARRAY / _TEXT
constexpr int32_t T_ARR = 0, T_MAP = 1;

using json::lit;
using json::quoted;
using json::JSON_MAX;
using json::ST_JSON_MORE;

// is s[0, n) the 9-byte word w ("undefined", "__proto__")?
YDEV bool is_word(const uint8_t* s, uint32_t n, const char* w) {
  if (n != 9) return false;
  for (uint32_t i = 0; i < 9; i++) if (s[i] != (uint8_t)w[i]) return false;
  return true;
}

// toString of type t as one JSON string: live countable ContentStrings along the list (text::emit_text's flat walk)
YDEV void emit_string(snap::Doc& D, int32_t t, snap::OutCap& o, uint64_t& steps, uint64_t limit) {
  using namespace snap;
  o.b('"');
  for (int32_t x = t < 0 ? -1 : D.ty[t].start; x >= 0; x = D.it[x].right) {
    if (++steps > limit) { D.fail(ST_UNSUP); return; }
    const SI& u = D.it[x];
    if (u.kind != SK_ITEM || (u.flags & F_DEL) || u.ref != 4) continue;
    uint32_t np = 0;
    for (int32_t p = u.p0; p >= 0; p = D.pc[p].next) {
      if (++np > D.n_pc) { D.fail(ST_UNSUP); return; }
      const Piece q = D.pc[p];
      if (q.pre) { o.b(0xEF); o.b(0xBF); o.b(0xBD); }
      if (q.end > q.off) json::esc(o, D.in + q.off, q.end - q.off);
      if (q.post) { o.b(0xEF); o.b(0xBF); o.b(0xBD); }
      if (o.n >= JSON_MAX) { D.fail(ST_NOMEM); return; }
    }
  }
  o.b('"');
}

// one ContentJSON element (a varString of JSON text) at c; undef: the word `undefined` (nothing is written).
// FLOATS (a context opened with YGM_F_FLOATS; a compile-time option as json::Walk's): the text is copied without the
// float refusal -- its numbers are canonical by the state's parse -- and Any values take any_json's FLOATS form.
template <bool FLOATS = false>
YDEV void json_elem(snap::Doc& D, Cur& c, snap::OutCap& o, bool& undef) {
  uint32_t vl; const uint32_t vo = c.buf(vl);
  undef = false;
  if (c.err) { D.fail(ST_MALFORMED); return; }
  if (is_word(D.in + vo, vl, "undefined")) { undef = true; return; }
  if (!FLOATS && json::json_has_float(D.in + vo, vl)) { D.fail(ST_NONCANON); return; }
  o.copy(D.in + vo, vl);
}

// the live entries of Map type t as a frame on the stack at sp: [entries in output order (k) | k | next = 0]; sp then
// stands above it.  The entries are collected newest first (the type's list), turned oldest first, and the index keys
// moved to the front in ascending order (through the free stack above: only when there is one).
YDEV void map_frame(snap::Doc& D, int32_t t, uint32_t& sp) {
  using namespace snap;
  const uint32_t b = sp;
  uint32_t k = 0, m = 0, steps = 0;
  for (int32_t e = D.ty[t].map; e >= 0; e = D.me[e].next) {
    if (++steps > D.n_me) { D.fail(ST_UNSUP); return; }
    const int32_t x = D.me[e].item;
    if (x < 0 || D.deleted(x)) continue;
    if (b + k + 2u >= D.cap_st) { D.fail(ST_NOMEM); return; }
    D.st[b + k++] = e;
    uint64_t v;
    if (index_key(D.in + D.me[e].key_off, D.me[e].key_len, v)) m++;
  }
  for (uint32_t i = 0, j = k; i + 1 < j; i++) { j--; const int32_t s = D.st[b + i]; D.st[b + i] = D.st[b + j]; D.st[b + j] = s; }
  if (m) {
    if ((uint64_t)b + 2ull * k + 2u >= D.cap_st) { D.fail(ST_NOMEM); return; }
    uint32_t ni = 0, nr = 0;
    for (uint32_t i = 0; i < k; i++) {
      const int32_t e = D.st[b + i];
      uint64_t v;
      if (index_key(D.in + D.me[e].key_off, D.me[e].key_len, v)) D.st[b + k + ni++] = e; else D.st[b + nr++] = e;
    }
    for (uint32_t i = nr; i-- > 0;) D.st[b + m + i] = D.st[b + i];
    for (uint32_t i = 0; i < m; i++) {   // insertion sort by index value (yjs writes most maps in ascending order)
      const int32_t e = D.st[b + k + i];
      uint64_t v = 0, w = 0;
      index_key(D.in + D.me[e].key_off, D.me[e].key_len, v);
      uint32_t j = i;
      while (j > 0) {
        const int32_t f = D.st[b + j - 1];
        index_key(D.in + D.me[f].key_off, D.me[f].key_len, w);
        if (w <= v) break;
        D.st[b + j] = f; j--;
      }
      D.st[b + j] = e;
    }
  }
  D.st[b + k] = (int32_t)k; D.st[b + k + 1] = 0;
  sp = b + k + 2u;
}

// The walk.  Every loop is bounded as emit_root's: each list item is visited once, each map entry written once and
// each type returned from once in a well-formed document; a list that cycles exhausts the bound and ends in ST_UNSUP.
template <bool FLOATS = false>
YDEV void emit_tojson(snap::Doc& D, const uint8_t* name, uint32_t name_len, uint32_t kind, snap::OutCap& o) {
  using namespace snap;
  const int32_t root = find_root(D, name, name_len);
  const uint64_t limit = 2ull * D.n_it + 2ull * D.n_ty + D.n_me + 4u;
  uint64_t steps = 0;
  if (kind == KIND_TEXT) { emit_string(D, root, o, steps, limit); return; }
  if (root < 0) { lit(o, kind == KIND_MAP ? "{}" : "[]"); return; }
  uint32_t sp = 0;
  bool in_map = kind == KIND_MAP;   // the type being written
  bool has = false;                 // it has an entry already
  int32_t x = -1;                   // Array: the next list item
  if (in_map) { o.b('{'); map_frame(D, root, sp); } else { o.b('['); x = D.ty[root].start; }
  for (;;) {
    if (++steps > limit) { D.fail(ST_UNSUP); return; }
    if (D.err) return;
    if (o.n >= JSON_MAX) { D.fail(ST_NOMEM); return; }
    int32_t child = -1;   // a ContentType item to write next
    if (in_map) {
      const uint32_t k = (uint32_t)D.st[sp - 2u], i = (uint32_t)D.st[sp - 1u];
      if (i < k) {
        D.st[sp - 1u] = (int32_t)(i + 1u);
        const MapEnt& e = D.me[D.st[sp - 2u - k + i]];
        const SI& u = D.it[e.item];
        if (u.kind != SK_ITEM || (u.ref != 8 && u.ref != 2 && u.ref != 7)) { D.fail(ST_UNSUP); return; }
        if (is_word(D.in + e.key_off, e.key_len, "__proto__")) { D.fail(ST_UNSUP); return; }
        if (u.ref == 7) {
          if (has) o.b(',');
          has = true;
          quoted(o, D.in + e.key_off, e.key_len); o.b(':');
          child = e.item;
        } else {
          if (u.p1 < 0) { D.fail(ST_UNSUP); return; }
          const Piece q = D.pc[u.p1];
          Cur c{D.in, q.off, q.end, 0, 0};
          for (uint32_t j = 1; j < q.cnt && !c.err; j++) { if (u.ref == 2) { uint32_t l; c.buf(l); } else any_skip(c); }
          if (c.err || c.pos >= c.end) { D.fail(ST_MALFORMED); return; }
          bool undef = u.ref == 8 ? D.in[c.pos] == 127 : false;
          if (u.ref == 2) { Cur p = c; uint32_t vl; const uint32_t vo = p.buf(vl); undef = !p.err && is_word(D.in + vo, vl, "undefined"); }
          if (undef) continue;
          if (has) o.b(',');
          has = true;
          quoted(o, D.in + e.key_off, e.key_len); o.b(':');
          if (u.ref == 8) { const int r = v2::any_json<OutCap, true, FLOATS>(c, o); if (r) { D.fail(r); return; } }
          else json_elem<FLOATS>(D, c, o, undef);
          continue;
        }
      }
    } else if (x >= 0) {
      const SI& u = D.it[x];
      const int32_t cur = x;
      x = u.right;
      if (u.kind != SK_ITEM || (u.flags & F_DEL) || u.ref == 6) continue;   // (a format is not countable)
      if (u.ref == 7) {
        if (has) o.b(',');
        has = true;
        child = cur;
      } else if (u.ref == 8 || u.ref == 2) {
        uint32_t np = 0;
        for (int32_t p = u.p0; p >= 0; p = D.pc[p].next) {
          if (++np > D.n_pc) { D.fail(ST_UNSUP); return; }
          const Piece q = D.pc[p];
          Cur c{D.in, q.off, q.end, 0, 0};
          for (uint32_t j = 0; j < q.cnt; j++) {
            if (has) o.b(',');
            has = true;
            if (u.ref == 8) { const int r = v2::any_json<OutCap, true, FLOATS>(c, o); if (r) { D.fail(r); return; } }
            else { bool undef; json_elem<FLOATS>(D, c, o, undef); if (undef) lit(o, "null"); }
            if (c.err) { D.fail(ST_MALFORMED); return; }
            if (D.err) return;
            if (o.n >= JSON_MAX) { D.fail(ST_NOMEM); return; }
          }
        }
        continue;
      } else { D.fail(ST_UNSUP); return; }   // a string, an embed, binary content, a sub-document
    }
    if (child >= 0) {   // the nested type, by its typeRef
      const SI& u = D.it[child];
      if (u.type < 0 || u.c_start >= u.c_end) { D.fail(ST_UNSUP); return; }
      const uint8_t tref = D.in[u.c_start];
      if (tref == 2) { emit_string(D, u.type, o, steps, limit); continue; }
      if (tref > 2) { D.fail(ST_UNSUP); return; }   // the Xml types (their toJSON is an XML string), an unknown typeRef
      if (sp + 2u >= D.cap_st) { D.fail(ST_NOMEM); return; }
      if (in_map) D.st[sp++] = T_MAP; else { D.st[sp++] = x; D.st[sp++] = T_ARR; }
      has = false;
      in_map = tref == 1;
      if (in_map) { o.b('{'); map_frame(D, u.type, sp); } else { o.b('['); x = D.ty[u.type].start; }
      continue;
    }
    // the end of the current type: close it and go on in its parent
    o.b(in_map ? '}' : ']');
    if (in_map) sp -= (uint32_t)D.st[sp - 2u] + 2u;
    if (!sp) return;
    in_map = D.st[--sp] == T_MAP;
    if (!in_map) x = D.st[--sp];
    has = true;
  }
}

// the JSON of root `name` of in[0, n) read as `kind`, over a workspace carved from ws, at most out_cap bytes at out.
// ST_JSON_MORE: out_len is the length a second run needs.  Pending structs / a pending delete set: the integrated
// part (ST_OK).
template <bool FLOATS = false>
YDEV_NI int tojson_run(const uint8_t* in, uint32_t n, uint32_t flags, uint8_t* ws, const snap::Caps& k, const uint8_t* name,
                       uint32_t name_len, uint32_t kind, uint8_t* out, uint32_t out_cap, uint32_t& out_len) {
  snap::Doc D;
  snap::carve(D, in, n, flags, ws, k, out, out_cap);
  out_len = 0;
  D.load();
  if (D.err) return D.err;
  snap::OutCap o{out, 0, out_cap};
  emit_tojson<FLOATS>(D, name, name_len, kind, o);
  if (D.err) return D.err;
  if (o.n >= JSON_MAX) return ST_NOMEM;
  out_len = o.n;
  return o.n > o.cap ? ST_JSON_MORE : ST_OK;
}
// document d's workspace from caps_of, its output region at the end (as json::json_doc)
template <bool FLOATS = false>
YDEV int tojson_doc(const uint8_t* in, uint32_t n, uint32_t flags, uint8_t* ws, const snap::Caps& k, const uint8_t* name, uint32_t name_len,
                    uint32_t kind, uint32_t& out_off, uint32_t& out_len) {
  out_off = (uint32_t)snap::ws_core_bytes(k);
  return tojson_run<FLOATS>(in, n, flags, ws, k, name, name_len, kind, ws + out_off, k.out, out_len);
}

}  // namespace tojson
}  // namespace ygm

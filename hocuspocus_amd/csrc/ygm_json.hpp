// ygm_json.hpp -- a stored document as ProseMirror / Tiptap JSON (ygm_json_v1, YGM_JSON_PROSEMIRROR):
//
//     utf8(JSON.stringify(yXmlFragmentToProsemirrorJSON(doc.getXmlFragment(name))))   doc = Y.applyUpdate(new Y.Doc(), state)
//
// y-prosemirror's function (what TiptapTransformer.fromYdoc(doc, name) returns), restated over yjs 13.5.16's own
// toArray / toDelta / getAttributes / nodeName:
//     serialize(XmlText)    = toDelta().map(d => {type:'text', text:d.insert, marks?: keys(d.attributes).map(k => {type:k, attrs:v})})
//     serialize(XmlElement) = {type:nodeName, attrs?: getAttributes() (>= 1 key), content?: toArray().map(serialize).flat() (toArray non-empty)}
//     result                = {type:'doc', content: fragment.toArray().map(serialize)}      (the top level is not flattened)
//   toArray        the list's live countable items
//   toDelta        along the list: a live ContentFormat flushes the pending string, then deletes (null) or sets its key
//                  in currentAttributes (a Map: a set of an existing key keeps its place, delete then set moves it to
//                  the end); live ContentStrings append to the pending string; a live ContentEmbed flushes and gives an
//                  op of its own; the end of the list flushes.  Ops are never merged, strings across deleted items are.
//   getAttributes  the type's map entries whose current item is not deleted: the last element of its ContentAny
//   key order      JavaScript's own-property order: canonical array-index keys ascending, then insertion order (the
//                  order the type's me[] entries were created in; currentAttributes' order)
// Any values are written by v2::any_json, format and embed values (canonical JSON text in V1) are copied.  The
// refusals (ST_UNSUP / ST_NONCANON) are include/ygm.h's table.  Like the text this is a last stage over parse,
// integrate_all and apply_ds of snap::Doc: no gc, no merge pass, no encoder, so neither F_COMPAT_135 nor gc matters.
//
// The marks Map lives in the workspace: Doc::tx (the transaction's delete set, dead after apply_ds) holds it as an
// ordered list of (key offset, key length, value offset, value length) into the input, searched linearly.  The walk's
// stack is Doc::st; an element's attribute entries are ordered on the free part of that stack.
// Output size: every op repeats the current marks, so the JSON is not bounded by Caps::out.  OutCap counts past its
// cap: json_run reports the needed length (ST_JSON_MORE) and the caller runs the document again into a region of
// that size (k_json's second launch; tools/snapdev/jsondev.cpp).
// ygm_json_fields_v1 -- every asked field of a document as one object keyed by field -- is the same load followed by
// emit_fields, which writes each field's root with the same walk (emit_root); see there.
#pragma once
#include "ygm_text.hpp"
#include "ygm_v2.hpp"

namespace ygm {
namespace json {

constexpr uint32_t KIND_PROSEMIRROR = 0u;   // YGM_JSON_PROSEMIRROR
constexpr int ST_JSON_MORE = 65;            // internal: the JSON needs out_len bytes (more than the region given)
constexpr uint32_t JSON_MAX = 0x80000000u;  // a JSON of 2^31 bytes or more: ST_NOMEM

YDEV void lit(snap::OutCap& o, const char* s) { while (*s) o.b((uint8_t)*s++); }
// the body of a JSON string as JSON.stringify escapes it (UTF-8 in, UTF-8 out: only ", \ and bytes below 0x20 change)
YDEV void esc(snap::OutCap& o, const uint8_t* s, uint32_t n) {
  const char* hx = "0123456789abcdef";
  for (uint32_t i = 0; i < n; i++) {
    if ((i & 0xFFFFFu) == 0xFFFFFu && o.n >= JSON_MAX) return;   // (the 32-bit count cannot wrap: checked every MiB)
    const uint8_t c = s[i];
    if (c == '"' || c == '\\') { o.b('\\'); o.b(c); }
    else if (c >= 0x20) o.b(c);
    else if (c == 8) { o.b('\\'); o.b('b'); } else if (c == 9) { o.b('\\'); o.b('t'); } else if (c == 10) { o.b('\\'); o.b('n'); }
    else if (c == 12) { o.b('\\'); o.b('f'); } else if (c == 13) { o.b('\\'); o.b('r'); }
    else { o.b('\\'); o.b('u'); o.b('0'); o.b('0'); o.b((uint8_t)hx[c >> 4]); o.b((uint8_t)hx[c & 15]); }
  }
}
YDEV void quoted(snap::OutCap& o, const uint8_t* s, uint32_t n) { o.b('"'); esc(o, s, n); o.b('"'); }
// canonical JSON text: does it hold a number JSON.stringify writes with a fraction or an exponent?
YDEV bool json_has_float(const uint8_t* s, uint32_t n) {
  bool in_str = false;
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t c = s[i];
    if (in_str) { if (c == '\\') i++; else if (c == '"') in_str = false; continue; }
    if (c == '"') { in_str = true; continue; }
    if (c == '-' || (c >= '0' && c <= '9')) {
      for (; i < n; i++) {
        const uint8_t d = s[i];
        if (d == '.' || d == 'e' || d == 'E') return true;
        if (!(d == '-' || d == '+' || (d >= '0' && d <= '9'))) { i--; break; }
      }
    }
  }
  return false;
}
// a mark name newer y-prosemirror versions rewrite (an overlapping-mark suffix "--" + 8 base64 characters)
YDEV bool hashed_mark(const uint8_t* k, uint32_t n) {
  if (n < 10 || k[n - 10] != '-' || k[n - 9] != '-') return false;
  for (uint32_t i = n - 8; i < n; i++) {
    const uint8_t c = k[i];
    if (!((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '+' || c == '/' || c == '=')) return false;
  }
  return true;
}

// FLOATS (a context opened with YGM_F_FLOATS; a compile-time option, so the other instantiations compile to what they
// were): attribute numbers go through any_json's FLOATS form, and mark and embed values are copied without the
// json_has_float refusal -- the state's parse has proven their numbers canonical (at most 15 significant digits, no
// exponent: what JSON.stringify writes), or the document carries ST_NONCANON from it already.
template <bool FLOATS>
struct Walk {
  snap::Doc& D;
  snap::OutCap& o;
  uint32_t n_mk;   // currentAttributes: D.tx[0, n_mk) as (client: key offset, clock: key length, len: value offset, pad: value length)

  YDEV bool mk_key_eq(uint32_t i, uint32_t ko, uint32_t kl) const { return D.key_eq(D.tx[i].client, D.tx[i].clock, ko, kl); }
  // updateCurrentAttributes of a live ContentFormat [c0, c1): key varstring, value varstring (JSON)
  YDEV void format(uint32_t c0, uint32_t c1) {
    Cur c{D.in, c0, c1, 0, 0};
    uint32_t kl, vl;
    const uint32_t ko = c.buf(kl), vo = c.buf(vl);
    if (c.err) { D.fail(ST_MALFORMED); return; }
    const bool null = vl == 4 && D.in[vo] == 'n' && D.in[vo + 1] == 'u' && D.in[vo + 2] == 'l' && D.in[vo + 3] == 'l';
    uint32_t i = 0;
    while (i < n_mk && !mk_key_eq(i, ko, kl)) i++;
    if (null) {
      if (i < n_mk) { for (uint32_t j = i + 1; j < n_mk; j++) D.tx[j - 1] = D.tx[j]; n_mk--; }
      return;
    }
    if (i == n_mk) {
      if (n_mk >= D.cap_tx) { D.fail(ST_NOMEM); return; }
      n_mk++;
      D.tx[i].client = ko; D.tx[i].clock = kl;
    }
    D.tx[i].len = vo; D.tx[i].pad = vl;
  }
  YDEV void mark(uint32_t i, bool& first) {
    const snap::Rng m = D.tx[i];
    if (hashed_mark(D.in + m.client, m.clock)) { D.fail(snap::ST_UNSUP); return; }
    if (!FLOATS && json_has_float(D.in + m.len, m.pad)) { D.fail(ST_NONCANON); return; }
    if (!first) o.b(',');
    first = false;
    lit(o, "{\"type\":"); quoted(o, D.in + m.client, m.clock); lit(o, ",\"attrs\":"); o.copy(D.in + m.len, m.pad); o.b('}');
  }
  // ,"marks":[...] of an op when currentAttributes is not empty: index keys ascending, then the Map's order
  YDEV void marks() {
    if (!n_mk) return;
    lit(o, ",\"marks\":[");
    bool first = true;
    uint64_t prev = 0; bool any_prev = false;
    for (;;) {   // (each round emits the smallest index key above the last: quadratic in the index keys only)
      uint64_t best = 0; int32_t bi = -1;
      for (uint32_t i = 0; i < n_mk; i++) {
        uint64_t v;
        if (!index_key(D.in + D.tx[i].client, D.tx[i].clock, v) || (any_prev && v <= prev)) continue;
        if (bi < 0 || v < best) { best = v; bi = (int32_t)i; }
      }
      if (bi < 0) break;
      mark((uint32_t)bi, first);
      prev = best; any_prev = true;
      if (D.err || o.n >= JSON_MAX) return;
    }
    for (uint32_t i = 0; i < n_mk && !D.err && o.n < JSON_MAX; i++) {
      uint64_t v;
      if (!index_key(D.in + D.tx[i].client, D.tx[i].clock, v)) mark(i, first);
    }
    o.b(']');
  }
  // one attribute: "key":value, the value the last element of the entry's current ContentAny item
  YDEV void attr(const snap::MapEnt& e, bool& first) {
    const snap::SI& u = D.it[e.item];
    if (u.ref != 8 || u.p1 < 0) { D.fail(snap::ST_UNSUP); return; }
    const snap::Piece q = D.pc[u.p1];
    Cur c{D.in, q.off, q.end, 0, 0};
    for (uint32_t k = 1; k < q.cnt && !c.err; k++) any_skip(c);
    if (c.err || c.pos >= c.end) { D.fail(ST_MALFORMED); return; }
    if (D.in[c.pos] == 127 || D.in[c.pos] == 116) { D.fail(snap::ST_UNSUP); return; }   // undefined, Uint8Array
    o.b(first ? '{' : ',');
    first = false;
    quoted(o, D.in + e.key_off, e.key_len); o.b(':');
    const int r = v2::any_json<snap::OutCap, false, FLOATS>(c, o);
    if (r) D.fail(r);
  }
  // ,"attrs":{...} of element type t when it has a live entry.  The entries go onto the free stack above sp (newest
  // first, as the type's list holds them) and are written index keys ascending, then oldest first.
  YDEV void attrs(int32_t t, uint32_t sp) {
    uint32_t k = 0, steps = 0;
    for (int32_t e = D.ty[t].map; e >= 0; e = D.me[e].next) {
      if (++steps > D.n_me) { D.fail(snap::ST_UNSUP); return; }
      const int32_t x = D.me[e].item;
      if (x < 0 || D.deleted(x)) continue;
      if (sp + k >= D.cap_st) { D.fail(ST_NOMEM); return; }
      D.st[sp + k++] = e;
    }
    if (!k) return;
    lit(o, ",\"attrs\":");
    bool first = true;
    uint64_t prev = 0; bool any_prev = false;
    for (;;) {
      uint64_t best = 0; int32_t bi = -1;
      for (uint32_t i = 0; i < k; i++) {
        const snap::MapEnt& e = D.me[D.st[sp + i]];
        uint64_t v;
        if (!index_key(D.in + e.key_off, e.key_len, v) || (any_prev && v <= prev)) continue;
        if (bi < 0 || v < best) { best = v; bi = (int32_t)i; }
      }
      if (bi < 0) break;
      attr(D.me[D.st[sp + bi]], first);
      prev = best; any_prev = true;
      if (D.err) return;
    }
    for (uint32_t i = k; i-- > 0 && !D.err;) {
      const snap::MapEnt& e = D.me[D.st[sp + i]];
      uint64_t v;
      if (!index_key(D.in + e.key_off, e.key_len, v)) attr(e, first);
    }
    o.b('}');
  }
};

// The walk.  Every loop is bounded as emit_text's: each list item is visited once and each type returned from once in
// a well-formed document (n_it + n_ty + 1 steps), a piece chain has at most n_pc pieces, a type's entries at most
// n_me.  A list that cycles exhausts the bound and ends in ST_UNSUP.  The stack holds the ContentType items the walk
// is inside of; what it needs on the way back (element or text) is read from the item again.
// {"type":"doc","content":[...]} of root type `root` (a ty[] index), -1: the empty document.  D.tx and D.st are the
// walk's alone and start empty: roots can be written one after another.
template <bool FLOATS = false>
YDEV void emit_root(snap::Doc& D, int32_t root, snap::OutCap& o) {
  using namespace snap;
  lit(o, "{\"type\":\"doc\",\"content\":[");
  if (root < 0) { lit(o, "]}"); return; }   // doc.getXmlFragment(name) of a name the update has no root for: an empty fragment
  Walk<FLOATS> W{D, o, 0};
  const uint64_t limit = (uint64_t)D.n_it + D.n_ty + 1u;
  uint64_t steps = 0;
  uint32_t sp = 0;
  bool in_text = false;   // the current list is an XmlText's
  bool opened = true;     // the current element's "content":[ is written (toArray() is not empty)
  bool has = false;       // the array being written has an entry
  bool str = false;       // an op's string is open (toDelta's pending str)
  int32_t x = D.ty[root].start;
  for (;;) {
    if (++steps > limit) { D.fail(ST_UNSUP); return; }
    if (D.err) return;
    if (o.n >= JSON_MAX) { D.fail(ST_NOMEM); return; }
    if (x < 0) {
      if (in_text) {
        if (str) { o.b('"'); W.marks(); o.b('}'); str = false; }
        if (sp == 1) { o.b(']'); has = true; }   // (directly under the fragment: an array of its own)
        in_text = false;
      } else {
        if (!sp) break;
        if (opened) o.b(']');
        o.b('}');
        has = true;
      }
      if (!sp) break;
      x = D.it[D.st[--sp]].right;
      opened = true;   // (the parent holds the type just left)
      continue;
    }
    const SI& u = D.it[x];
    if (u.kind != SK_ITEM || (u.flags & F_DEL)) { x = u.right; continue; }
    if (in_text) {
      if (u.ref == 4) {
        if (!str) { if (has) o.b(','); has = true; lit(o, "{\"type\":\"text\",\"text\":\""); str = true; }
        uint32_t np = 0;
        for (int32_t p = u.p0; p >= 0; p = D.pc[p].next) {
          if (++np > D.n_pc) { D.fail(ST_UNSUP); return; }
          const Piece q = D.pc[p];
          if (q.pre) { o.b(0xEF); o.b(0xBF); o.b(0xBD); }
          if (q.end > q.off) esc(o, D.in + q.off, q.end - q.off);
          if (q.post) { o.b(0xEF); o.b(0xBF); o.b(0xBD); }
          if (o.n >= JSON_MAX) { D.fail(ST_NOMEM); return; }
        }
      } else if (u.ref == 6) {
        if (str) { o.b('"'); W.marks(); o.b('}'); str = false; }
        W.format(u.c_start, u.c_end);
      } else if (u.ref == 5) {
        if (str) { o.b('"'); W.marks(); o.b('}'); str = false; }
        Cur c{D.in, u.c_start, u.c_end, 0, 0};
        uint32_t vl; const uint32_t vo = c.buf(vl);
        if (c.err) { D.fail(ST_MALFORMED); return; }
        if (!FLOATS && json_has_float(D.in + vo, vl)) { D.fail(ST_NONCANON); return; }
        if (has) o.b(',');
        has = true;
        lit(o, "{\"type\":\"text\",\"text\":"); o.copy(D.in + vo, vl); W.marks(); o.b('}');
      } else if (u.ref == 7) { D.fail(ST_UNSUP); return; }   // a type inside an XmlText
      x = u.right;
      continue;
    }
    // a fragment's or an element's list
    if (u.ref == 6) { x = u.right; continue; }   // (not countable: toArray skips it)
    if (u.ref != 7 || u.type < 0 || u.c_start >= u.c_end) { D.fail(ST_UNSUP); return; }
    const uint8_t tref = D.in[u.c_start];
    if (tref != 3 && tref != 6) { D.fail(ST_UNSUP); return; }
    if (!opened) { lit(o, ",\"content\":["); opened = true; has = false; }
    if (sp >= D.cap_st) { D.fail(ST_NOMEM); return; }
    D.st[sp++] = x;
    if (tref == 6) {
      if (sp == 1) { if (has) o.b(','); o.b('['); has = false; }   // (inside an element the ops join its content: flat())
      in_text = true; W.n_mk = 0; str = false;
    } else {
      Cur c{D.in, u.c_start + 1u, u.c_end, 0, 0};
      uint32_t nl; const uint32_t no = c.buf(nl);
      if (c.err) { D.fail(ST_MALFORMED); return; }
      if (has) o.b(',');
      lit(o, "{\"type\":"); quoted(o, D.in + no, nl);
      W.attrs(u.type, sp);
      opened = false; has = false;
    }
    x = D.ty[u.type].start;
  }
  lit(o, "]}");
}
template <bool FLOATS = false>
YDEV void emit_json(snap::Doc& D, const uint8_t* name, uint32_t name_len, uint32_t kind, snap::OutCap& o) {
  (void)kind;
  emit_root<FLOATS>(D, snap::find_root(D, name, name_len), o);
}

// ---- every asked field of a document as one object (ygm_json_fields_v1):
//     utf8(JSON.stringify(TiptapTransformer.fromYdoc(doc, fields)))      = { "<field>": <emit_root of that field>, ... }
// A field list is zero or more lib0 varStrings back to back.  No name: every key of doc.share -- the root types in
// ty[] order, which is the order yjs creates them in while it reads the structs (Doc::parse calls root_type where
// readClientsStructRefs calls doc.get).  The object's keys follow data[field] = ... assignments in list order:
// canonical array-index keys ascending, then the others by first assignment; a repeated name keeps its first place.
// data["__proto__"] = ... sets the prototype and the key vanishes: refused (ST_UNSUP) where the field stands in that
// order.  Nothing is kept per field: the list (or ty[]) is decoded again for every selection, as Walk::marks does over
// the marks Map, so the cost is quadratic in the names (at most FIELDS_MAX) and the workspace holds nothing new.
constexpr uint32_t FIELDS_MAX = 1024u;

// a well-formed field list: varuints minimal and of at most 5 bytes, lengths inside the list, names strict UTF-8 (they
// are written into the output), at most FIELDS_MAX names.  Anything else: ST_INVAL for the document.
YDEV int fields_check(const uint8_t* fl, uint32_t fn) {
  uint32_t pos = 0, count = 0;
  while (pos < fn) {
    uint64_t len = 0; uint32_t nb = 0; uint8_t r;
    do {
      if (pos >= fn || nb == 5) return ST_INVAL;
      r = fl[pos++];
      len |= (uint64_t)(r & 127) << (7 * nb++);
    } while (r & 128);
    if ((nb > 1 && r == 0) || len > (uint64_t)(fn - pos)) return ST_INVAL;
    if (utf8_u16(fl + pos, (uint32_t)len) < 0) return ST_INVAL;
    pos += (uint32_t)len;
    if (++count > FIELDS_MAX) return ST_INVAL;
  }
  return ST_OK;
}

// the asked fields in turn: the names of a checked list, or (an empty list) the document's root types
struct Fields {
  const snap::Doc& D;
  const uint8_t* fl; uint32_t fn;
  uint32_t pos;   // the list's byte position, or the ty[] index
  YDEV bool all() const { return fn == 0; }
  // the next field: its name, where it stands (list position / ty[] index) and its root type (-1: none)
  YDEV bool next(const uint8_t*& s, uint32_t& n, uint32_t& at, int32_t& root) {
    if (all()) {
      while (pos < D.n_ty && D.ty[pos].item != -1) pos++;
      if (pos >= D.n_ty) return false;
      at = pos; root = (int32_t)pos; s = D.in + D.ty[pos].name_off; n = D.ty[pos].name_len;
      pos++;
      return true;
    }
    if (pos >= fn) return false;
    at = pos;
    uint32_t len = 0, sh = 0; uint8_t r;
    do { r = fl[pos++]; len |= (uint32_t)(r & 127) << sh; sh += 7; } while (r & 128);   // (checked: ends inside the list)
    s = fl + pos; n = len; pos += len;
    root = -2;   // (looked up when the field is written)
    return true;
  }
  // list form: does the name stand in the list before position `at`?  (root types have one name each)
  YDEV bool before(uint32_t at, const uint8_t* s, uint32_t n) const {
    if (all()) return false;
    Fields f{D, fl, fn, 0};
    const uint8_t* t; uint32_t tn, ta; int32_t tr;
    while (f.next(t, tn, ta, tr) && ta < at) {
      if (tn != n) continue;
      uint32_t i = 0;
      while (i < n && t[i] == s[i]) i++;
      if (i == n) return true;
    }
    return false;
  }
};

template <bool FLOATS = false>
YDEV void emit_fields(snap::Doc& D, const uint8_t* fl, uint32_t fn, snap::OutCap& o) {
  Fields F{D, fl, fn, 0};
  bool first = true, index_pass = true, any_prev = false;
  uint64_t prev = 0;
  for (;;) {
    const uint8_t* s = nullptr; uint32_t n = 0, at = 0; int32_t root = -1;
    bool got = false;
    if (index_pass) {   // the smallest index key above the last one written (equal names give equal values: written once)
      uint64_t best = 0;
      const uint8_t* t; uint32_t tn, ta; int32_t tr;
      F.pos = 0;
      while (F.next(t, tn, ta, tr)) {
        uint64_t v;
        if (!index_key(t, tn, v) || (any_prev && v <= prev)) continue;
        if (!got || v < best) { best = v; s = t; n = tn; root = tr; got = true; }
      }
      if (got) { prev = best; any_prev = true; }
      else { index_pass = false; F.pos = 0; }
    }
    if (!index_pass) {   // then the other names, each where it stands first
      uint64_t v;
      while ((got = F.next(s, n, at, root)) && (index_key(s, n, v) || F.before(at, s, n))) {}
      if (!got) break;
    }
    if (n == 9) {
      const char* pr = "__proto__";
      uint32_t i = 0;
      while (i < 9 && s[i] == (uint8_t)pr[i]) i++;
      if (i == 9) { D.fail(snap::ST_UNSUP); return; }
    }
    o.b(first ? '{' : ',');
    first = false;
    quoted(o, s, n); o.b(':');
    if (o.n >= JSON_MAX) { D.fail(ST_NOMEM); return; }
    emit_root<FLOATS>(D, root == -2 ? snap::find_root(D, s, n) : root, o);
    if (D.err) return;
    if (o.n >= JSON_MAX) { D.fail(ST_NOMEM); return; }
  }
  if (first) o.b('{');
  o.b('}');
}

// the JSON of root `name` of in[0, n) over a workspace carved from ws, at most out_cap bytes at out.  ST_JSON_MORE:
// out_len is the length a second run needs.  Pending structs / a pending delete set: the integrated part (ST_OK).
// FIELDS: name[0, name_len) is a field list and the JSON the object of its fields (emit_fields); the state's own
// status comes before the list's.  FLOATS: the walk's FLOATS form (Walk).
template <bool FIELDS = false, bool FLOATS = false>
YDEV_NI int json_run(const uint8_t* in, uint32_t n, uint32_t flags, uint8_t* ws, const snap::Caps& k, const uint8_t* name,
                     uint32_t name_len, uint32_t kind, uint8_t* out, uint32_t out_cap, uint32_t& out_len) {
  snap::Doc D;
  snap::carve(D, in, n, flags, ws, k, out, out_cap);
  out_len = 0;
  D.load();
  if (D.err) return D.err;
  snap::OutCap o{out, 0, out_cap};
  if (FIELDS) {
    if (fields_check(name, name_len)) return ST_INVAL;
    emit_fields<FLOATS>(D, name, name_len, o);
  } else emit_json<FLOATS>(D, name, name_len, kind, o);
  if (D.err) return D.err;
  if (o.n >= JSON_MAX) return ST_NOMEM;
  out_len = o.n;
  return o.n > o.cap ? ST_JSON_MORE : ST_OK;
}
// document d's workspace from caps_of, its output region at the end (as text::text_doc)
template <bool FIELDS = false, bool FLOATS = false>
YDEV int json_doc(const uint8_t* in, uint32_t n, uint32_t flags, uint8_t* ws, const snap::Caps& k, const uint8_t* name, uint32_t name_len,
                  uint32_t kind, uint32_t& out_off, uint32_t& out_len) {
  out_off = (uint32_t)snap::ws_core_bytes(k);
  return json_run<FIELDS, FLOATS>(in, n, flags, ws, k, name, name_len, kind, ws + out_off, k.out, out_len);
}

}  // namespace json
}  // namespace ygm

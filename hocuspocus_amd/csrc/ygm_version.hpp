// ygm_version.hpp -- the cut of version history (Y.createDocFromSnapshot, yjs 13.5.16 Y@ createDocFromSnapshot):
//
//     restore(state, version) = snapshot( cut(S, version.sv) ++ version.ds )
//
// S is the no-GC snapshot of the state (ygm_snapshot.hpp with F_SNAP_NOGC | F_SNAP_STATE: client blocks descending,
// each from clock 0, no Skip), version the encoded Snapshot V1 (writeDeleteSet, then writeStateVector).  The reference
// splits the store's Items at the version's clocks (getItemCleanStart: Items only, a GC struct stays whole), writes per
// client with a clock k > 0 the structs below k (struct.write(encoder, 0): origin, rightOrigin, parent and parentSub
// as they are, the last one's content shortened by ContentX.splice) and appends the version's delete set; the engine
// then snapshots that update.  cut() is the byte-level part: one parse of S, no integration.
//
// The code is written for one wave per document with every value wave-uniform: W supplies the wave-wide pieces (the
// lookup of a client in the version's state vector and the store of an entry, the copy of a contiguous run) and the
// lane that stores single bytes.  HostW is the one-lane form (development harnesses, tools/snapdev/versiondev.cpp);
// the kernels' form is in ygm_version.hip.
#pragma once
#include "ygm_v1.hpp"

namespace ygm {
namespace ver {

constexpr int ST_UNSUP = 9;           // YGM_EUNSUPPORTED
constexpr uint32_t MAX_SV = 4096u;    // state-vector entries (and delete-set clients) of a version: the table's size
struct SvEnt { uint32_t client, clock; };

struct HostW {
  YDEV uint32_t lane() const { return 0; }
  YDEV int32_t find(const SvEnt* t, uint32_t n, uint32_t client) const {
    for (uint32_t i = 0; i < n; i++) if (t[i].client == client) return (int32_t)i;
    return -1;
  }
  YDEV void put(SvEnt* t, uint32_t i, uint32_t client, uint32_t clock) const { t[i].client = client; t[i].clock = clock; }
  YDEV void copy(uint8_t* d, const uint8_t* s, uint32_t n) const { for (uint32_t i = 0; i < n; i++) d[i] = s[i]; }
};

// the writer: single bytes by one lane, runs by the wave; stores stop at cap, n counts on (> cap: it did not fit)
template <class W>
struct WOut {
  W w; uint8_t* p; uint32_t n, cap;
  YDEV void b(uint8_t v) { if (n < cap && w.lane() == 0) p[n] = v; n++; }
  YDEV void vu(uint64_t v) { while (v > 127) { b((uint8_t)(0x80 | (v & 127))); v >>= 7; } b((uint8_t)v); }
  YDEV void run(const uint8_t* s, uint32_t len) { if (len && n <= cap && len <= cap - n) w.copy(p + n, s, len); n += len; }
};

// cut(S, version) into out (capacity cap >= sn + vn + 16); tbl: MAX_SV entries of scratch (LDS in the kernel).
// Returns a status; out_len is set when it is ST_OK.
//   truncated version                                   ST_MALFORMED     varuint above 2^53            ST_RANGE
//   non-minimal varuint in the version                  ST_NONCANON      (Y.encodeSnapshot never writes one)
//   a client repeated in its delete set / state vector  ST_NONCANON      (yjs would re-encode)
//   a version clock above the state's, or a client with a clock > 0 that S does not have    ST_INVAL (yjs throws)
//   more than MAX_SV state-vector entries or delete-set clients, a client id past 32 bits   ST_UNSUP
// Bytes after the state vector are ignored (decodeSnapshot ignores them).
template <class W>
YDEV_NI int cut_doc(const W& w, const uint8_t* S, uint32_t sn, const uint8_t* V, uint32_t vn, uint32_t flags, SvEnt* tbl, uint8_t* out,
                    uint32_t cap, uint32_t& out_len) {
  out_len = 0;
  // ---- the version: delete set (clients checked, copied verbatim at the end), then the state vector into tbl
  Cur v{V, 0, vn, 0, 0};
  bool dup = false, many = false, wide = false, high = false;
  uint32_t ne = 0;
  const uint64_t nd = v.vu();
  for (uint64_t q = 0; q < nd && !v.err; q++) {
    const uint64_t client = v.vu(), nr = v.vu();
    for (uint64_t r = 0; r < nr && !v.err; r++) { v.vu(); v.vu(); }
    if (v.err) break;
    if (client > 0xFFFFFFFFull) { wide = true; continue; }
    if (w.find(tbl, ne, (uint32_t)client) >= 0) dup = true;
    else if (ne >= MAX_SV) many = true;
    else { w.put(tbl, ne, (uint32_t)client, 0u); ne++; }
  }
  const uint32_t ds_end = v.pos;
  ne = 0;
  uint32_t nk = 0;   // clients kept: clock > 0
  const uint64_t nsv = v.err ? 0 : v.vu();
  for (uint64_t i = 0; i < nsv && !v.err; i++) {
    const uint64_t client = v.vu(), clock = v.vu();
    if (v.err) break;
    if (client > 0xFFFFFFFFull) { wide = true; continue; }
    if (w.find(tbl, ne, (uint32_t)client) >= 0) { dup = true; continue; }
    if (ne >= MAX_SV) { many = true; continue; }
    if (clock > 0xFFFFFFFFull) high = true;
    w.put(tbl, ne, (uint32_t)client, clock > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)clock); ne++;
    nk += clock > 0 ? 1u : 0u;
  }
  if (v.err) return v.err;
  if (v.nm || dup) return ST_NONCANON;
  if (many || wide) return ST_UNSUP;
  if (high) return ST_INVAL;

  // ---- S: one walk; a kept block's verbatim structs and the header of a cut one are one contiguous run
  WOut<W> o{w, out, 0, cap};
  o.vu(nk);
  Cur c{S, 0, sn, 0, 0};
  uint32_t matched = 0;
  const uint64_t nb = c.vu();
  for (uint64_t b = 0; b < nb && !c.err; b++) {
    const uint64_t ns = c.vu(), client = c.vu(), clock0 = c.vu();
    if (c.err) break;
    if (clock0 != 0 || client > 0xFFFFFFFFull) return ST_UNSUP;   // (not a snapshot's block)
    const int32_t ix = w.find(tbl, ne, (uint32_t)client);
    const uint64_t k = ix >= 0 ? tbl[ix].clock : 0u;
    const uint32_t first = c.pos;
    uint64_t clock = 0, m = 0, l_clock = 0, l_len = 0;
    uint32_t l_cstart = first, l_end = first;
    uint8_t l_kind = K_GC, l_ref = 0;
    for (uint64_t s = 0; s < ns && !c.err; s++) {
      SInfo si; read_struct_fast(c, si, flags);
      if (c.err) break;
      if (si.kind == K_SKIP) return ST_UNSUP;
      if (clock < k) { m++; l_clock = clock; l_len = si.len; l_cstart = si.cstart; l_end = si.end; l_kind = si.kind; l_ref = si.ref; }
      clock += si.len;
    }
    if (c.err) break;
    if (k > clock) return ST_INVAL;   // the version is ahead of the state
    if (k == 0) continue;             // absent from the version, or clock 0: dropped
    matched++;
    o.vu(m); o.vu(client); o.vu(0);
    if (!(l_kind == K_ITEM && l_clock + l_len > k)) { o.run(S + first, l_end - first); continue; }   // (a straddled GC stays whole)
    o.run(S + first, l_cstart - first);
    const uint64_t t = k - l_clock;   // units kept, 0 < t < l_len
    Cur q{S, l_cstart, l_end, 0, 0};
    if (l_ref == 1) o.vu(t);
    else if (l_ref == 4) {   // ContentString.splice: UTF-16 units; a cut pair ends the kept text with U+FFFD
      uint32_t l; const uint32_t s0 = q.buf(l);
      if (q.err) return ST_MALFORMED;
      bool mid; const uint32_t e = u16_to_byte(S + s0, l, t, mid);
      if (mid) { o.vu((uint64_t)(e - 4u) + 3u); o.run(S + s0, e - 4u); o.b(0xEF); o.b(0xBF); o.b(0xBD); }
      else { o.vu(e); o.run(S + s0, e); }
    } else if (l_ref == 2 || l_ref == 8) {   // ContentJSON / ContentAny: the first t elements
      q.vu();
      const uint32_t s0 = q.pos;
      for (uint64_t e = 0; e < t && !q.err; e++) { if (l_ref == 2) { uint32_t l; q.buf(l); } else any_skip(q); }
      if (q.err || q.pos > l_end) return ST_MALFORMED;
      o.vu(t); o.run(S + s0, q.pos - s0);
    } else return ST_UNSUP;   // (other content has length 1)
  }
  if (c.err) return c.err;
  if (matched != nk) return ST_INVAL;   // a version client with a clock that S does not have
  o.run(V, ds_end);
  if (o.n > cap) return ST_NOMEM;
  out_len = o.n;
  return ST_OK;
}

}  // namespace ver
}  // namespace ygm

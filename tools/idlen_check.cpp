// idlen_check.cpp -- the lean merge kernel's fast parse with the client id's length built in (lean_parse_fast<., true>
// of hocuspocus_amd/csrc/ygm_merge_lean.hpp) against the generic instantiation, on the CPU (tooling).  Both are
// transcribed here whole, with the device builtins modelled as the ISA defines them (v_alignbyte_b32 takes its count
// modulo 4, v_bfe_u32 offset and width modulo 32, v_dot4_u32_u8 sums the four byte products), and compared in
// everything they return -- fast, the record (client, clock, clen, span), hasd -- on every input that passes the
// kernel's test of an update (lean_id5_ok: no structs, or bytes 2 .. 5 with the top bit and byte 6 without), with the
// lane holding an update or not and the row's parent-key branch taken or not.  Also checked: from seven bytes on that
// test is ((T >> 2) & 0x1F) == 0x10 on the terminator mask.
//
// Windows: 01 01, a five-byte id, a clock of 1 .. 6 bytes, then the info byte and two bytes after it, the rest and the
// mask bits past the 16-byte window random.  Coverage: every value of the id's fifth byte at every update length
// 0 .. 32 (a value with the top bit set fails the test and is only counted); the ids 2^28, 2^28 + 1, 0x7FFFFFFF,
// 0x80000000, 0xFFFFFFFF and 2^24 random ones (--quick: 2^16), each with every clock length; every value of the info
// byte and of each of the two bytes after it at every clock length (the bytes whose position depends on p); and 2^22
// whole updates of the fast shape (see there), which are the items among the compared.
// Prints the counts; exit status 1 when there is a mismatch.
//
//     g++ -O2 -std=c++17 -pthread -o idlen_check idlen_check.cpp && ./idlen_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <thread>
#include <vector>

static uint32_t ubfe(uint32_t x, uint32_t off, uint32_t width) {
  off &= 31u; width &= 31u;
  return width ? (x >> off) & ((1u << width) - 1u) : 0u;
}
static uint32_t udot4(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) r += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
  return r;
}
static uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * (s & 3u))); }
static uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
static uint32_t lnctz(uint32_t x) { return (uint32_t)__builtin_ctz(x | 0x80000000u); }
static uint32_t pext28(uint32_t x, uint32_t n) {
  const uint32_t m = ubfe(x, 0u, umin(8u * n, 31u)) & 0x7f7f7f7fu;
  return udot4(m, 0x00008001u) | (udot4(m, 0x80010000u) << 14);
}
static uint32_t pext28_full(uint32_t x) {
  const uint32_t m = x & 0x7f7f7f7fu;
  return udot4(m, 0x00008001u) | (udot4(m, 0x80010000u) << 14);
}
static uint32_t lean_vu_over5(uint32_t n) { return (n + 2u) >> 3; }

struct Out {
  bool fast, hasd;
  uint32_t client, clock, clen, span;
  bool operator==(const Out& o) const {
    return fast == o.fast && hasd == o.hasd && client == o.client && clock == o.clock && clen == o.clen && span == o.span;
  }
};
// lean_parse_fast, ID5 as in the header.  key: KEYROW, or another lane of the row brought the parent-key branch in
// (the function's ballot, of which this lane's own part is valid && nsk == 0); tl / td: the bytes n - 3 and n - 1
template <bool ID5>
static Out parse_fast(const uint32_t (&d)[4], uint32_t H, uint32_t Z, uint32_t tl, uint32_t td, uint32_t s, uint32_t n, bool valid, bool key) {
  const uint32_t V = 0xFFFFFFFFu >> ((32u - n) & 31u);
  const uint32_t T = ~H & V, HV = H & V;
  const uint32_t h2 = HV & (HV >> 1), h4 = h2 & (h2 >> 2), h7 = h4 & (h4 >> 3);
  uint32_t bad = h7 | (Z & (HV << 1) & V);
  const uint32_t b0 = d[0] & 0xFFu, b1 = (d[0] >> 8) & 0xFFu;
  bad |= (b0 ^ 1u) | (b1 ^ 1u);
  uint32_t e = ID5 ? 6u : 2u + lnctz(T >> 2);
  const uint32_t cl_n = e - 1u;
  const uint32_t cl_y = ID5 || cl_n >= 5u ? (d[1] >> 16) & 0xFFu : 0u;
  const uint32_t cl_x = alignbyte(d[1], d[0], 2u);
  const uint32_t client = (ID5 ? pext28_full(cl_x) : pext28(cl_x, cl_n)) | (cl_y << 28);
  bad |= (ID5 ? 0u : lean_vu_over5(cl_n)) | (cl_y & 0x70u);
  const uint32_t p = e + 1u;
  const uint32_t pc = p < 31u ? p : 31u;
  e = pc + lnctz(T >> pc);
  const uint32_t ck_n = e - p + 1u;
  const uint64_t U01 = ((uint64_t)d[1] << 32) | d[0], U23 = ((uint64_t)d[3] << 32) | d[2];
  const uint64_t cw = ID5 ? ((uint64_t)alignbyte(d[3], d[2], 3u) << 32) | alignbyte(d[2], d[1], 3u)
                          : (U01 >> (8u * (p & 7u))) | (p & 7u ? (U23 << (64u - 8u * (p & 7u))) : 0ull);
  const uint32_t ck_y = ck_n >= 5u ? (uint32_t)(cw >> 32) & 0xFFu : 0u;
  const uint32_t clock = pext28((uint32_t)cw, ck_n) | (ck_y << 28);
  bad |= lean_vu_over5(ck_n) | (ck_y & 0x70u);
  bad |= clock == 0xFFFFFFFFu ? 1u : 0u;
  const uint32_t ip = e + 1u;
  const uint32_t x3 = (uint32_t)(cw >> (8u * (ck_n & 7u)));
  const uint32_t info = x3 & 0xFFu;
  const uint32_t nsk = ((info >> 6) & 1u) + ((info >> 7) & 1u);
  const uint32_t pp = ip + 1u < 31u ? ip + 1u : 31u;
  const uint32_t t0 = (T >> pp) | 0x80000000u, t1 = t0 & (t0 - 1u), t2 = t1 & (t1 - 1u), t3 = t2 & (t2 - 1u);
  const uint32_t pl = nsk == 2u ? pp + lnctz(t3) + 1u : pp + lnctz(t1) + 1u;
  bool fits = pl + 3u == n;
  bool shape = nsk != 0u && (info & 0x3Fu) == 4u;
  if (key || (valid && nsk == 0u)) {
    const uint32_t lk = (x3 >> 16) & 0xFFu;
    const uint32_t kp = ip + 3u < 31u ? ip + 3u : 31u;
    const bool par = x3 << 16 == 0x01040000u && lk < 32u && ((HV >> kp) & ((1u << (lk & 31u)) - 1u)) == 0u;
    fits = nsk == 0u ? ip + 6u + lk == n : fits;
    shape = shape || (nsk == 0u && par);
  }
  const bool item = bad == 0u && shape && fits && n <= 32u && tl == 1u && ((HV >> ((n - 2u) & 31u)) & 1u) == 0u;
  const bool dsonly = b0 == 0u && n >= 2u && n <= 32u;
  const uint32_t im = item ? 0xFFFFFFFFu : 0u;
  Out o;
  o.client = client & im; o.clock = clock & im; o.clen = 1u & im;
  o.span = (((s + ip) << 16) | (1u << 8) | ((n - 1u - ip) & 0xFFu)) & im;
  o.hasd = item ? td != 0u : b1 != 0u;
  o.fast = item || dsonly;
  return o;
}
// the test the kernel asks of every update (lean_id5_ok), and its reading on the terminator mask, which holds from
// seven bytes on
static bool id5_ok(const uint32_t (&d)[4], uint32_t H) { return (d[0] & 0xFFu) == 0u || ((H >> 2) & 0x1Fu) == 0x0Fu; }
static bool id5_on_T(const uint32_t (&d)[4], uint32_t H, uint32_t n) {
  const uint32_t T = ~H & (0xFFFFFFFFu >> ((32u - n) & 31u));
  return (d[0] & 0xFFu) == 0u || ((T >> 2) & 0x1Fu) == 0x10u;
}

struct Rng {
  uint64_t s;
  uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
};
struct Tally { uint64_t cases = 0, skipped = 0, bad = 0, items = 0; };

// one window: 01 01, the id's five bytes, a clock of ck_n bytes (ck: its 7-bit groups), then tail[]; H / Z of the
// window's bytes, the mask bits past it from hi16; compared at the update length n
static void one(Tally& t, const uint8_t (&id)[5], uint32_t ck_n, uint64_t ck, const uint8_t (&tail)[3], uint32_t fill, uint32_t hi16,
                uint32_t n) {
  uint8_t w[16];
  for (int i = 0; i < 16; i++) w[i] = (uint8_t)(fill >> (8 * (i & 3)));
  w[0] = 1; w[1] = 1;
  memcpy(w + 2, id, 5);
  uint32_t q = 7;
  for (uint32_t i = 0; i < ck_n && q < 16; i++, q++) w[q] = (uint8_t)(((ck >> (7 * i)) & 0x7F) | (i + 1 < ck_n ? 0x80u : 0u));
  for (int i = 0; i < 3 && q < 16; i++, q++) w[q] = tail[i];
  uint32_t d[4], H = hi16 << 16, Z = 0;
  memcpy(d, w, 16);
  for (int i = 0; i < 16; i++) { H |= (uint32_t)(w[i] >> 7) << i; Z |= (uint32_t)(w[i] == 0) << i; }
  const bool ok = id5_ok(d, H);
  if (n >= 7u && n <= 32u && ok != id5_on_T(d, H, n)) t.bad++;
  if (!ok) { t.skipped++; return; }
  // the bytes n - 3 and n - 1 where the window holds them, else from the fill; a staged position; the lane with and
  // without an update; the parent-key branch brought in by the row or not
  const uint32_t tl = n >= 3u && n - 3u < 16u ? w[n - 3u] : fill & 3u, td = n >= 1u && n - 1u < 16u ? w[n - 1u] : (fill >> 8) & 1u;
  const uint32_t s = (fill >> 16) & 0xFFFu;
  for (int v = 0; v < 2; v++)
    for (int key = 0; key < 2; key++) {
      t.cases++;
      if (!(parse_fast<true>(d, H, Z, tl, td, s, n, v != 0, key != 0) == parse_fast<false>(d, H, Z, tl, td, s, n, v != 0, key != 0))) t.bad++;
    }
}
// a whole update of the fast shape (u[0 .. n), n <= 32; bytes past it: the next update's, random): the window, the
// masks of all 32 bytes and the tail bytes as the kernel loads them.  cut: the same bytes at a shorter length too
static void whole(Tally& t, const uint8_t* u, uint32_t n, uint32_t s) {
  uint32_t d[4], H = 0, Z = 0;
  memcpy(d, u, 16);
  for (int i = 0; i < 32; i++) { H |= (uint32_t)(u[i] >> 7) << i; Z |= (uint32_t)(u[i] == 0) << i; }
  if (!id5_ok(d, H)) { t.skipped++; return; }
  const uint32_t tl = u[(n > 3u ? n : 3u) - 3u], td = u[(n > 3u ? n : 3u) - 1u];
  for (int v = 0; v < 2; v++)
    for (int key = 0; key < 2; key++) {
      const Out a = parse_fast<true>(d, H, Z, tl, td, s, n, v != 0, key != 0), b = parse_fast<false>(d, H, Z, tl, td, s, n, v != 0, key != 0);
      t.cases++;
      t.items += a.fast && a.clen;
      if (!(a == b)) t.bad++;
    }
}
static uint32_t put_vu(uint8_t* p, uint64_t v, uint32_t nb) {   // v in exactly nb bytes (minimal when v's top group is non-zero)
  for (uint32_t i = 0; i < nb; i++) p[i] = (uint8_t)(((v >> (7 * i)) & 0x7F) | (i + 1 < nb ? 0x80u : 0u));
  return nb;
}
static void id_bytes(uint32_t v, uint8_t (&id)[5]) {
  for (int i = 0; i < 4; i++) id[i] = (uint8_t)(((v >> (7 * i)) & 0x7F) | 0x80u);
  id[4] = (uint8_t)(v >> 28);
}

int main(int argc, char** argv) {
  const bool quick = argc > 1 && !strcmp(argv[1], "--quick");
  const unsigned hc = std::thread::hardware_concurrency(), nt = hc == 0 ? 4 : hc > 16 ? 16 : hc;
  const uint32_t n_rand = quick ? 1u << 16 : 1u << 24;
  std::atomic<uint64_t> cases{0}, skipped{0}, bad{0}, items{0};
  std::vector<std::thread> th;
  for (unsigned ti = 0; ti < nt; ti++)
    th.emplace_back([&, ti] {
      Tally t;
      Rng r{0x9E3779B97F4A7C15ull * (ti + 1)};
      uint8_t id[5], tail[3], u[48];
      // random ids (the first five of thread 0: the edges), every clock length, a random update length and n = 32
      const uint32_t edge[5] = {1u << 28, (1u << 28) + 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
      for (uint32_t i = ti; i < n_rand; i += nt) {
        id_bytes(i < 5 ? edge[i] : (r.next() | (1u << 28)), id);
        for (uint32_t ck_n = 1; ck_n <= 6; ck_n++) {
          const uint64_t ck = ((uint64_t)r.next() << 32 | r.next()) | (1ull << (7 * (ck_n - 1)));   // (a minimal varuint: top group non-zero)
          for (int j = 0; j < 3; j++) tail[j] = (uint8_t)r.next();
          const uint32_t fill = r.next(), hi16 = r.next() & 0xFFFFu;
          one(t, id, ck_n, ck, tail, fill, hi16, r.next() % 33u);
          one(t, id, ck_n, ck, tail, fill, hi16, 32u);
          one(t, id, ck_n, i & 1 ? ~0ull : ck, tail, fill, 0u, 7u + ck_n + 3u);   // the update ends with the tail; every other one: all clock bits set
        }
      }
      // every value of the fifth byte on 256 ids per thread, every clock length, every update length
      for (uint32_t i = ti; i < (quick ? 64u : 1024u); i += nt) {
        id_bytes(r.next(), id);
        for (uint32_t y = 0; y < 256; y++) {
          id[4] = (uint8_t)y;
          for (uint32_t ck_n = 1; ck_n <= 6; ck_n++) {
            for (int j = 0; j < 3; j++) tail[j] = (uint8_t)r.next();
            const uint64_t ck = ((uint64_t)r.next() << 32 | r.next()) | (1ull << (7 * (ck_n - 1)));
            for (uint32_t n = 0; n <= 32; n++) one(t, id, ck_n, ck, tail, r.next(), r.next() & 0xFFFFu, n);
          }
        }
      }
      // every value of the info byte and of each of the two bytes after it, at every clock length
      for (uint32_t i = ti; i < (quick ? 64u : 1024u); i += nt) {
        id_bytes(r.next() | (1u << 28), id);
        for (uint32_t ck_n = 1; ck_n <= 6; ck_n++)
          for (int pos = 0; pos < 3; pos++)
            for (uint32_t b = 0; b < 256; b++) {
              for (int j = 0; j < 3; j++) tail[j] = (uint8_t)r.next();
              tail[pos] = (uint8_t)b;
              const uint64_t ck = ((uint64_t)r.next() << 32 | r.next()) | (1ull << (7 * (ck_n - 1)));
              one(t, id, ck_n, ck, tail, r.next(), r.next() & 0xFFFFu, 32u);
              one(t, id, ck_n, ck, tail, r.next(), 0u, 7u + ck_n + 3u);
            }
      }
      // whole updates of the fast shape: an origin, a right origin, both (ids of 1 .. 5 and clocks of 1 .. 3 bytes), the
      // parent key of 1 .. 8 characters; document clocks of 1 .. 5 bytes and 0xFFFFFFFF; at their length, one byte
      // shorter and longer, and cut below seven bytes (bits 2 .. 6 of the mask then belong to what follows)
      for (uint32_t i = ti; i < n_rand / 4u; i += nt) {
        for (int j = 0; j < 48; j++) u[j] = (uint8_t)r.next();
        u[0] = 1; u[1] = 1;
        id_bytes(i < 5 ? edge[i] : (r.next() | (1u << 28)), id);
        memcpy(u + 2, id, 5);
        const uint32_t ck_n = 1u + i % 5u;
        uint64_t ck = (r.next() & ((1ull << (7 * ck_n)) - 1ull)) | (1ull << (7 * (ck_n - 1)));
        if (ck_n == 5u) ck = i % 3u == 0 ? 0xFFFFFFFFull : i % 3u == 1 ? 0xFFFFFFFEull : ck & 0xFFFFFFFFull;
        uint32_t q = 7u + put_vu(u + 7, ck, ck_n);
        const uint32_t kind = (i / 5u) % 4u;
        if (kind == 3u) {
          const uint32_t lk = 1u + (i / 20u) % 8u;
          u[q++] = 0x04; u[q++] = 1; u[q++] = (uint8_t)lk;
          for (uint32_t j = 0; j < lk; j++) u[q++] = (uint8_t)('a' + j);
        } else {
          u[q++] = (uint8_t)(kind == 0 ? 0x84 : kind == 1 ? 0x44 : 0xC4);
          for (uint32_t j = 0; j < (kind == 2u ? 2u : 1u); j++) {
            const uint32_t ob = 1u + (i / 20u + j) % 5u, kb = 1u + (i / 100u + j) % 3u;
            if (q + ob + kb + 3u > 32u) break;
            q += put_vu(u + q, r.next() | (1ull << (7 * (ob - 1))), ob);
            u[q - 1] &= 0x0F | (ob < 5u ? 0x70 : 0);
            q += put_vu(u + q, r.next() | (1ull << (7 * (kb - 1))), kb);
          }
        }
        u[q++] = 1; u[q++] = (uint8_t)('a' + i % 26u); u[q++] = (uint8_t)(i % 7u == 0);
        if (q > 32u) continue;
        const uint32_t s = r.next() & 0xFFFu;
        whole(t, u, q, s); whole(t, u, q - 1u, s); whole(t, u, q < 32u ? q + 1u : q, s);
        whole(t, u, i % 7u, s);
      }
      cases += t.cases; skipped += t.skipped; bad += t.bad; items += t.items;
    });
  for (auto& x : th) x.join();
  printf("{\"compared\": %llu, \"of_them_items\": %llu, \"failing_the_id_test\": %llu, \"mismatches\": %llu}\n", (unsigned long long)cases.load(),
         (unsigned long long)items.load(), (unsigned long long)skipped.load(), (unsigned long long)bad.load());
  return bad.load() ? 1 : 0;
}

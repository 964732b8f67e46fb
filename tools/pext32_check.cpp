// pext32_check.cpp -- the lean merge kernel's varuint value (pext32 of hocuspocus_amd/csrc/ygm_merge_lean.hpp) against
// the shift ladder it replaced, on the CPU (tooling).  The device function is a bit-field extract and two dot products
// of bytes; both are modelled here as the ISA defines them (v_bfe_u32 takes offset and width modulo 32, a width of 0
// gives 0; v_dot4_u32_u8 sums the four byte products).
//
// Every x of 2^32 for every length n = 0 .. 5 (the function reads n as min(8 n, 31) and n >= 5 only), every n = 6 .. 32
// and the small negative lengths an invalid lane can bring (n = -1 .. -8, wrapped) on 2^24 random x and x of every
// continuation pattern, every fifth byte y.  Prints the number of mismatches; exit status 1 when there is one.
//
//     g++ -O3 -pthread -o pext32_check pext32_check.cpp && ./pext32_check
#include <cstdint>
#include <cstdio>
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
static uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// the ladder: mask to n bytes, drop the top bits, close the gaps in three steps
static uint32_t pext32_ladder(uint32_t x, uint32_t y, uint32_t n) {
  x &= n >= 4u ? 0xFFFFFFFFu : ((1u << (8u * n)) - 1u);
  x &= 0x7f7f7f7fu;
  x = ((x >> 1) & 0x3f803f80u) | (x & 0x007f007fu);
  x = ((x >> 2) & 0x0fffc000u) | (x & 0x00003fffu);
  return x | (n >= 5u ? (y & 0x7Fu) << 28 : 0u);
}
// the kernel's
static uint32_t pext32_dot(uint32_t x, uint32_t y, uint32_t n) {
  const uint32_t m = ubfe(x, 0u, umin(8u * n, 31u)) & 0x7f7f7f7fu;
  const uint32_t lo = udot4(m, 0x00008001u), hi = udot4(m, 0x80010000u);
  return (lo | (hi << 14)) | (n >= 5u ? (y & 0x7Fu) << 28 : 0u);
}
// the fast parse's: the fifth byte taken once where there is one, no mask on it (the shift drops its bits 4 .. 7)
static uint32_t pext32_fast(uint32_t x, uint32_t y, uint32_t n) {
  const uint32_t y5 = n >= 5u ? y & 0xFFu : 0u;
  const uint32_t m = ubfe(x, 0u, umin(8u * n, 31u)) & 0x7f7f7f7fu;
  return (udot4(m, 0x00008001u) | (udot4(m, 0x80010000u) << 14)) | (y5 << 28);
}

int main() {
  const unsigned nt = std::thread::hardware_concurrency() ? std::thread::hardware_concurrency() : 4;
  std::atomic<uint64_t> bad{0}, done{0};
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; t++)
    th.emplace_back([&, t] {
      uint64_t b = 0, c = 0;
      // every x, n = 0 .. 5 (y = 0x5A and 0xFF: the value's top bits come from y's low four only)
      for (uint64_t x = t; x < (1ull << 32); x += nt)
        for (uint32_t n = 0; n <= 5; n++)
          for (uint32_t y : {0x5Au, 0xFFu}) {
            const uint32_t want = pext32_ladder((uint32_t)x, y, n);
            b += pext32_dot((uint32_t)x, y, n) != want;
            b += pext32_fast((uint32_t)x, y, n) != want;
            c++;
          }
      // every n = 0 .. 32 and -8 .. -1, every y, on random x and on every continuation pattern of x
      uint64_t s = 0x9E3779B97F4A7C15ull * (t + 1);
      for (uint32_t i = 0; i < (1u << 24) / nt + 16; i++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        uint32_t x = (uint32_t)(s >> 16);
        if (i < 16) x = (x & 0x7f7f7f7fu) | ((i & 1) << 7) | ((i & 2) << 14) | ((i & 4) << 21) | ((i & 8) << 28);
        for (int n = -8; n <= 32; n++)
          for (uint32_t y = (i & 7u); y < 256; y += 8) {
            const uint32_t want = pext32_ladder(x, y, (uint32_t)n);
            b += pext32_dot(x, y, (uint32_t)n) != want;
            b += pext32_fast(x, y, (uint32_t)n) != want;
            c++;
          }
      }
      bad += b; done += c;
    });
  for (auto& x : th) x.join();
  printf("{\"cases\": %llu, \"mismatches\": %llu}\n", (unsigned long long)done.load(), (unsigned long long)bad.load());
  return bad.load() ? 1 : 0;
}
